"""A display bank attached to the RXA engine (qh_rxa_attach_display): xsender -> Spectrum2 (sender.c:66-86) bank to bank on the device.

(1) plumbing: the rows the attached bank publishes are bit for bit those of a second bank, same settings, fed from the host with the
downloaded sender rows of the same calls and swap_iq = 1 -- the same kernels on the same floats.  (2) against the reference: oracle.
OracleAnalyzer fed block by block through Spectrum0 with the oracle's signal behind nbp0 in the chain's own (I, Q) order, which Spectrum0
reads swapped as Spectrum2 does; the gates of tests/test_gpu_analyzer.py (every pixel within one mlog10 step of 0.0022 dB, at most 2 % of
the pixels more than 1e-4 dB apart).  (3) refusals.  -m gpu."""
import numpy as np
import pytest

from rxa_taps_util import ARGS, BF, CALLS, DSP_RATE, MODES, NPIX, OVERLAP, SIZE, capture, compare_rows, engine, oracle_channel, oracle_rows, signal

pytestmark = pytest.mark.gpu


def _bank(qh, ndisp, bf=BF):
    g = qh.AnalyzerBank(ndisp, SIZE)
    g.SetDisplaySampleRate(DSP_RATE)
    args = list(ARGS); args[5] = bf
    g.SetAnalyzer(*args)
    return g


def test_attached_bank_against_host_fed_bank_and_oracle(qh, oracle):
    x = signal(MODES, sum(CALLS) * 1024, seed=1)
    e, g, h = engine(qh, MODES), _bank(qh, 5), _bank(qh, 5)
    try:
        e.attach_display(g, 0)
        got, fed, pos = [], [], 0
        for nb in CALLS:
            before = g.frames()
            e.process_host(np.ascontiguousarray(x[:, pos:pos + nb * 1024]))
            rows = np.stack([e.sender_rows_host(c) for c in range(5)])
            nf = h.feed_host(0, rows.astype(np.complex128), swap_iq=1)
            assert g.frames() - before == nf, (nb, g.frames() - before, nf)
            if nf:
                a, b = g.rows_host(0), h.rows_host(0)
                assert a.shape == (5, nf, NPIX) and np.array_equal(a, b), nb
                got.append(a)
            fed.append(rows)
            pos += nb * 1024
        got = np.concatenate(got, 1)
        assert got.shape[1] == (sum(CALLS) * 256 - SIZE) // (SIZE - OVERLAP) + 1
        fed = np.concatenate(fed, 1)
        for c, m in enumerate(MODES):
            o = oracle_channel(oracle, c, m, nbp_only=True)
            z = capture(o, oracle.WdspChannel.HOOK_FMSQ, x[c])[0]
            o.close()
            want = oracle_rows(oracle, z)
            assert want.max() > -30.0, c                    # the tones are in the passband: the display shows a signal
            # which of the two the reference's pixels depend on: the same bank fed from the host with np.float32 of the oracle's signal
            # differs from the attached bank's rows only by the input's last-bit differences, not by the plumbing
            k = _bank(qh, 1)
            k.feed_host(0, z.astype(np.complex64).astype(np.complex128)[None, :], swap_iq=1)
            d = np.abs(k.rows_host(0)[0].astype(np.float64) - want)
            k.close()
            print("channel", c, "host-fed with float32 of the oracle's signal: max", d.max(), "share above 1e-4 dB", np.mean(d > 1e-4))
            compare_rows(got[c], want, ("channel", c))
    finally:
        e.attach_display(None)
        e.close(); g.close(); h.close()


def test_refusals_and_detach(qh):
    x = signal(MODES, 8 * 1024, seed=9)
    e, g = engine(qh, MODES), _bank(qh, 5)
    four, narrow = _bank(qh, 4), _bank(qh, 5, bf=128)
    lib = qh.load()
    try:
        assert lib.qh_rxa_attach_display(e._h, four._h, 0) == -2            # QH_ERR_INVALID: a display per channel
        assert lib.qh_rxa_attach_display(e._h, narrow._h, 0) == -2          # buff_size is not dsp_size
        assert lib.qh_rxa_attach_display(e._h, g._h, 1) == -2               # no such sub-span
        e.attach_display(g, 0)
        assert lib.qh_rxa_set_sender(e._h, 1, 0) == -2                      # the display reads every channel's rows
        e.process_host(np.ascontiguousarray(x[:, :4 * 1024]))
        n = g.frames()
        assert n == 1
        e.attach_display(None)
        e.process_host(np.ascontiguousarray(x[:, 4 * 1024:]))
        assert g.frames() == n
        assert lib.qh_rxa_set_sender(e._h, 1, 0) == 0
    finally:
        e.close(); g.close(); four.close(); narrow.close()
