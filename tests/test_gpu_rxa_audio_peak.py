"""xcbl / xspeak / xmpeak in the batched RXA engine (RXA.c:591-593) against the restatement (tests/rxa_audio_peak_ref.py).

The three stages apply one real filter to I and Q alike after the AGC, so with a constant panel, fixed gain and out_rate == dsp_rate
they commute with the panel's 2x2 matrix: the engine's output with a stage on equals the restated stage applied to the output of an
engine with the same settings and the stage off (that engine's chain is pinned to the oracle by test_gpu_rxa_parity.py).  Where a test
changes the panel or the fixed gain between calls, the stage-off engine runs with the panel at identity and the panel is applied per
call behind the restated stages.  Tolerance: 1e-9 relative RMS, the chain's own bound.  -m gpu."""
import ctypes as C

import numpy as np
import pytest

from conftest import rel_rms
from quisk_amd import synth
from rxa_audio_peak_ref import AudioPeakChain, panel

pytestmark = pytest.mark.gpu

CALLS = (3, 1, 17, 19, 80)             # blocks of 1024 input samples (192 k -> 48 k, 256 per block); 80 takes the time tiles of the AGC
TOL = 1e-9


def _engine(qh, nch, modes, dsp_rate=48000, passband=(300.0, 3000.0)):
    e = qh.RxaEngine(nch, dsp_rate=dsp_rate, out_rate=dsp_rate)
    for c in range(nch):
        e.SetRXAShiftRun(c, 1); e.SetRXAShiftFreq(c, synth.shift_freq(c)); e.RXANBPSetRun(c, 1)
        e.SetRXAMode(c, modes[c])
        pb = (-8000.0, 8000.0) if modes[c] == 5 else (-4000.0, 4000.0) if modes[c] in (6, 10) else \
            (-passband[1], -passband[0]) if modes[c] in (0, 3, 7) else passband
        e.RXASetPassband(c, *pb)
    return e


def _input(nch, n, modes):
    x = synth.make_input_numpy(nch, n)
    for c, m in enumerate(modes):
        if m in (6, 10):
            x[c] = synth.make_mode_input_numpy("am", c, n)
        elif m == 5:
            x[c] = synth.make_mode_input_numpy("fm", c, n)
    return x


class _Both:
    """the stage settings go to the engine and to the channel's restatement"""

    def __init__(self, e, refs):
        self.e, self.refs = e, refs

    def __getattr__(self, name):
        def call(c, *a):
            getattr(self.e, name)(c, *a)
            getattr(self.refs[c], name)(*a)
        return call


SETTINGS = [
    lambda s, c: s.SetRXASPCWRun(c, 1),
    lambda s, c: (s.SetRXASPCWFreq(c, 800.0), s.SetRXASPCWBandwidth(c, 50.0), s.SetRXASPCWGain(c, 1.5), s.SetRXASPCWRun(c, 1)),
    lambda s, c: s.SetRXAmpeakRun(c, 1),
    lambda s, c: (s.SetRXAmpeakFilFreq(c, 0, 1000.0), s.SetRXAmpeakFilBw(c, 0, 100.0), s.SetRXAmpeakFilFreq(c, 1, 1400.0),
                  s.SetRXAmpeakFilBw(c, 1, 60.0), s.SetRXAmpeakFilGain(c, 1, 2.0), s.SetRXAmpeakRun(c, 1)),
    lambda s, c: s.SetRXACBLRun(c, 1),
    lambda s, c: (s.SetRXACBLRun(c, 1), s.SetRXASPCWFreq(c, 700.0), s.SetRXASPCWRun(c, 1), s.SetRXAmpeakRun(c, 1)),
    lambda s, c: None,
]


def _run(qh, modes, settings, calls=CALLS, dsp_rate=48000, between=None, prep=None, ident_panel=False):
    """(outputs of the engine with the stages, outputs of the stage-off engine, restatements) call by call"""
    nch = len(modes)
    a, b = _engine(qh, nch, modes, dsp_rate), _engine(qh, nch, modes, dsp_rate)
    if prep:
        prep(a); prep(b)
    if ident_panel:
        b.SetRXAPanelGain1(-1, 1.0)
    refs = [AudioPeakChain(float(dsp_rate)) for _ in range(nch)]
    both = _Both(a, refs)
    for c in range(nch):
        settings[c](both, c)
    x = _input(nch, sum(calls) * a.dsp_insize, modes)
    ya, yb, yr = [], [], []
    pos = 0
    try:
        for k, nb in enumerate(calls):
            if between:
                between(k, a, b, both, refs)
            xa = np.ascontiguousarray(x[:, pos:pos + nb * a.dsp_insize])
            pa, pb = a.process_host(xa), b.process_host(xa)
            ya.append(pa); yb.append(pb)
            yr.append(np.stack([refs[c].process(pb[c]) for c in range(nch)]))
            pos += nb * a.dsp_insize
    finally:
        a.close(); b.close()
    return np.concatenate(ya, 1), np.concatenate(yb, 1), np.concatenate(yr, 1)


def _check(ya, yr, chans, tol=TOL):
    for c in chans:
        r = rel_rms(ya[c], yr[c])
        assert r < tol, (c, r)


def test_stages_against_restatement_usb_ragged(qh):
    modes = [1] * 7
    ya, yb, yr = _run(qh, modes, SETTINGS)
    _check(ya, yr, range(7))
    assert np.array_equal(ya[6], yb[6])                        # the channel without a stage: bit for bit


def test_every_detector_mode(qh):
    # USB, AM + CBL, FM + SPEAK, SAM + MPEAK, LSB + all, CWU, DIGU, FM and USB without a stage (FM beside USB: the two-stream split path)
    modes = [1, 6, 5, 10, 0, 4, 9, 5, 1]
    st = [SETTINGS[0], SETTINGS[4], SETTINGS[1], SETTINGS[2], SETTINGS[5], SETTINGS[1], SETTINGS[3], SETTINGS[6], SETTINGS[6]]
    ya, yb, yr = _run(qh, modes, st)
    _check(ya, yr, range(9))
    assert np.array_equal(ya[7], yb[7]) and np.array_equal(ya[8], yb[8])


def test_second_dsp_rate(qh):
    ya, _, yr = _run(qh, [1] * 6, SETTINGS[:6], calls=(2, 5, 9), dsp_rate=96000)
    _check(ya, yr, range(6))


def test_setters_between_calls(qh):
    """flushing setters zero their cascade only; run / enable / npeaks freeze and resume; no peak -> exact zeros; flush() all"""
    modes = [1] * 6
    st = [SETTINGS[0], SETTINGS[0], SETTINGS[2], SETTINGS[3], SETTINGS[4], SETTINGS[5]]
    zero_calls = {}

    def between(k, a, b, s, refs):
        if k == 1:
            s.SetRXASPCWFreq(0, 900.0); s.SetRXAmpeakFilBw(2, 1, 120.0); s.SetRXASPCWRun(1, 0); s.SetRXACBLRun(4, 0)
        elif k == 2:
            s.SetRXASPCWRun(1, 1); s.SetRXAmpeakFilEnable(2, 0, 0); s.SetRXAmpeakNpeaks(3, 1); s.SetRXACBLRun(4, 1)
            s.SetRXAmpeakFilEnable(5, 0, 0); s.SetRXAmpeakFilEnable(5, 1, 0); zero_calls[5] = 2
        elif k == 3:
            s.SetRXAmpeakFilEnable(2, 0, 1); s.SetRXAmpeakNpeaks(3, 2); s.SetRXASPCWBandwidth(0, 70.0)
            s.SetRXAmpeakFilEnable(5, 0, 1); s.SetRXAmpeakFilEnable(5, 1, 1); s.SetRXAmpeakNpeaks(5, 0); zero_calls[5] = 3
            s.SetRXAmpeakFilGain(3, 0, 0.5); s.SetRXASPCWGain(5, 3.0)
        elif k == 4:
            s.SetRXAmpeakNpeaks(5, 2)
            a.flush(); b.flush()
            for r in refs:
                r.flush()

    ya, _, yr = _run(qh, modes, st, between=between)
    _check(ya, yr, range(6))
    starts = np.cumsum((0,) + CALLS) * 256
    for c, k in ((5, 2), (5, 3)):
        assert not np.any(ya[c, starts[k]:starts[k + 1]]), (c, k)


def test_fixed_gain_and_panel_changes_reach_only_new_samples(qh):
    """a 50 Hz wide SPEAK rings over call boundaries while SetRXAAGCFixed, SetRXAPanelGain1 and SetRXAPanelCopy change"""
    modes = [1] * 3
    st = [lambda s, c: (s.SetRXASPCWBandwidth(c, 50.0), s.SetRXASPCWRun(c, 1)),
          lambda s, c: (s.SetRXASPCWBandwidth(c, 50.0), s.SetRXASPCWRun(c, 1), s.SetRXACBLRun(c, 1)),
          lambda s, c: None]
    pan = [dict(gain1=4.0, copy=0) for _ in range(3)]
    calls = (3, 4, 2, 5, 3, 6)

    def prep(e):
        e.SetRXAAGCMode(-1, 0); e.SetRXAAGCFixed(-1, 20.0)

    def between(k, a, b, s, refs):
        if k in (1, 3, 5):
            g = (20.0, 6.0, 30.0, 12.0, 0.0, 26.0)[k]
            a.SetRXAAGCFixed(-1, g); b.SetRXAAGCFixed(-1, g)
            p = dict(gain1=(4.0, 2.5, 4.0, 0.5, 1.0, 3.0)[k], copy=(0, 1, 0, 3, 0, 2)[k])
            for c in range(3):
                a.SetRXAPanelGain1(c, p["gain1"]); a.SetRXAPanelCopy(c, p["copy"])
                pan[c] = p
        seen.append([dict(p) for p in pan])

    seen = []
    ya, yb, yr = _run(qh, modes, st, calls=calls, between=between, prep=prep, ident_panel=True)
    starts = np.cumsum((0,) + calls) * 256
    for c in range(3):
        ref = np.concatenate([panel(yr[c, starts[k]:starts[k + 1]], **seen[k][c]) for k in range(len(calls))])
        r = rel_rms(ya[c], ref)
        assert r < TOL, (c, r)


def test_with_other_features(qh):
    """AGC mode 3 (time tiles in the 80-block call), ANF and bp1 at position 1, meters: the agc meter reads the same"""
    modes = [1] * 4
    st = [SETTINGS[0], SETTINGS[5], SETTINGS[3], SETTINGS[4]]

    def prep(e):
        e.SetRXAANFRun(1, 1); e.SetRXAANFPosition(1, 1)
        e.SetRXAANFRun(3, 1); e.SetRXAANFPosition(3, 0)
        e.enable_meters(True)

    meters = []

    def between(k, a, b, s, refs):
        if k:
            meters.append([(a.GetRXAMeter(c, 5), b.GetRXAMeter(c, 5), a.GetRXAMeter(c, 6), b.GetRXAMeter(c, 6)) for c in range(4)])

    ya, _, yr = _run(qh, modes, st, between=between, prep=prep)
    _check(ya, yr, range(4))
    for row in meters:
        for pa, pb, va, vb in row:
            assert pa == pb and va == vb


def test_i16_egress_and_graph_replay(qh):
    import torch
    dev = torch.device("cuda:0")
    nch, nblk = 4, 8
    modes = [1] * nch
    a, b = _engine(qh, nch, modes), _engine(qh, nch, modes)
    refs = [AudioPeakChain(48000.0) for _ in range(nch)]
    both = _Both(a, refs)
    for c, f in enumerate((SETTINGS[0], SETTINGS[2], SETTINGS[5], SETTINGS[6])):
        f(both, c)
    from quisk_amd.rxa import AudioFormat
    fmt = AudioFormat("i16", volume=2.0 ** 28)      # (short)(int)(volume x / 65536): 4096 x
    a.set_graph_replay(True); b.set_graph_replay(True)
    ncall = 12
    x = synth.make_input_numpy(nch, ncall * nblk * 1024)
    d_in = torch.zeros((nch, nblk * 1024), dtype=torch.complex128, device=dev)
    d_a = torch.zeros((nch, nblk * 256), dtype=torch.complex128, device=dev)
    d_b = torch.zeros((nch, nblk * 256), dtype=torch.complex128, device=dev)
    ya, yr = [], []
    try:
        for k in range(ncall):
            if k == 6:
                both.SetRXASPCWFreq(0, 750.0); both.SetRXAmpeakFilGain(1, 1, 1.7)
            d_in.copy_(torch.from_numpy(np.ascontiguousarray(x[:, k * nblk * 1024:(k + 1) * nblk * 1024])))
            a.process_ptr(d_in.data_ptr(), nblk * 1024, d_a.data_ptr(), nblk * 256, nblk)
            b.process_ptr(d_in.data_ptr(), nblk * 1024, d_b.data_ptr(), nblk * 256, nblk)
            torch.cuda.synchronize()
            pb = d_b.cpu().numpy()
            ya.append(d_a.cpu().numpy())
            yr.append(np.stack([refs[c].process(pb[c]) for c in range(nch)]))
        assert a.graph_launches() > 0
        ya, yr = np.concatenate(ya, 1), np.concatenate(yr, 1)
        _check(ya, yr, range(nch))
    finally:
        a.close(); b.close()
    # i16 audio frames: a fresh engine's first call through qh_rxa_process_audio against the complex output of the first call above
    # narrowed by qh_audio_pack
    e = _engine(qh, nch, modes)
    both = _Both(e, [AudioPeakChain(48000.0) for _ in range(nch)])
    for c, f in enumerate((SETTINGS[0], SETTINGS[2], SETTINGS[5], SETTINGS[6])):
        f(both, c)
    try:
        d_pcm = torch.zeros((nch, nblk * 256 * 2), dtype=torch.int16, device=dev)
        d_ref = torch.zeros_like(d_pcm)
        d_in.copy_(torch.from_numpy(np.ascontiguousarray(x[:, :nblk * 1024])))
        e.process_audio_ptr(d_in.data_ptr(), nblk * 1024, d_pcm.data_ptr(), nblk * 256 * 4, nblk, fmt)
        src = torch.from_numpy(np.ascontiguousarray(ya[:, :nblk * 256])).to(dev)
        torch.cuda.synchronize()
        lib = qh.load()
        assert lib.qh_audio_pack(0, None, src.data_ptr(), nblk * 256, nch, nblk * 256, C.byref(fmt), d_ref.data_ptr(), nblk * 256 * 4) == 0
        torch.cuda.synchronize()
        pcm, ref = d_pcm.cpu().numpy().astype(np.int32), d_ref.cpu().numpy().astype(np.int32)
        assert np.any(pcm != 0) and np.max(np.abs(pcm - ref)) <= 1
    finally:
        e.close()


def test_untouched_engine_is_bit_identical(qh):
    """new setters with run 0 (and designs) on one engine, none on the other: same output bits, device bytes and replays"""
    import torch
    dev = torch.device("cuda:0")
    nch, nblk = 3, 4
    modes = [1] * nch
    a, b = _engine(qh, nch, modes), _engine(qh, nch, modes)
    a.SetRXACBLRun(-1, 0); a.SetRXASPCWRun(-1, 0); a.SetRXAmpeakRun(-1, 0); a.SetRXASPCWFreq(1, 900.0)
    a.SetRXAmpeakFilBw(-1, 1, 80.0); a.SetRXAmpeakNpeaks(2, 1); a.SetRXAmpeakFilEnable(0, 0, 0)
    x = synth.make_input_numpy(nch, 10 * nblk * 1024)
    d_in = torch.zeros((nch, nblk * 1024), dtype=torch.complex128, device=dev)
    outs = [torch.zeros((nch, nblk * 256), dtype=torch.complex128, device=dev) for _ in range(2)]
    try:
        for e in (a, b):
            e.set_graph_replay(True)
        for k in range(10):
            d_in.copy_(torch.from_numpy(np.ascontiguousarray(x[:, k * nblk * 1024:(k + 1) * nblk * 1024])))
            for e, o in zip((a, b), outs):
                e.process_ptr(d_in.data_ptr(), nblk * 1024, o.data_ptr(), nblk * 256, nblk)
            torch.cuda.synchronize()
            assert torch.equal(outs[0], outs[1]), k
        assert a.device_bytes() == b.device_bytes()
        assert a.graph_launches() == b.graph_launches() > 0
    finally:
        a.close(); b.close()


def test_invalid_index_is_refused_and_changes_nothing(qh):
    modes = [1, 1]
    a, b = _engine(qh, 2, modes), _engine(qh, 2, modes)
    lib = qh.load()
    for e in (a, b):
        e.SetRXAmpeakRun(-1, 1)
    for bad in (lambda: lib.qh_rxa_SetRXAmpeakNpeaks(a._h, -1, 3), lambda: lib.qh_rxa_SetRXAmpeakNpeaks(a._h, 0, -1),
                lambda: lib.qh_rxa_SetRXAmpeakFilEnable(a._h, 0, 2, 1), lambda: lib.qh_rxa_SetRXAmpeakFilFreq(a._h, -1, -1, 500.0),
                lambda: lib.qh_rxa_SetRXAmpeakFilBw(a._h, 1, 2, 10.0), lambda: lib.qh_rxa_SetRXAmpeakFilGain(a._h, 0, 5, 3.0)):
        assert bad() == -2                                      # QH_ERR_INVALID
    x = synth.make_input_numpy(2, 6 * 1024)
    try:
        assert np.array_equal(a.process_host(x), b.process_host(x))
    finally:
        a.close(); b.close()
