"""Every FM channel of an RXA engine with its own de-emphasis and audio filters (SetRXAFMAFFilter, SetRXAFMNCde / MPde / NCaud / MPaud,
wdsp/fmd.c:278-384) against the composed reference of tests/rxa_fm_filters_ref.py, one reference per channel.  -m gpu.

Engines: dsp_size 64, rates 48000 / 48000 / 48000 unless said, calls of 4096 to 16384 samples, AGC mode 0 at 0 dB.  The gate is the
project's 1e-6 relative RMS; every test prints what it measured.  "Bit for bit" is np.array_equal.

Bit identity and the paired tile.  Two FM channels with the same de-emphasis design share a tile (real part / imaginary part of one
transform), so a channel's last bits hang on its PARTNER's samples and on which half it sits in, through the rounding of the shared
transform (tests/test_gpu_channel_isolation.py measures that coupling and says why; here: 2.7e-12 on a peak of 8.3).  A channel left
over pairs with itself.  So "channel 0 bit for bit that of an engine where channel 1's design is another" can hold only where channel
0's tile is the same in both engines.  In the two-designs case the comparison engine gets its rows in the order that makes channel 0's
partner the same signal.  In the RXASetNC case channel 0 loses its partner to the setter, whatever the setter sets: it is bit for bit the
same under two different settings of channel 1 (nothing of the other channel's SETTINGS reaches it), and against the engine where nothing
was set -- where it shares a tile with channel 1 -- it moves by the rounding of that tile, measured, printed and held to the project's
gate.  Either way every channel is held to its reference, before and behind the setter."""
import numpy as np
import pytest

from conftest import rel_rms
from rxa_chain_ref import keyed_fm_over_a_floor
from rxa_fm_filters_ref import BAND_A, BAND_B, FM, RxaFmRef, fm_tone

pytestmark = pytest.mark.gpu

TOL = 1e-6
USB, AM = 1, 6
SIZE, RATE = 64, 48000
CALLS = (64, 128, 256)                  # blocks of 64: 4096, 8192 and 16384 samples


def _signal(c, n, rate=RATE):
    return fm_tone(n, rate, carrier=(-1500.0, 700.0, 0.0, 2100.0, -400.0, 900.0, 300.0)[c % 7], tone=700.0 + 150.0 * c, dev=2500.0 + 100.0 * c,
                   amp=0.3, seed=40 + c, sigma=0.002)


class Bank:
    """an engine and one reference per channel; a setter goes to both"""

    def __init__(self, qh, modes, size=SIZE, rates=(RATE, RATE, RATE), refs=True):
        self.e = qh.RxaEngine(len(modes), dsp_size=size, in_rate=rates[0], dsp_rate=rates[1], out_rate=rates[2])
        self.refs = [RxaFmRef(self.e.dsp_insize, size, *rates) for _ in modes] if refs else []
        self.modes = list(modes)
        for c, m in enumerate(modes):
            self.set("SetRXAMode", c, m)
            self.set("RXASetPassband", c, *((300.0, 3000.0) if m == USB else (-8000.0, 8000.0)))
            self.set("SetRXAAGCMode", c, 0)
            self.set("SetRXAAGCFixed", c, 0.0)

    def set(self, name, c, *a):
        getattr(self.e, name)(c, *a)
        if self.refs:
            getattr(self.refs[c], name)(*a)

    def call(self, x):
        y = self.e.process_host(x)
        r = np.stack([ref.xrxa(x[c]) for c, ref in enumerate(self.refs)]) if self.refs else None
        return y, r

    def run(self, x, calls=CALLS, between=None):
        ys, rs, pos = [], [], 0
        for k, nb in enumerate(calls):
            if between:
                between(k, self)
            n = nb * self.e.dsp_insize
            y, r = self.call(np.ascontiguousarray(x[:, pos:pos + n]))
            ys.append(y); rs.append(r)
            pos += n
        return np.concatenate(ys, 1), (np.concatenate(rs, 1) if self.refs else None)

    def close(self):
        self.e.close()
        for r in self.refs:
            r.close()


def _input(nch, calls=CALLS, size=SIZE, rate=RATE):
    n = sum(calls) * size
    return np.stack([_signal(c, n, rate) for c in range(nch)])


def _held(y, r, what, chans=None):
    for c in (range(y.shape[0]) if chans is None else chans):
        err = rel_rms(y[c], r[c])
        print("%s: channel %d against its reference, relative RMS %.3g" % (what, c, err))
        assert np.max(np.abs(r[c])) > 1e-4, (what, c)
        assert err < TOL, (what, c, err)


def test_two_designs_odd_counts(qh):
    """five FM channels with bands A, B, A, B, A beside a USB and an AM channel: the sort by design, one equal pair per design, a
    self-pair.  Channel 0 bit for bit that of an engine in which all five run A (its rows ordered so that channel 0 keeps its partner)."""
    modes = [FM] * 5 + [USB, AM]
    x = _input(7)
    b = Bank(qh, modes)
    for c in (1, 3):
        b.set("SetRXAFMAFFilter", c, *BAND_B)
    y, r = b.run(x)
    assert b.e.debug_fm_rows()[:2] == (2, 2)
    b.close()
    _held(y, r, "two designs")
    a = Bank(qh, modes, refs=False)
    ya, _ = a.run(x[[0, 2, 1, 3, 4, 5, 6]])         # pairs (0, 1), (2, 3), (4, 4) there: channel 1 carries channel 2's signal
    assert a.e.debug_fm_rows()[:2] == (1, 1)
    a.close()
    assert np.array_equal(y[0], ya[0])
    assert np.array_equal(y[5], ya[5]) and np.array_equal(y[6], ya[6])


def test_nc_de_differs_from_nc_aud(qh):
    b = Bank(qh, [FM, FM])
    b.set("SetRXAFMNCde", 0, 256)
    b.set("SetRXAFMNCaud", 0, 1024)
    y, r = b.run(_input(2))
    b.close()
    _held(y, r, "nc_de 256, nc_aud 1024")


@pytest.mark.parametrize("nc0,nc1", [(512, 2048), (2048, 4096), (2048, 8192)])
def test_different_nc_across_channels(qh, nc0, nc1):
    """(2048, 4096): 8192-point tiles; (2048, 8192): the partitioned form, two partitions on one row and one on the other"""
    b = Bank(qh, [FM, FM, FM])
    for c, nc in ((0, nc0), (1, nc1), (2, nc0)):
        b.set("SetRXAFMNCde", c, nc)
        b.set("SetRXAFMNCaud", c, nc)
    y, r = b.run(_input(3))
    b.close()
    _held(y, r, "nc %d beside %d" % (nc0, nc1))


@pytest.mark.parametrize("tile", [8192, 6144])
def test_two_designs_on_the_other_band_tiles(qh, tile):
    """the two-lane-group 8192 form and the 6144 plan read the design row too (qh_rxa_set_band_tile)"""
    b = Bank(qh, [FM, FM, FM, USB])
    b.e.set_band_tile(tile)
    b.set("SetRXAFMAFFilter", 1, *BAND_B)
    b.set("SetRXAFMNCaud", 2, 1024)
    y, r = b.run(_input(4))
    assert b.e.band_tile() == tile and b.e.debug_fm_rows()[:2] == (2, 3)
    b.close()
    _held(y, r, "band tile %d" % tile)


def test_minimum_phase_per_filter_and_per_channel(qh):
    """channel 0: mp_de 1, mp_aud 0; channel 1: linear phase; channel 2: mp_de 0, mp_aud 1"""
    b = Bank(qh, [FM, FM, FM])
    b.set("SetRXAFMMPde", 0, 1)
    b.set("SetRXAFMMPaud", 2, 1)
    y, r = b.run(_input(3))
    b.close()
    _held(y, r, "mp")


def test_af_filter_in_mid_stream_keeps_both_lines(qh):
    b = Bank(qh, [FM, FM])
    y, r = b.run(_input(2), between=lambda k, s: s.set("SetRXAFMAFFilter", 1, *BAND_B) if k == 1 else None)
    b.close()
    _held(y, r, "SetRXAFMAFFilter in mid-stream")
    lo = CALLS[0] * SIZE
    _held(y[:, lo:lo + 2048], r[:, lo:lo + 2048], "the 2048 samples behind the change")


def test_nc_de_in_mid_stream_zeroes_the_de_emphasis_line_only(qh):
    b = Bank(qh, [FM, FM])
    y, r = b.run(_input(2), between=lambda k, s: s.set("SetRXAFMNCde", 1, 1024) if k == 1 else None)
    b.close()
    _held(y, r, "SetRXAFMNCde in mid-stream")
    lo = CALLS[0] * SIZE
    _held(y[:, lo:lo + 2048], r[:, lo:lo + 2048], "the 2048 samples behind the change")


def test_the_same_value_set_twice_changes_no_bit(qh):
    x = _input(2)
    outs = []
    for twice in (False, True):
        b = Bank(qh, [FM, FM], refs=False)

        def between(k, s):
            if k == 1 or (k == 2 and twice):
                s.set("SetRXAFMAFFilter", 1, *BAND_B)
                s.set("SetRXAFMNCde", 1, 1024)
                s.set("SetRXAFMMPaud", 1, 1)
        outs.append(b.run(x, between=between)[0])
        b.close()
    assert np.array_equal(outs[0], outs[1])


def test_rxasetnc_on_one_of_two_fm_channels(qh):
    """no longer fails the engine; both channels held to their references.  Channel 0 is bit for bit the same whether channel 1 is set
    to 1024 or to 512 taps (in both it has lost its partner); against the engine where nothing was set, where the two share a tile, it
    moves by that tile's rounding (see the module's note): printed, and far inside the gate."""
    x = _input(2)
    b = Bank(qh, [FM, FM])
    y, r = b.run(x, between=lambda k, s: s.set("RXASetNC", 1, 1024) if k == 1 else None)
    b.close()
    _held(y, r, "RXASetNC(1, 1024)")
    outs = {}
    for nc in (1024, 512, None):
        e = Bank(qh, [FM, FM], refs=False)
        outs[nc] = e.run(x, between=lambda k, s: s.set("RXASetNC", 1, nc) if (k == 1 and nc) else None)[0]
        e.close()
    assert np.array_equal(outs[1024], y)
    assert np.array_equal(outs[1024][0], outs[512][0])
    assert not np.array_equal(outs[1024][1], outs[512][1])
    first = CALLS[0] * SIZE
    assert np.array_equal(outs[1024][0][:first], outs[None][0][:first])            # ahead of the setter: the same engine
    worst = np.max(np.abs(outs[1024][0] - outs[None][0]))
    print("channel 0 without its partner against channel 0 beside it: max %.3e on a peak of %.3g, relative RMS %.3g"
          % (worst, np.max(np.abs(outs[None][0])), rel_rms(outs[1024][0], outs[None][0])))
    assert rel_rms(outs[1024][0], outs[None][0]) < TOL


def test_defaults_set_explicitly_change_nothing(qh):
    x = _input(3)
    outs, nbytes = [], []
    for explicit in (False, True):
        b = Bank(qh, [FM, FM, USB], refs=False)
        if explicit:
            for c in range(3):
                b.set("SetRXAFMAFFilter", c, 300.0, 3000.0)
                b.set("SetRXAFMNCde", c, 2048); b.set("SetRXAFMNCaud", c, 2048)
                b.set("SetRXAFMMPde", c, 0); b.set("SetRXAFMMPaud", c, 0)
        outs.append(b.run(x)[0])
        nbytes.append(b.e.device_bytes())
        assert b.e.debug_fm_rows() == (1, 1, 2)
        b.close()
    assert np.array_equal(outs[0], outs[1])
    assert nbytes[0] == nbytes[1], nbytes


def test_ctcss_notch_and_fmsq_beside_another_band(qh):
    calls = (128, 192, 192)
    n = sum(calls) * SIZE
    x = np.stack([keyed_fm_over_a_floor(n, RATE, seed=3 + c) for c in range(2)])
    b = Bank(qh, [FM, FM])
    b.set("SetRXAFMAFFilter", 1, *BAND_B)
    for c in range(2):
        b.set("SetRXACTCSSRun", c, 1)
        b.set("SetRXAFMSQRun", c, 1)
    y, r = b.run(x, calls=calls)
    for c, ref in enumerate(b.refs):
        print("channel %d: squelch margins %s, cycles %s" % (c, ref.margins(), ref.cycles()))
        assert ref.margins_ok(), (c, ref.margins())
        assert ref.cycles()["fmsq"] >= 1, (c, ref.cycles())
    b.close()
    _held(y, r, "CTCSS notch and FMSQ")


def test_refusals(qh):
    from quisk_amd import QuiskHipError
    x = _input(2, calls=(64, 64))
    n = 64 * SIZE
    b = Bank(qh, [FM, FM], refs=False)
    a = Bank(qh, [FM, FM], refs=False)
    y0, ya0 = b.e.process_host(x[:, :n]), a.e.process_host(x[:, :n])
    assert np.array_equal(y0, ya0)
    bad = [("SetRXAFMNCde", (1000,)), ("SetRXAFMNCaud", (32,)), ("SetRXAFMNCde", (131072,)), ("SetRXAFMAFFilter", (float("nan"), 3000.0)),
           ("SetRXAFMAFFilter", (300.0, float("inf"))), ("SetRXAFMAFFilter", (0.0, 3000.0)), ("SetRXAFMAFFilter", (-5.0, 3000.0)),
           ("SetRXAFMAFFilter", (3000.0, 3000.0)), ("SetRXAFMAFFilter", (3000.0, 300.0))]
    for name, args in bad:
        with pytest.raises(QuiskHipError, match="error -2"):
            getattr(b.e, name)(1, *args)
    assert np.array_equal(b.e.process_host(x[:, n:]), a.e.process_host(x[:, n:]))
    # a band up to the Nyquist frequency: accepted by the setter, refused by the next call, nothing run
    b.e.SetRXAFMAFFilter(1, 300.0, 22000.0)
    with pytest.raises(QuiskHipError, match="error -3"):
        b.e.process_host(x[:, :n])
    b.e.SetRXAFMAFFilter(1, 300.0, 3000.0)
    assert np.array_equal(b.e.process_host(x[:, :n]), a.e.process_host(x[:, :n]))
    # xfmsq's shared noise filter: different nc among its channels is still refused
    for c in range(2):
        b.e.SetRXAFMSQRun(c, 1)
    b.e.SetRXAFMSQNC(1, 1024)
    with pytest.raises(QuiskHipError, match="FMSQ channels with different nc or mp"):
        b.e.process_host(x[:, :n])
    a.close(); b.close()


def test_a_new_dsp_rate_keeps_the_lines(qh):
    """qh_rxa_set_dsp_rate 48 k -> 96 k on an engine with bands A and B and FM filters of 4096 taps.  The oracle has no run-time rate
    setter, so the reference behind the change is a fresh oracle channel at the new rates with the SAME filter tail carried over
    (FmFilters.new_rate: new impulses, the lines kept, fmd.c:201-216).  For a fresh channel to be the reference, nothing ahead of the
    detector may carry state over the change, and the detector must see the new signal from its first sample (it takes an angle: a
    weak remainder in a kept line is a full-scale audio of its own until the new signal's main lobe arrives, and exact silence leaves
    the loop on rounding noise).  So: rates 96000 / 48000 / 48000, which leaves no input resampler behind the change, and nbp0 switched
    off (RXANBPSetRun 0: xnbp copies), on both sides.  Then what the engine puts out behind the change is the kept lines' response to
    the old audio plus the new audio, which zeroed lines would miss by the first part's whole size (printed).  Ahead of the change the
    last call is held: the front resampler's own start is the loop's rounding-noise start, and the filters have forgotten it by then."""
    calls, rates = (64, 128, 64), (96000, RATE, RATE)
    x = _input(2, calls, size=128, rate=96000)
    b = Bank(qh, [FM, FM], rates=rates)
    b.set("SetRXAFMAFFilter", 1, *BAND_B)
    for c in range(2):
        b.set("RXANBPSetRun", c, 0)
        b.set("SetRXAFMNCde", c, 4096); b.set("SetRXAFMNCaud", c, 4096)
        b.set("SetRXACTCSSRun", c, 0)       # the lines are the subject: the notch behind them is left out on both sides
    y, r = b.run(x, calls)
    last = sum(calls[:2]) * SIZE
    _held(y[:, last:], r[:, last:], "the last call ahead of the new rate")
    b.e.set_dsp_rate(96000)
    after = Bank(qh, [FM, FM], rates=(96000, 96000, RATE))
    after.e.close()
    after.e = b.e
    for c in range(2):
        after.refs[c].RXANBPSetRun(0)
        after.refs[c].o.SetRXACTCSSRun(0)
        tail = b.refs[c].fm
        tail.new_rate(96000)
        after.refs[c].fm = tail
    x2 = _input(2, (128,), rate=96000)[:, ::-1].copy()
    y2, r2 = after.call(x2)
    lines = [float(np.sqrt(np.mean(np.abs(r2[c][:512]) ** 2))) for c in range(2)]
    print("rms of the first 512 outputs behind the change (the kept lines' response): %s" % lines)
    assert min(lines) > 0.1, lines
    _held(y2, r2, "behind the new rate")
    _held(y2[:, :512], r2[:, :512], "the first 512 outputs behind the new rate")
    b.close(); after.refs[0].close(); after.refs[1].close()


def test_a_new_dsp_size_drops_the_lines(qh):
    """qh_rxa_set_dsp_size 64 -> 128 (setSize_fmd makes the fircores anew, fmd.c:218-237): behind it the engine is a fresh chain"""
    calls = (64, 128)
    x = _input(2, calls)
    b = Bank(qh, [FM, FM])
    b.set("SetRXAFMAFFilter", 1, *BAND_B)
    y, r = b.run(x, calls)
    _held(y, r, "ahead of the new size")
    b.e.set_dsp_size(128)
    after = Bank(qh, [FM, FM], size=128)
    after.e.close()
    after.e = b.e
    after.set_ref = None
    after.refs[1].SetRXAFMAFFilter(*BAND_B)
    x2 = _input(2, (64,), size=128)[:, ::-1].copy()
    y2, r2 = after.call(x2)
    _held(y2, r2, "behind the new size")
    b.close(); after.refs[0].close(); after.refs[1].close()
