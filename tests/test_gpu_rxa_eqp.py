"""xeqp in the batched RXA engine (RXA.c:579) against the restatement (tests/wdsp_eqp_ref.py).  -m gpu.

The whole-chain oracle has no equalizer, so two identities make the reference (tests/test_eqp_restatement.py holds them on the CPU):

  post-filter: where only linear time-invariant stages and memoryless real gains follow the equalizer (bp1, a fixed AGC gain, the panel
      with gain2I = gain2Q, no output resampler), engine(EQ on) = EQ_ref(engine(EQ off)) -- for AM, SAM and FM too, whose detectors sit
      ahead of it;
  pre-filter: with the shift off and in_rate = dsp_rate = out_rate, everything ahead of xeqp in an SSB chain is linear and time-invariant
      at the dsp rate, so engine(EQ on)(x) = oracle(EQ off)(EQ_ref(x)), whatever follows the equalizer (AGC, ANF).

Calls of (1, 3, 9, 1, 40, 17, 2) blocks of 256 dsp samples: less than a tile, across the 2049-output tile of nc 2048, many tiles.

A channel that sits the stage out while another keeps the stage's ping-pong pair flipping is held against the whole-chain reference
(tests/rxa_chain_ref.py) on both paths: test_equalizer_keeps_its_delay_line_while_a_channel_sits_it_out."""
import numpy as np
import pytest

from conftest import rel_rms
from quisk_amd import synth
from wdsp_eqp_ref import Eqp

pytestmark = pytest.mark.gpu

CALLS = (1, 3, 9, 1, 40, 17, 2)
TOL = 1e-9
TAPS_TOL = 1e-12                # tests/test_design_eq_host.py's bound on the design
USB, FM, AM, SAM = 1, 5, 6, 10
G4 = [2, -6, 5, 9]
G10 = [3, -12, 12, -6, 9, 0, -12, 12, 4, -9, 7]
P3 = (3, [0.0, 400.0, 1500.0, 5000.0], [-2.0, 6.0, -9.0, 3.0])         # a preamp of -2 dB
INVALID, UNSUPPORTED = "error -2", "error -3"


def _signal(mode, c, n, fs):
    """noise and tones through the passband (USB), or a carrier with two modulating tones over noise (AM / SAM / FM), at baseband"""
    r = np.random.default_rng(2000 + c)
    t = np.arange(n) / fs
    noise = (r.standard_normal(n) + 1j * r.standard_normal(n))
    if mode == USB:
        z = 0.02 * noise
        for f, a in ((350.0 + 40 * c, 0.1), (1100.0 + 90 * c, 0.07), (2700.0 - 50 * c, 0.05)):
            z = z + a * np.exp(2j * np.pi * ((f * t) % 1.0))
        return z
    m = 0.4 * np.cos(2 * np.pi * ((450.0 + 30 * c) * t)) + 0.3 * np.cos(2 * np.pi * ((2100.0 - 40 * c) * t))
    if mode == FM:
        ph = 2 * np.pi * 3000.0 * np.cumsum(m) / fs
        return 0.3 * np.exp(1j * ph) + 0.003 * noise
    return 0.3 * (1.0 + m) * np.exp(1j * 0.7) + 0.003 * noise


def _input(modes, n, fs, shifted):
    t = np.arange(n) / fs
    rows = []
    for c, m in enumerate(modes):
        z = _signal(m, c, n, fs)
        rows.append(z * np.exp(-2j * np.pi * ((synth.shift_freq(c) * t) % 1.0)) if shifted else z)
    return np.stack(rows)


def _engine(qh, modes, dsp_size=256, in_rate=192000, shift=True, bp1=False):
    e = qh.RxaEngine(len(modes), dsp_size=dsp_size, in_rate=in_rate, dsp_rate=48000, out_rate=48000)
    for c, m in enumerate(modes):
        e.SetRXAShiftRun(c, 1 if shift else 0)
        if shift:
            e.SetRXAShiftFreq(c, synth.shift_freq(c))
        e.RXANBPSetRun(c, 1)
        e.SetRXAMode(c, m)
        e.RXASetPassband(c, *((150.0, 4000.0) if m == USB else (-8000.0, 8000.0) if m == FM else (-5000.0, 5000.0)))
        e.SetRXAAGCMode(c, 0); e.SetRXAAGCFixed(c, 10.0)
        if bp1:
            e.SetRXABandpassRun(c, 1)
    return e


class _Both:
    """a setter on the engine's channel c (or every channel, -1) and on the restatements"""

    def __init__(self, e, refs):
        self.e, self.refs = e, refs

    def __getattr__(self, name):
        def call(c, *a):
            if name != "flush":
                getattr(self.e, name)(c, *a)
            for k in (range(len(self.refs)) if c < 0 else (c,)):
                getattr(self.refs[k], name)(*a)
        return call

    def take_mp_taps(self):
        """behind a process call, ahead of the restatement's: a running minimum-phase channel takes the taps the library uploaded for that
        call (wdsp_eqp_ref.Eqp says why); the delay line is kept"""
        for k, r in enumerate(self.refs):
            if r.mp and r.run:
                r.use_taps(self.e.debug_eqp(k))


def _profiles(both):
    both.SetRXAGrphEQ(1, G4)
    both.SetRXAGrphEQ10(2, G10)
    both.SetRXAEQProfile(3, *P3)


def _post(qh, modes, prep=None, between=None, calls=CALLS, dsp_size=256, bp1=False):
    """A (equalizer as set by prep / between) and B (never touched) over the calls; A against EQ_ref(B), call by call"""
    a, b = _engine(qh, modes, dsp_size, bp1=bp1), _engine(qh, modes, dsp_size, bp1=bp1)
    refs = [Eqp(48000, size=dsp_size) for _ in modes]
    both = _Both(a, refs)
    x = _input(modes, sum(calls) * a.dsp_insize, 192000.0, True)
    ya, yr, pos = [], [], 0
    try:
        if prep:
            prep(both)
        for k, nb in enumerate(calls):
            if between:
                between(k, a, b, both)
            xa = np.ascontiguousarray(x[:, pos:pos + nb * a.dsp_insize])
            pos += nb * a.dsp_insize
            pa, pb = a.process_host(xa), b.process_host(xa)
            both.take_mp_taps()
            ya.append(pa); yr.append(np.stack([refs[c].process(pb[c]) for c in range(len(modes))]))
        taps = [a.debug_eqp(c) for c in range(len(modes))]
    finally:
        a.close(); b.close()
    return np.concatenate(ya, 1), np.concatenate(yr, 1), refs, taps


def _hold(ya, yr, what):
    for c in range(ya.shape[0]):
        err = rel_rms(ya[c], yr[c])
        print("%s, channel %d: relative RMS %.3g" % (what, c, err))
        assert np.any(yr[c]) and err < TOL, (c, err)


def _hold_taps(refs, taps):
    for c, (r, t) in enumerate(zip(refs, taps)):
        want = r.design()
        assert t is not None and len(t) == r.nc
        err = np.abs(t - want).max() / np.abs(want).max()
        print("channel %d: taps %.3g of the largest from the restated design" % (c, err))
        assert err <= TAPS_TOL, (c, err)


@pytest.mark.parametrize("dsp_size,nc", [(256, 2048), (256, 4096), (64, 256)])
def test_linear_path_against_the_post_filter_identity(qh, dsp_size, nc):
    """all-USB, shift on, 192k -> 48k, fixed gain; per channel: the default flat profile, GrphEQ, GrphEQ10 and a 3-point profile with a
    preamp.  nc 4096 takes 8192-point tiles; nc 256 runs on an engine of 64-sample blocks beside the other stages' 2048 taps."""
    def prep(both):
        if nc != 2048:
            both.SetRXAEQNC(-1, nc)
        _profiles(both)
        both.SetRXAEQRun(-1, 1)

    calls = CALLS if dsp_size == 256 else tuple(4 * k for k in CALLS)
    ya, yr, refs, taps = _post(qh, [USB] * 4, prep, calls=calls, dsp_size=dsp_size)
    _hold_taps(refs, taps)
    _hold(ya, yr, "linear path, dsp_size %d, nc %d" % (dsp_size, nc))


def test_per_mode_path_against_the_post_filter_identity(qh):
    """USB, AM, SAM, FM with the equalizer on in all four and bp1 behind it"""
    def prep(both):
        _profiles(both)
        both.SetRXAEQRun(-1, 1)

    ya, yr, refs, taps = _post(qh, [USB, AM, SAM, FM], prep, bp1=True)
    _hold_taps(refs, taps)
    _hold(ya, yr, "per-mode path")


def _pre(qh, oracle, setup, tol, what):
    """engine(EQ on)(x) against oracle(EQ off)(EQ_ref(x)): four USB channels at 48 kHz throughout, shift off"""
    modes = [USB] * 4
    e = _engine(qh, modes, in_rate=48000, shift=False)
    refs = [Eqp(48000) for _ in modes]
    both = _Both(e, refs)
    x = _input(modes, sum(CALLS) * 256, 48000.0, False)
    ws = []
    try:
        setup(e, -1)
        _profiles(both)
        both.SetRXAEQRun(-1, 1)
        pos, ys = 0, []
        for nb in CALLS:
            ys.append(e.process_host(np.ascontiguousarray(x[:, pos:pos + nb * 256])))
            pos += nb * 256
        y = np.concatenate(ys, 1)
        for c in range(4):
            w = oracle.WdspChannel(256, 256, 48000, 48000, 48000)
            ws.append(w)
            w.SetRXAShiftRun(0); w.RXANBPSetRun(1); w.SetRXAMode(USB); w.RXASetPassband(150.0, 4000.0)
            w.SetRXAAGCMode(0); w.SetRXAAGCFixed(10.0)
            setup(w, None)
            want = w.xrxa(refs[c].process(x[c]))
            err = rel_rms(y[c], want)
            print("%s, channel %d: relative RMS %.3g" % (what, c, err))
            assert np.any(want) and err < tol, (c, err)
    finally:
        e.close()
        for w in ws:
            w.close()


def _on(obj, ch, name, *a):
    getattr(obj, name)(*((ch,) + a if ch is not None else a))


def test_pre_filter_identity_with_agc_mode_3_behind(qh, oracle):
    """1e-9: the bound tests/test_gpu_wcpagc_batch.py holds the AGC to"""
    _pre(qh, oracle, lambda o, ch: _on(o, ch, "SetRXAAGCMode", 3), 1e-9, "AGC mode 3 behind the equalizer")


@pytest.mark.parametrize("position", [0, 1])
def test_pre_filter_identity_with_anf_behind(qh, oracle, position):
    """ANF at position 0, and at position 1 with bp1 between: 1e-6, the project's gate for the LMS stages"""
    def setup(o, ch):
        _on(o, ch, "SetRXAANFPosition", position)
        _on(o, ch, "SetRXAANFRun", 1)

    _pre(qh, oracle, setup, 1e-6, "ANF at position %d behind the equalizer" % position)


def test_setter_walk(qh):
    """USB with the equalizer as the last filter, 21 calls; between them: profiles, Ctfmode, Wintype, MP 1 (taps from debug_eqp), NC 2048 ->
    1024 (line zeroed), Run 0 on two channels for three calls and Run 1 again (line kept from before), flush.  Against the restatement."""
    calls = CALLS * 3

    def between(k, a, b, both):
        if k == 0:
            both.SetRXAEQRun(-1, 1)
        elif k == 2:
            _profiles(both)
        elif k == 4:
            both.SetRXAEQCtfmode(2, 1); both.SetRXAEQCtfmode(3, 1)
        elif k == 5:
            both.SetRXAEQWintype(-1, 1)
        elif k == 7:
            both.SetRXAEQMP(3, 1); both.SetRXAEQMP(0, 1)
        elif k == 9:
            both.SetRXAEQNC(1, 1024); both.SetRXAEQNC(3, 1024)
        elif k == 11:
            both.SetRXAEQRun(1, 0); both.SetRXAEQRun(2, 0)
        elif k == 12:
            both.SetRXAGrphEQ(1, [0, 4, -4, 8])              # while it is off: taken up when it runs again
        elif k == 14:
            both.SetRXAEQRun(1, 1); both.SetRXAEQRun(2, 1)
        elif k == 16:
            a.flush(); b.flush(); both.flush(-1)
        elif k == 18:
            both.SetRXAEQMP(-1, 0); both.SetRXAGrphEQ10(0, G10)

    ya, yr, refs, taps = _post(qh, [USB] * 4, None, between, calls=calls)
    _hold(ya, yr, "setter walk")
    _hold_taps(refs, taps)


def _raises(code, f, *a):
    with pytest.raises(Exception) as ei:
        f(*a)
    assert code in str(ei.value), str(ei.value)


def test_refusals(qh):
    """every stated deviation returns its code, and the next valid call gives the bits of an engine that never saw the bad setter"""
    modes = [USB] * 4
    a, n = _engine(qh, modes), _engine(qh, modes)
    x = _input(modes, 24 * 1024, 192000.0, True)
    blk = [np.ascontiguousarray(x[:, k * 4096:(k + 1) * 4096]) for k in range(6)]
    try:
        for e in (a, n):
            e.SetRXAGrphEQ(1, G4); e.SetRXAGrphEQ10(2, G10); e.SetRXAEQProfile(3, *P3); e.SetRXAEQRun(-1, 1)
        # a running equalizer with nc above 4096: taken by the setter, refused at the process call, nothing run
        a.SetRXAEQNC(2, 8192)
        _raises(UNSUPPORTED, a.process_host, blk[0])
        a.SetRXAEQNC(2, 2048)
        assert np.array_equal(a.process_host(blk[0]), n.process_host(blk[0]))
        # ... not refused while that channel's equalizer is off (a new nc zeroes the line, so the other engine gets a valid new nc too)
        a.SetRXAEQRun(2, 0); n.SetRXAEQRun(2, 0)
        a.SetRXAEQNC(2, 8192); n.SetRXAEQNC(2, 1024)
        assert np.array_equal(a.process_host(blk[1]), n.process_host(blk[1]))
        a.SetRXAEQNC(2, 2048); n.SetRXAEQNC(2, 2048)
        a.SetRXAEQRun(2, 1); n.SetRXAEQRun(2, 1)
        # QH_ERR_INVALID at the setter, nothing changed
        _raises(INVALID, a.SetRXAEQNC, 0, 300)
        _raises(INVALID, a.SetRXAEQNC, 0, 128)
        _raises(INVALID, a.SetRXAEQProfile, 1, 0, [0.0], [0.0])
        _raises(INVALID, a.SetRXAEQProfile, 1, 2, [0.0, float("nan"), 900.0], [0.0, 1.0, 2.0])
        _raises(INVALID, a.SetRXAEQProfile, 1, 2, [0.0, 300.0, 900.0], [0.0, float("inf"), 2.0])
        _raises(INVALID, a.SetRXAEQProfile, 1, 2, [0.0, 300.0, 900.0], [float("nan"), 1.0, 2.0])
        _raises(INVALID, a.SetRXAEQProfile, 1, 2, None, [0.0, 1.0, 2.0])
        _raises(INVALID, a.SetRXAEQProfile, 1, 2, [0.0, 300.0, 900.0], None)
        _raises(INVALID, a.SetRXAGrphEQ, 1, None)
        _raises(INVALID, a.SetRXAGrphEQ10, 1, None)
        assert np.array_equal(a.process_host(blk[2]), n.process_host(blk[2]))
        # two frequencies that coincide at Nyquist with different gains: refused at the process call while the channel runs, nothing run
        a.SetRXAEQProfile(1, 2, [0.0, 30000.0, 40000.0], [0.0, 3.0, -3.0])
        _raises(UNSUPPORTED, a.process_host, blk[3])
        a.SetRXAEQRun(1, 0); n.SetRXAEQRun(1, 0)
        assert np.array_equal(a.process_host(blk[3]), n.process_host(blk[3]))
        a.SetRXAGrphEQ(1, G4)
        a.SetRXAEQRun(1, 1); n.SetRXAEQRun(1, 1)
        assert np.array_equal(a.process_host(blk[4]), n.process_host(blk[4]))
        # ... with equal gains they are accepted
        for e in (a, n):
            e.SetRXAEQProfile(1, 3, [0.0, 500.0, 30000.0, 40000.0], [0.0, -3.0, 3.0, 3.0])
        ya = a.process_host(blk[5])
        assert np.array_equal(ya, n.process_host(blk[5])) and np.all(np.isfinite(ya.view(np.float64))) and np.any(ya[1])
    finally:
        a.close(); n.close()


SIT_BLOCKS, SIT_BEFORE, SIT_AFTER = 3, 3, 2       # blocks a call; calls channel 1 runs the stage before it sits out, and from its return on


def _sit_out(e, sat, per_mode):
    """Two USB channels at the default sizes, a fixed gain (channel 0: AGC mode 3 where the per-mode path is asked for), the equalizer on in
    both; channel 1 switches it off for `sat` calls after SIT_BEFORE calls and on again.  e: the engine, or None for the references alone.
    Against the whole-chain reference (tests/rxa_chain_ref.py), whose xeqp keeps its line while run is 0 (eq.c:204-207).  Returns the
    engine's calls (or None), the references' calls, and channel 1's call of return from a reference whose line was zeroed there."""
    from rxa_chain_ref import RxaChainRef
    refs, lost = [RxaChainRef(), RxaChainRef()], RxaChainRef()

    def both(name, c, *a):
        for t, lead in ((e, (c,)), (refs[c], ())) + (((lost, ()),) if c == 1 else ()):
            if t is not None:
                getattr(t, name)(*lead, *a)

    for c in range(2):
        both("SetRXAShiftRun", c, 1); both("SetRXAShiftFreq", c, synth.shift_freq(c)); both("RXANBPSetRun", c, 1)
        both("SetRXAMode", c, USB); both("RXASetPassband", c, 150.0, 4000.0)
        both("SetRXAAGCMode", c, 3 if per_mode and c == 0 else 0); both("SetRXAAGCFixed", c, 10.0)
        both("SetRXAEQRun", c, 1)
    both("SetRXAGrphEQ10", 0, G10); both("SetRXAEQProfile", 1, *P3)
    ncalls, n = SIT_BEFORE + sat + SIT_AFTER, SIT_BLOCKS * 1024
    t = np.arange(ncalls * n) / 192000.0
    # a steady two-tone inside the passband (USB takes the input's negative side) on each channel's carrier: 768 dsp samples a call, well
    # inside the 2047-sample line
    x = np.stack([(0.2 * np.exp(-2j * np.pi * (((600.0 + 100 * c) * t) % 1.0)) + 0.15 * np.exp(-2j * np.pi * (((1700.0 + 150 * c) * t) % 1.0)))
                  * np.exp(-2j * np.pi * ((synth.shift_freq(c) * t) % 1.0)) for c in range(2)])
    ys, rs, lost_back = [], [], None
    for k in range(ncalls):
        if k == SIT_BEFORE:
            both("SetRXAEQRun", 1, 0)
        if k == SIT_BEFORE + sat:
            both("SetRXAEQRun", 1, 1)
            lost.eqp.delay[:] = 0.0
        seg = np.ascontiguousarray(x[:, k * n:(k + 1) * n])
        if e is not None:
            ys.append(e.process_host(seg))
        rs.append(np.stack([r.xrxa(seg[c]) for c, r in enumerate(refs)]))
        back = lost.xrxa(seg[1])
        if k == SIT_BEFORE + sat:
            lost_back = back
    for r in refs + [lost]:
        r.close()
    return ys or None, rs, lost_back


@pytest.mark.parametrize("path", ["linear", "per_mode"])
@pytest.mark.parametrize("sat", [1, 2])
def test_equalizer_keeps_its_delay_line_while_a_channel_sits_it_out(qh, sat, path):
    """Channel 0 runs the equalizer throughout, so the stage's ping-pong pair flips on every call; channel 1 runs it for three calls, sits
    out `sat` calls (an odd and an even number of flips) and runs it again: its first call back is gated on its own, channel 0 over the
    run, 1e-6 relative RMS (the whole-chain reference's gate, tests/test_gpu_rxa_stage_combinations.py).  On the linear path and on the
    per-mode one (AGC mode 3 on channel 0).  First the reference's own sensitivity: with the line zeroed at the return the call of
    return differs by more than 1e-3 (it does by 1.0: the 768 samples of a call do not reach the centre tap of the 2048)."""
    e = qh.RxaEngine(2)
    try:
        ys, rs, lost_back = _sit_out(e, sat, path == "per_mode")
    finally:
        e.close()
    back = SIT_BEFORE + sat
    sens = rel_rms(lost_back, rs[back][1])
    print("sat out %d, %s: a lost line changes the call of return by %.3g relative RMS" % (sat, path, sens))
    assert sens > 1e-3, sens
    per = ["%.1e/%.1e" % (rel_rms(y[0], r[0]), rel_rms(y[1], r[1])) for y, r in zip(ys, rs)]
    e_back = rel_rms(ys[back][1], rs[back][1])
    e0 = rel_rms(np.concatenate([y[0] for y in ys]), np.concatenate([r[0] for r in rs]))
    e1 = rel_rms(np.concatenate([y[1] for y in ys]), np.concatenate([r[1] for r in rs]))
    print("channel 1's call of return %.3g; over the run: channel 0 %.3g, channel 1 %.3g; per call (channel 0/channel 1) %r" % (e_back, e0, e1, per))
    assert e_back < 1e-6, (e_back, per)
    assert e0 < 1e-6 and e1 < 1e-6, (e0, e1, per)
