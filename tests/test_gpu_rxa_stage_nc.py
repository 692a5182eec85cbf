"""nc, mp and window per stage: RXANBPSetNC / MP (wdsp/nbp.c:563-588), RXABPSNBASetNC / MP (snb.c:829-855), SetRXABandpassNC / MP / Window
(bandpass.c:411-457).  2 to 3 channels, dsp_size 64, 48 kHz at all three rates, five ragged calls of 1 to 40 blocks (6400 samples: the calls
cross the 4097-sample seam of the 8192-point tiles).  -m gpu.

  (a) the seven NC names (three plus four MP names) on one engine are RXASetNC (RXASetMP) on another, bit for bit, over a USB / AM / FM bank
  (b) one stage at a time on the linear chain nbp0 -> bp1, per output sample against the closed long-double form composed of
      tests/rxa_linear_ref.py's pieces, at the bound that module's `margins` applies: 16 E, E the float64 overlap-save model's own error
  (c) bpsnba on its own nc and mp beside nbp0 at 2048 taps, SNBA on, against the oracle's channel with its bpsnba replaced (below): 1e-6
  (d) bpsnba at 8192 taps (two partitions) beside a one-tile nbp0, and the reverse on a second channel: the same reference, 1e-6
  (e) a changed nc zeroes its own stage's delay line alone; a new window keeps it; a setter given the value in force changes no bit
  (f) a per-stage setter between graph-replayed calls drops the graphs: the replayed output is the plain launches', bit for bit

The reference of (c) and (d).  In USB the blanker's bandpass takes the channel's signal AHEAD of nbp0 and its output REPLACES nbp0's
(xbpsnbain / xbpsnbaout at position 0, RXA.c:567,572), so with the shift off and one rate throughout its input is the channel's input and
its output is what the oracle's stage hook at the xfmsq site finds in midbuff: the hook puts there the output of a fircore of the
test's own (pyoracle.Fircore: wo_fircore_*) with the impulse recalc_bpsnba_filter designs for the stage's own nc and mp (wo_fir_bandpass
at RXAbpsnbaCheck's 250 .. 5700 Hz, window 0, gain 1; wo_mp_imp when mp is set; the notches do not run, so make_nbp has nothing to do), and
xsnba, bp1 and the rest of the oracle's chain follow.  nbp0's own output reaches the S meter alone there: the reverse channel of (d) is held
by that meter against an oracle channel with nbp0 at 8192 taps."""
import ctypes as C

import numpy as np
import pytest
import torch

import rxa_linear_ref as R
from conftest import rel_rms

pytestmark = pytest.mark.gpu
RATE, SIZE = 48000, 64
BLOCKS = (1, 40, 7, 33, 19)
N = sum(BLOCKS) * SIZE
USB, LSB, FM, AM = 1, 0, 5, 6
BAND = (300.0, 3000.0)
AGC_DB = 6.0
NC_NAMES = ("RXANBPSetNC", "RXABPSNBASetNC", "SetRXABandpassNC", "SetRXAEQNC", "SetRXAFMSQNC", "SetRXAFMNCde", "SetRXAFMNCaud")    # RXA.c:938-944
MP_NAMES = ("RXANBPSetMP", "RXABPSNBASetMP", "SetRXABandpassMP", "SetRXAEQMP", "SetRXAFMSQMP", "SetRXAFMMPde", "SetRXAFMMPaud")    # RXA.c:951-957


def noise_and_tones(nch, seed=3, n=N):
    rng = np.random.default_rng(seed)
    t = np.arange(n) / float(RATE)
    x = 0.1 * (rng.standard_normal((nch, n)) + 1j * rng.standard_normal((nch, n)))
    for c in range(nch):
        x[c] += np.exp(-2j * np.pi * (1650.0 + 100.0 * c) * t) + 10.0 * np.exp(-2j * np.pi * (3400.0 + 50.0 * c) * t)
    return x


def walk(e, x, blocks=BLOCKS, between=None):
    out, pos = [], 0
    for j, nb in enumerate(blocks):
        if between:
            between(j, e)
        out.append(e.process_host(np.ascontiguousarray(x[:, pos:pos + nb * SIZE])))
        pos += nb * SIZE
    assert pos == x.shape[1]
    return np.concatenate(out, axis=1)


def make(qh, nch):
    return qh.RxaEngine(nch, dsp_size=SIZE, in_rate=RATE, dsp_rate=RATE, out_rate=RATE)


# ------------------------------------------------------------------------------------------------------------------ (a)
def mixed_bank(qh):
    e = make(qh, 3)
    e.SetRXAShiftRun(-1, 0)
    for c, (mode, band) in enumerate(((USB, BAND), (AM, (-4000.0, 4000.0)), (FM, (-4000.0, 4000.0)))):
        e.SetRXAMode(c, mode)
        e.RXASetPassband(c, *band)
    e.SetRXASNBARun(0, 1)                               # bpsnba runs on the USB channel
    e.SetRXAAGCMode(-1, 0)
    e.SetRXAAGCFixed(-1, AGC_DB)
    return e


def mixed_input():
    rng = np.random.default_rng(8)
    t = np.arange(N) / float(RATE)
    usb = 0.3 * np.exp(-2j * np.pi * 1200.0 * t)
    am = 0.3 * (1.0 + 0.5 * np.cos(2 * np.pi * 700.0 * t)) * np.exp(2j * np.pi * 0.3)
    fm = 0.3 * np.exp(2j * np.sin(2 * np.pi * 800.0 * t))
    return np.stack([usb, am, fm]) + 0.01 * (rng.standard_normal((3, N)) + 1j * rng.standard_normal((3, N)))


@pytest.mark.parametrize("which, value", [("nc", 512), ("nc", 8192), ("mp", 1)])
def test_the_seven_names_are_rxasetnc_and_rxasetmp(qh, which, value):
    x = mixed_input()
    names, whole = (NC_NAMES, "RXASetNC") if which == "nc" else (MP_NAMES, "RXASetMP")

    def per_stage(j, e):
        if j == 2:
            for n in names:
                getattr(e, n)(-1, value)

    def at_once(j, e):
        if j == 2:
            getattr(e, whole)(-1, value)
    a, b, p = mixed_bank(qh), mixed_bank(qh), mixed_bank(qh)
    try:
        ya, yb, yp = walk(a, x, between=per_stage), walk(b, x, between=at_once), walk(p, x)
    finally:
        a.close(); b.close(); p.close()
    assert np.all(np.isfinite(yb))
    assert np.array_equal(ya, yb)
    first = sum(BLOCKS[:2]) * SIZE
    for c in range(3):                                  # and the setting is seen on every channel
        assert np.array_equal(yb[c, :first], yp[c, :first]) and not np.array_equal(yb[c, first:], yp[c, first:]), c


# ------------------------------------------------------------------------------------------------------------------ (b), (e)
def linear_engine(qh, nch):
    """USB, nbp0 and bp1 both running, a fixed AGC gain: the linear chain"""
    e = make(qh, nch)
    e.SetRXAShiftRun(-1, 0)
    e.SetRXAMode(-1, LSB)
    e.SetRXAMode(-1, USB)
    e.RXASetPassband(-1, *BAND)
    e.SetRXABandpassRun(-1, 1)
    e.SetRXAAGCMode(-1, 0)
    e.SetRXAAGCFixed(-1, AGC_DB)
    return e


def stage(inp, designs, conv):
    """A fircore's output over the stream `inp`: designs = [(start, taps, keep)], each in force from sample `start`; keep False: the delay
    line is zeroed there (setNc_fircore), True: it runs on under the new taps (setMp_fircore, setImpulse_fircore)"""
    out = np.zeros(inp.size, dtype=inp.dtype)
    for i, (s, h, keep) in enumerate(designs):
        e = designs[i + 1][0] if i + 1 < len(designs) else inp.size
        src = inp.copy()
        if not keep:
            src[:s] = 0
        out[s:e] = conv(src[:e], h)[s:e]
    return out


def linear_ref(x, nbp, bp1):
    """(want in long double, bound packed per part) of nbp0 -> bp1 -> fixed gain and panel for the two stages' design lists"""
    R.require_long_double()
    want = R.panel(stage(stage(x.astype(R.CLD), nbp, R.conv_ld), bp1, R.conv_ld), AGC_DB)
    model = R.panel(stage(stage(x.astype(np.complex128), nbp, R.os_filter64), bp1, R.os_filter64), AGC_DB)
    E = float(max(np.max(np.abs(model.real - want.real)), np.max(np.abs(model.imag - want.imag))))
    b = R.MARGIN * E + (2.0 * np.pi * 2.0 ** -64) * (np.arange(want.size) + 1.0) * np.abs(want).astype(np.float64)
    return want, b + 1j * b, E


def taps(nc, wintype):
    return R.band_taps(nc, BAND[0], BAND[1], RATE, wintype)


LINEAR = {
    # name: (setters ahead of the first call, nbp0's designs, bp1's designs)
    "bp1 1024 window 0": ((("SetRXABandpassNC", 1024), ("SetRXABandpassWindow", 0)), ((2048, 0),), ((1024, 0),)),
    "nbp0 512": ((("RXANBPSetNC", 512),), ((512, 0),), ((2048, 1),)),
}


@pytest.mark.parametrize("name", list(LINEAR))
def test_one_stage_at_a_time_against_the_closed_form(qh, name):
    setters, nbp, bp1 = LINEAR[name]
    nch = 2
    x = noise_and_tones(nch)
    e = linear_engine(qh, nch)
    try:
        for n, v in setters:
            getattr(e, n)(-1, v)
        y = walk(e, x)
    finally:
        e.close()
    calls = np.concatenate([[0], np.cumsum(BLOCKS)[:-1]]) * SIZE
    for c in range(nch):
        want, bound, E = linear_ref(x[c], [(0, taps(*nbp[0]), False)], [(0, taps(*bp1[0]), False)])
        assert R.rms(want) > 0.5
        w = R.assert_inside("%s ch %d" % (name, c), y[c:c + 1], want[None, :], bound[None, :], (), calls)
        print("%s ch %d: E %.3e, worst error / bound %.3g" % (name, c, E, w["ratio"]))
        # the per-stage value is seen: the closed form of create_rxa's chain (2048 taps in both, bp1's window 1) lies far outside
        default, _, _ = linear_ref(x[c], [(0, taps(2048, 0), False)], [(0, taps(2048, 1), False)])
        assert np.max(np.abs(default - want)) > 1e3 * np.max(bound.real)


STATE = {
    # name: (setter ahead of the third call, which stage's design list gets (start, taps, keep) appended)
    "bp1 nc": (("SetRXABandpassNC", 1024), "bp1", (1024, 1), False),
    "nbp0 nc": (("RXANBPSetNC", 1024), "nbp", (1024, 0), False),
    "bp1 window": (("SetRXABandpassWindow", 0), "bp1", (2048, 0), True),
}


@pytest.mark.parametrize("name", list(STATE))
def test_a_new_nc_zeroes_its_own_line_and_a_new_window_keeps_it(qh, name):
    """the setter falls between the second and the third call.  Behind it the closed form has the changed stage start from an empty line
    (nc) or run on (window) while the OTHER stage's line runs on: had it been zeroed too, the samples behind the change would miss the
    bound by orders of magnitude (asserted on the reference itself)"""
    (setter, value), which, design, keep = STATE[name]
    nch = 2
    x = noise_and_tones(nch, seed=5)
    at = sum(BLOCKS[:2]) * SIZE
    e = linear_engine(qh, nch)
    try:
        y = walk(e, x, between=lambda j, e: getattr(e, setter)(-1, value) if j == 2 else None)
    finally:
        e.close()
    calls = np.concatenate([[0], np.cumsum(BLOCKS)[:-1]]) * SIZE
    for c in range(nch):
        nbp, bp1 = [(0, taps(2048, 0), False)], [(0, taps(2048, 1), False)]
        (nbp if which == "nbp" else bp1).append((at, taps(*design), keep))
        want, bound, E = linear_ref(x[c], nbp, bp1)
        w = R.assert_inside("%s ch %d" % (name, c), y[c:c + 1], want[None, :], bound[None, :], (), calls)
        print("%s ch %d: E %.3e, worst error / bound %.3g" % (name, c, E, w["ratio"]))
        # the reference with BOTH lines zeroed at the change (and, for the window, with its line zeroed) is far away
        both = [(0, taps(2048, 0), False), (at, nbp[-1][1], False)], [(0, taps(2048, 1), False), (at, bp1[-1][1], False)]
        far, _, _ = linear_ref(x[c], *both)
        assert np.max(np.abs(far[at:at + 1024] - want[at:at + 1024])) > 1e3 * np.max(bound.real)


def snba_engine(qh, nch):
    e = make(qh, nch)
    e.SetRXAShiftRun(-1, 0)
    e.SetRXAMode(-1, USB)
    e.RXASetPassband(-1, *BAND)
    e.SetRXASNBARun(-1, 1)
    e.SetRXAAGCMode(-1, 0)
    e.SetRXAAGCFixed(-1, AGC_DB)
    return e


def test_a_new_nbp0_nc_leaves_bpsnba_and_bp1_running_on(qh):
    """USB with SNBA: the audio goes x -> bpsnba -> xsnba -> bp1, nbp0's output feeds the S meter alone (RXA.c:567-572).  RXANBPSetNC on
    one engine, nothing on the other: the same audio bit for bit -- neither bpsnba's line (which RXASetNC zeroes with nbp0's) nor bp1's
    was touched; and the per-stage setters given the values in force change no bit either"""
    nch = 2
    x = crackle(nch)

    def change(j, e):
        if j == 2:
            e.RXANBPSetNC(-1, 1024)

    def same(j, e):
        if j == 2:
            e.RXANBPSetNC(-1, 2048); e.RXABPSNBASetNC(-1, 2048); e.SetRXABandpassNC(-1, 2048)
            e.RXANBPSetMP(-1, 0); e.RXABPSNBASetMP(-1, 0); e.SetRXABandpassMP(-1, 0); e.SetRXABandpassWindow(-1, 1)
    a, b, p = snba_engine(qh, nch), snba_engine(qh, nch), snba_engine(qh, nch)
    try:
        ya, yb, yp = walk(a, x, between=change), walk(b, x, between=same), walk(p, x)
    finally:
        a.close(); b.close(); p.close()
    assert np.abs(yp).max() > 0.05
    assert np.array_equal(ya, yp)
    assert np.array_equal(yb, yp)


# ------------------------------------------------------------------------------------------------------------------ (c), (d)
def crackle(nch, n=N):
    """carriers inside bpsnba's band with impulses for the blanker to repair"""
    rng = np.random.default_rng(900)
    t = np.arange(n) / float(RATE)
    x = np.zeros((nch, n), dtype=np.complex128)
    for c in range(nch):
        x[c] = sum(a * np.exp(-2j * np.pi * (f + 30.0 * c) * t) for a, f in ((0.08, 700.0), (0.05, 1210.0), (0.03, 2300.0)))
        k = rng.integers(0, n, n // 533)
        x[c, k] += (2.0 + 6.0 * rng.random(k.size)) * np.exp(2j * np.pi * rng.random(k.size))
    return x + 0.01 * (rng.standard_normal((nch, n)) + 1j * rng.standard_normal((nch, n)))


def bpsnba_impulse(oracle, nc, mp):
    """recalc_bpsnba_filter (snb.c:807-822) in USB: calc_nbp_impulse without notches is fir_bandpass (nbp.c:233-237); mp: calc_fircore's
    mp_imp (firmin.c:327-328)"""
    h = oracle.fir_bandpass(nc, 250.0, 5700.0, float(RATE), 0, 1, 1.0 / (2.0 * SIZE))
    if mp:
        L = oracle.lib()
        L.wo_mp_imp.argtypes = [C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_int]
        L.wo_mp_imp.restype = None
        out = np.zeros(nc, dtype=np.complex128)
        L.wo_mp_imp(nc, h.ctypes.data, out.ctypes.data, 16, 0)
        h = out
    return h


class SnbaRef:
    """the oracle's USB channel with SNBA on and its bpsnba replaced by a fircore of the stage's own nc and mp (the module's head)"""

    def __init__(self, oracle, nc, mp, nbp_nc=None):
        self.o = oracle.WdspChannel(SIZE, SIZE, RATE, RATE, RATE)
        o = self.o
        o.SetRXAShiftRun(0); o.SetRXAMode(USB); o.RXASetPassband(*BAND)
        if nbp_nc:
            o.RXASetNC(nbp_nc)                          # (every fircore of the oracle's channel; its bpsnba is replaced, bp1 is set back below)
        o.SetRXASNBARun(1); o.SetRXAAGCMode(0); o.SetRXAAGCFixed(AGC_DB)
        self.core = oracle.Fircore(SIZE, nc, bpsnba_impulse(oracle, nc, mp))
        self.block = None
        o.set_stage_hook(self._hook, sites=(oracle.WdspChannel.HOOK_FMSQ,))

    def _hook(self, where, z, aux):
        z[:] = self.core(self.block)

    def xrxa(self, x):
        out = np.empty(x.size, dtype=np.complex128)
        for b in range(0, x.size, SIZE):
            self.block = x[b:b + SIZE]
            out[b:b + SIZE] = self.o.xrxa(self.block)
        return out

    def close(self):
        self.o.close()


def test_the_replaced_bpsnba_is_the_oracles_own_at_the_defaults(oracle):
    """the composition itself, on the CPU (it runs under -m gpu with the file): at nc 2048 and mp 0 the replaced stage leaves the oracle's
    own output to the last bit"""
    x = crackle(1)[0]
    r = SnbaRef(oracle, 2048, 0)
    o = oracle.WdspChannel(SIZE, SIZE, RATE, RATE, RATE)
    o.SetRXAShiftRun(0); o.SetRXAMode(USB); o.RXASetPassband(*BAND); o.SetRXASNBARun(1); o.SetRXAAGCMode(0); o.SetRXAAGCFixed(AGC_DB)
    a, b = r.xrxa(x), o.xrxa(x)
    r.close(); o.close()
    assert np.abs(b).max() > 0.05 and np.array_equal(a, b)


def test_bpsnba_on_its_own_nc_and_mp(qh, oracle):
    nch = 2
    x = crackle(nch)
    e = snba_engine(qh, nch)
    plain = snba_engine(qh, nch)
    try:
        e.RXABPSNBASetNC(-1, 256)
        e.RXABPSNBASetMP(-1, 1)
        y, yp = walk(e, x), walk(plain, x)
    finally:
        e.close(); plain.close()
    for c in range(nch):
        r = SnbaRef(oracle, 256, 1)
        ref = r.xrxa(x[c])
        r.close()
        assert np.all(np.isfinite(ref)) and np.abs(ref).max() > 0.05
        print("bpsnba 256 mp ch %d: rel rms %.3e (the default bpsnba: %.3e)" % (c, rel_rms(y[c], ref), rel_rms(yp[c], ref)))
        assert rel_rms(y[c], ref) < 1e-6
        assert rel_rms(yp[c], ref) > 1e-2               # 256 minimum-phase taps are another filter than 2048 linear-phase ones


def test_a_partitioned_and_a_one_tile_stage_share_a_call(qh, oracle):
    """channel 0: bpsnba at 8192 taps (two partitions) beside nbp0 at 2048; channel 1: nbp0 at 8192 beside bpsnba at 2048.  Both stages
    then run their partitioned form with rows of one and of two partitions, next to bp1 in one tile"""
    blocks = (3, 40, 37, 40, 40)                        # 10240 samples: the 8192 taps' group delay (4096) and a signal behind it
    x = crackle(2, n=sum(blocks) * SIZE)
    e = snba_engine(qh, 2)
    try:
        e.enable_meters(True)
        e.RXABPSNBASetNC(0, 8192)
        e.RXANBPSetNC(1, 8192)
        y = walk(e, x, blocks=blocks)
        s_meter = [e.GetRXAMeter(1, mt) for mt in (0, 1)]
    finally:
        e.close()
    r0 = SnbaRef(oracle, 8192, 0)
    ref0 = r0.xrxa(x[0])
    r0.close()
    r1 = SnbaRef(oracle, 2048, 0, nbp_nc=8192)
    # bp1 back at 2048 taps is not a name the oracle has: compare the S meter (nbp0's output) alone on this one ...
    r1.xrxa(x[1])
    want_meter = [r1.o.GetRXAMeter(mt) for mt in (0, 1)]
    r1.close()
    r2 = SnbaRef(oracle, 2048, 0)                       # ... and the audio, which nbp0's output does not reach, on the default channel
    ref1 = r2.xrxa(x[1])
    r2.close()
    for c, ref in ((0, ref0), (1, ref1)):
        assert np.all(np.isfinite(ref)) and np.abs(ref).max() > 0.05
        print("mixed forms ch %d: rel rms %.3e" % (c, rel_rms(y[c], ref)))
        assert rel_rms(y[c], ref) < 1e-6
    print("mixed forms ch 1 S meter: engine %s oracle %s" % (s_meter, want_meter))
    for got, want in zip(s_meter, want_meter):
        assert want > -100.0 and abs(got - want) < 0.002   # the gate of tests/test_gpu_rxa_parity.py's meters (meter.c's fast log)


# ------------------------------------------------------------------------------------------------------------------ (f)
def test_a_per_stage_setter_between_replayed_calls_drops_the_graphs(qh):
    """one block a call on fixed device buffers; a replay needs the same call three times in a row, so the setters fall between stretches
    of six calls, each on a graph captured under the old settings"""
    nch, ncalls = 2, 30
    x = noise_and_tones(nch, seed=9, n=ncalls * SIZE)
    events = {6: ("SetRXABandpassNC", 1024), 12: ("RXANBPSetMP", 1), 18: ("SetRXABandpassWindow", 0), 24: ("RXANBPSetNC", 512)}
    dev = torch.device("cuda:0")

    def run(replay, events):
        e = linear_engine(qh, nch)
        try:
            e.set_graph_replay(replay)
            d_in = torch.zeros((nch, SIZE), dtype=torch.complex128, device=dev)
            d_out = torch.zeros((nch, SIZE), dtype=torch.complex128, device=dev)
            ys = []
            for j in range(ncalls):
                if j in events:
                    getattr(e, events[j][0])(-1, events[j][1])
                d_in.copy_(torch.from_numpy(np.ascontiguousarray(x[:, j * SIZE:(j + 1) * SIZE])))
                torch.cuda.synchronize()
                e.process_ptr(d_in.data_ptr(), SIZE, d_out.data_ptr(), SIZE, 1)
                e.synchronize()
                ys.append(d_out.cpu().numpy())
            return np.concatenate(ys, axis=1), e.graph_launches()
        finally:
            e.close()
    plain, n_plain = run(False, events)
    replayed, n_replayed = run(True, events)
    assert n_plain == 0 and n_replayed >= 10, (n_plain, n_replayed)
    assert np.abs(plain).max() > 0.5
    assert np.array_equal(plain, replayed)
    # every setter is seen: a run with the later ones left out differs from its call on, and not before
    for at in sorted(events):
        fewer, _ = run(False, {j: v for j, v in events.items() if j < at})
        assert np.array_equal(fewer[:, :at * SIZE], plain[:, :at * SIZE]) and not np.array_equal(fewer[:, at * SIZE:], plain[:, at * SIZE:]), at
