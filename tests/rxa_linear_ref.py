"""The linear RXA chain -- shift, input resampler, nbp0, fixed gain, panel, output resampler -- as one closed linear form in long double,
a float64 overlap-save model of the same chain, and the per-sample bound the engine's tile kernels are held to.  numpy only; the taps
come from oracle.fir_bandpass and oracle.resample_taps (the library's design is pinned to those by tests/test_design_host.py).

    z[n]   = x[n] exp(2 pi i phi[n] / 2^64)                       where SetRXAShiftRun is 1, else x[n]
    mid[m] = sum_k hr[k] u[M m - k],  u[L i] = z[i]                xresample with phnum = 0 at the stream's start (resample.c:120-157)
    y[m]   = panel(g sum_k hb[k] mid[m - k])                       hb = fir_bandpass(nc, flow, fhigh, dsp_rate, wintype, 1, gain)
    out    = the same resampler form at dsp_rate -> out_rate       when they differ

The oscillator is the contract of quisk_amd/csrc/qh_osfir.hpp (NCO state): the phase is a 64-bit count of turns; its step per input
sample is d = floor(frac(f / rate) 2^64), computed here exactly in rationals; the phase stands still while the shift is off; a new
frequency changes the step from the next call on and keeps the phase.

Bound, per output sample and per part:  |got - want| <= 16 E + 2 pi 2^-64 n_in |want[m]|

E is the largest per-sample error of the float64 model (overlap-save on 4096-point tiles, np.fft in complex128, impulse responses over
2048 taps as partitions of 2048) against the long-double form for the case; 16 is the margin of tests/filter_forms_ref.py for what a
kernel does differently from numpy's transform (radix order, twiddle tables, products summed ahead of the inverse transform, here also
the oscillator moved behind the filter).  n_in is the absolute input index: the second term allows the step one unit of its last place
(the library divides f by the rate in long double before it takes the floor).  Both come from the reference alone.
"""
import collections
import functools
import math
from fractions import Fraction

import numpy as np

import filter_forms_ref as F
from filter_forms_ref import TOL64, assert_inside, rms, worst_sample  # noqa: F401  (the tests take them from here)

LD, CLD = np.longdouble, np.clongdouble
KHIST_FRONT, KHIST_BAND = 2240, 4095            # qh_engine.hpp kHistFront, kHistBand: the delay lines of the front and the band stage
PART = 2048                                     # taps per partition of the float64 model
USB, LSB, CWU = 1, 0, 4
MARGIN = 16.0

Case = collections.namedtuple("Case", "name in_rate dsp_rate out_rate dsp_size mode band nc agc_db nbp_run kind schedule")


def case(name, in_rate=192000, dsp_rate=48000, out_rate=48000, dsp_size=256, mode=USB, band=(300.0, 3000.0), nc=2048, agc_db=6.0,
         nbp_run=1, kind="noise", schedule="retune"):
    """nc: one number, or a tuple that the channels cycle through.  kind: 'noise' (noise, an in-band tone and a blocker 20 dB over it
    400 Hz outside the band), 'clean' (the same without the blocker) or 'impulses'.  schedule: 'retune', 'fine', 'plain', 'off' (the
    shift never runs) or 'blocks' (one DSP block a call, the setters between stretches of six calls: the graph-replay runs)."""
    return Case(name, in_rate, dsp_rate, out_rate, dsp_size, mode, tuple(band), nc, agc_db, nbp_run, kind, schedule)


def require_long_double():
    assert np.finfo(np.longdouble).nmant >= 63, (
        "the reference needs a long double with a 64-bit significand (x87 extended or wider); this numpy's longdouble has %d bits"
        % (np.finfo(np.longdouble).nmant + 1))
    assert int(np.array([2 ** 64 - 1], dtype=np.uint64).astype(LD)[0]) == 2 ** 64 - 1, "uint64 -> long double must be exact"


def nc_of(cs, c):
    return cs.nc[c % len(cs.nc)] if isinstance(cs.nc, tuple) else cs.nc


# ---------------------------------------------------------------------------------------------------------------------------
# calls and the setter schedule
# ---------------------------------------------------------------------------------------------------------------------------
def call_blocks(cs):
    """Calls in DSP blocks, about 65 * 256 DSP-rate samples in all: single blocks, the largest call below and the smallest at the
    front's switch (n_in >= kHistFront) and the band stage's (n_mid >= kHistBand) between a tile writing the next delay line and
    hist_update_kernel, one more, the remainder, a single block.  dsp_size 256 at four input samples a DSP sample:
    1, 1, 2, 3, 15, 16, 17, 9, 1.  Schedule 'blocks': one block a call."""
    if cs.schedule == "blocks":
        return (1,) * (65 * 256 // cs.dsp_size)
    per_in = cs.dsp_size * cs.in_rate // cs.dsp_rate
    a, b = (KHIST_FRONT - 1) // per_in, (KHIST_BAND - 1) // cs.dsp_size
    sizes = [1, 1] + ([a, a + 1] if a >= 1 else []) + [b, b + 1, b + 2]
    rest = 65 * 256 // cs.dsp_size - sum(sizes) - 1
    return tuple(sizes + ([rest] if rest > 0 else []) + [1])


def shift_freq(c, k):
    """Channel c's k-th frequency: either sign, no two alike, below half of every input rate."""
    return (-1.0) ** (c + k) * (9000.0 + 1234.5 * c) + 777.25 * k


RETUNE = {1: (("freq", 1),),                    # straight after a call shorter than the front's delay line
          3: (("run", 0),), 4: (("run", 1),), 5: (("freq", 2),),
          6: (("run", 0), ("freq", 3)),         # a new frequency while the phase is parked
          7: (("run", 1),), 8: (("freq", 4),)}


# One block a call: a replay needs the same call three times in a row (a plain call, the capture, the replay) and every setter makes
# the captured sequence stale, so the setters fall between stretches of six calls -- each stretch replays, each event meets a graph
# captured under the old settings.
BLOCKS = {6: (("freq", 1),), 12: (("run", 0),), 18: (("run", 1),), 24: (("freq", 2),), 30: (("run", 0), ("freq", 3)),
          36: (("run", 1),), 42: (("freq", 4),)}
FINE = {4: (("freq", 2e-5),)}                   # one retune by 20 microhertz, for the planted phase-law fault of the CPU tests


def events(cs, ncalls):
    """{call index: ((setter, value), ...)} applied ahead of that call.  The value of 'freq' is the k of shift_freq, or (a float) an
    offset in Hz from the channel's first frequency."""
    ev = {"retune": RETUNE, "fine": FINE, "blocks": BLOCKS}.get(cs.schedule, {})
    return {j: e for j, e in ev.items() if j < ncalls}


def freq_value(c, v):
    return shift_freq(c, v) if isinstance(v, int) else shift_freq(c, 0) + v


def laws(cs, c):
    """(run, frequency) of channel c's oscillator during every call."""
    sizes = call_blocks(cs)
    ev = events(cs, len(sizes))
    run, f, out = (0 if cs.schedule == "off" else 1), shift_freq(c, 0), []
    for j in range(len(sizes)):
        for what, v in ev.get(j, ()):
            if what == "run":
                run = v
            else:
                f = freq_value(c, v)
        out.append((run, f))
    return out


def nco_step(f, rate):
    """floor(frac(f / rate) 2^64), exactly."""
    t = Fraction(float(f)) / Fraction(int(rate))
    t -= math.floor(t)
    return int(math.floor(t * 2 ** 64))


def nco_phase(cs, c):
    """(phase [n] as uint64 counts of 2^-64 turns, run [n]) per input sample of channel c."""
    per_in = cs.dsp_size * cs.in_rate // cs.dsp_rate
    step, run = [], []
    for nb, (r, f) in zip(call_blocks(cs), laws(cs, c)):
        step.append(np.full(nb * per_in, nco_step(f, cs.in_rate) if r else 0, dtype=np.uint64))
        run.append(np.full(nb * per_in, bool(r)))
    step, run = np.concatenate(step), np.concatenate(run)
    phase = np.zeros(step.size, dtype=np.uint64)
    np.cumsum(step[:-1], out=phase[1:])                 # wraps at 2^64 like the turns do
    return phase, run


def rotation(phase):
    """exp(2 pi i phase / 2^64) in long double."""
    t = phase.astype(LD) / LD(2) ** 64
    t = t - (t >= 0.5)                                  # [-0.5, 0.5): the argument's rounding stays at 2^-64
    a = (8 * np.arctan(LD(1))) * t
    r = np.empty(t.shape, dtype=CLD)
    r.real, r.imag = np.cos(a), np.sin(a)
    return r


# ---------------------------------------------------------------------------------------------------------------------------
# taps and the gain
# ---------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def resampler(in_rate, out_rate):
    """(taps in time order, L, M) of create_resample(in_rate, out_rate, fc 0, ncoef 0, gain 1), or None when the rates are equal."""
    if in_rate == out_rate:
        return None
    from oracle import pyoracle
    h, L, M, ncoef, cpp = pyoracle.resample_taps(in_rate, out_rate)
    assert h.size == ncoef == L * cpp
    return h.reshape(L, cpp).T.reshape(-1).copy(), L, M


@functools.lru_cache(maxsize=None)
def band_taps(nc, flow, fhigh, dsp_rate, wintype=0, gain=1.0):
    from oracle import pyoracle
    return pyoracle.fir_bandpass(nc, flow, fhigh, float(dsp_rate), wintype, 1, gain)


def stages(cs, c):
    """The chain's filters behind the oscillator: [(taps, L, M, gain behind it or None)]."""
    st = []
    r = resampler(cs.in_rate, cs.dsp_rate)
    if r:
        st.append((r[0], r[1], r[2], False))
    if cs.nbp_run:
        st.append((band_taps(nc_of(cs, c), cs.band[0], cs.band[1], cs.dsp_rate), 1, 1, False))
    if not st:
        st.append((np.ones(1), 1, 1, False))
    st[-1] = st[-1][:3] + (True,)                       # the fixed gain and the panel follow the DSP-rate stages
    r = resampler(cs.dsp_rate, cs.out_rate)
    if r:
        st.append((r[0], r[1], r[2], False))
    return st


def panel(y, agc_db, gain1=4.0, gain2=(1.0, 1.0), copy=0, select=3):
    """wcpAGC.c mode 0 (a fixed gain of 10^(dB / 20)) and patchpanel.c:55-101, in y's own type."""
    g = 10.0 ** (agc_db / 20.0)
    re, im = y.real * g, y.imag * g
    si, sq = select >> 1, select & 1
    I, Q = {0: (re * si, im * sq), 1: (re * si, re * si), 2: (im * sq, im * sq), 3: (im * sq, re * si)}[copy]
    out = np.empty(y.shape, dtype=y.dtype)
    out.real, out.imag = (gain1 * gain2[0]) * I, (gain1 * gain2[1]) * Q
    return out


# ---------------------------------------------------------------------------------------------------------------------------
# the long-double form: fast, and by direct sums
# ---------------------------------------------------------------------------------------------------------------------------
def conv_ld(x, h):
    """The first len(x) samples of x * h through np.fft in complex256."""
    n = x.size + h.size - 1
    N = 1 << (n - 1).bit_length()
    X = np.fft.fft(x.astype(CLD), N)
    assert X.dtype == CLD, "np.fft must run natively in long double (numpy >= 2.0)"
    return np.fft.ifft(X * np.fft.fft(np.asarray(h).astype(CLD), N))[:x.size]


def upsample(x, L):
    if L == 1:
        return x
    u = np.zeros(x.size * L, dtype=x.dtype)
    u[::L] = x
    return u


def mixed(cs, c, x, phase=None):
    """x behind the oscillator, in long double (phase: another phase law than the contract's, for a planted fault)."""
    p, run = nco_phase(cs, c)
    phase = p if phase is None else phase
    z = np.asarray(x).astype(CLD)
    z[run] *= rotation(phase[run])
    return z


def chain_ld(cs, c, x, phase=None, keep=None):
    """The chain's output in long double.  keep: a list that takes every stage's input."""
    y = mixed(cs, c, x, phase)
    for h, L, M, gain in stages(cs, c):
        if keep is not None:
            keep.append(y)
        y = conv_ld(upsample(y, L), h)[::M]
        if gain:
            y = panel(y, cs.agc_db)
    return y


def chain_direct(cs, c, x, lo, hi):
    """Outputs lo .. hi - 1 of the chain by direct long-double sums over exactly the samples they depend on."""
    st = stages(cs, c)
    need = [(lo, hi)]
    for h, L, M, _ in reversed(st):                     # outputs a .. b - 1 read u[a M - (nt - 1)] .. u[(b - 1) M], u[L i] = y[i]
        a, b = need[0]
        need.insert(0, (max(0, -((-(a * M - (h.size - 1))) // L)), (b - 1) * M // L + 1))
    a, b = need[0]
    y, y0 = mixed(cs, c, x)[a:b], a                     # y holds samples y0 .. of its stage (the oscillator is pointwise)
    for (h, L, M, gain), (a, b) in zip(st, need[1:]):
        u, u0 = upsample(y, L), y0 * L
        hl = np.asarray(h).astype(CLD)
        pos = np.arange(a, b) * M - u0
        acc = np.zeros(b - a, dtype=CLD)
        for k in range(h.size):
            idx = pos - k
            ok = (idx >= 0) & (idx < u.size)            # before the stream's start: zeros; beyond u: never (need covers it)
            if ok.all():
                acc += hl[k] * u[idx]
            elif ok.any():
                acc[ok] += hl[k] * u[idx[ok]]
        y, y0 = (panel(acc, cs.agc_db) if gain else acc), a
    return y


# ---------------------------------------------------------------------------------------------------------------------------
# the float64 model
# ---------------------------------------------------------------------------------------------------------------------------
def os_filter64(x, taps):
    """x * taps as overlap-save on 4096-point tiles in complex128 (filter_forms_ref.os_model); more than 2048 taps run as partitions
    of 2048 over delayed views of the stream, their outputs added in order."""
    taps = np.asarray(taps)
    y = None
    for p in range(0, taps.size, PART):
        xd = x if p == 0 else np.concatenate([np.zeros(min(p, x.size), dtype=np.complex128), x[:max(x.size - p, 0)]])
        part = F.os_model(xd, taps[p:p + PART], 1, F.F64)
        y = part if y is None else y + part
    return y


def chain_model64(cs, c, x):
    phase, run = nco_phase(cs, c)
    y = np.asarray(x).astype(np.complex128)
    y[run] = y[run] * rotation(phase[run]).astype(np.complex128)
    for h, L, M, gain in stages(cs, c):
        y = os_filter64(upsample(y, L), h)[::M]
        if gain:
            y = panel(y, cs.agc_db)
    return y


# ---------------------------------------------------------------------------------------------------------------------------
# inputs and the case records
# ---------------------------------------------------------------------------------------------------------------------------
def make_input(cs, c):
    """'noise' / 'clean': complex Gaussian noise of 0.1 a part, a unit tone at the band's centre and (noise) a blocker of 10, 400 Hz
    beyond the band's outer edge -- both where they land BEHIND the oscillator, so that they stay there across retunes, and at minus
    the design's frequencies (fir_bandpass's flow .. fhigh passes exp(-2 pi i f t), wdsp/fir.c:246-249); 'impulses':
    unit impulses every 977 samples, another offset and turn per channel."""
    phase, run = nco_phase(cs, c)
    n = phase.size
    if cs.kind == "impulses":
        x = np.zeros(n, dtype=np.complex128)
        pos = np.arange(7 + 13 * c, n, 977)
        x[pos] = 1j ** ((np.arange(pos.size) + c) % 4)
        return x
    rng = np.random.default_rng(4000 + 17 * c + cs.dsp_size + cs.in_rate // 1000)
    t = np.arange(n, dtype=np.float64)
    edge = max(cs.band, key=abs)                        # the edge away from zero, where a neighbouring signal sits
    sig = np.exp(-2j * np.pi * ((0.5 * (cs.band[0] + cs.band[1]) / cs.in_rate * t) % 1.0))
    if cs.kind == "noise":
        sig = sig + 10.0 * np.exp(-2j * np.pi * (((edge + math.copysign(400.0, edge)) / cs.in_rate * t) % 1.0))
    back = np.ones(n, dtype=np.complex128)
    back[run] = np.conj(rotation(phase[run])).astype(np.complex128)
    return sig * back + 0.1 * (rng.standard_normal(n) + 1j * rng.standard_normal(n))


@functools.lru_cache(maxsize=24)
def channel_ref(cs, c):
    """Channel c of a case, computed once and shared by every tile form: x, want (long double), E and the packed per-part bound."""
    require_long_double()
    x = make_input(cs, c)
    want = chain_ld(cs, c, x)
    model = chain_model64(cs, c, x)
    assert model.shape == want.shape
    E = float(max(np.max(np.abs(model.real - want.real)), np.max(np.abs(model.imag - want.imag))))
    n_in = np.ceil(np.arange(want.size) * (cs.in_rate / cs.out_rate)) + 1.0
    b = (MARGIN * E + (2.0 * np.pi * 2.0 ** -64) * n_in * np.abs(want).astype(np.float64))
    return {"x": x, "want": want, "E": E, "rms": rms(want), "bound": b + 1j * b}


def case_ref(cs, nch, form=0, meters=False):
    """The record of a case at nch channels: x [nch, n], want [nch, m], E per channel, the bound [nch, m] (packed per part), the
    call sizes in blocks and in input samples, the setter schedule, and the output indices at which the calls, the retunes and (for
    the band tile form and the meters asked for) the tiles start.  The channels' references are shared by every form."""
    ch = [channel_ref(cs, c) for c in range(nch)]
    blocks = call_blocks(cs)
    per_in, per_out = cs.dsp_size * cs.in_rate // cs.dsp_rate, cs.dsp_size * cs.out_rate // cs.dsp_rate
    calls = np.concatenate([[0], np.cumsum(blocks)[:-1]]) * per_out
    ev = events(cs, len(blocks))
    return {"x": np.stack([r["x"] for r in ch]), "want": np.stack([r["want"] for r in ch]), "E": [r["E"] for r in ch],
            "rms": [r["rms"] for r in ch], "bound": np.stack([r["bound"] for r in ch]), "blocks": blocks,
            "sizes": [nb * per_in for nb in blocks], "events": ev, "calls": calls, "retunes": calls[sorted(ev)] if ev else calls[:0], "tiles": tile_starts(cs, form, meters, nch)}


def tile_starts(cs, form=0, meters=False, nch=1):
    """Output indices at which the front's and the band stage's tiles start in every call, as Engine::process_chain lays them out
    (for the failure message and the margins record; no bound depends on them).  form: set_band_tile's argument."""
    blocks = call_blocks(cs)
    out_per_mid = Fraction(cs.out_rate, cs.dsp_rate)
    steps = []
    r = resampler(cs.in_rate, cs.dsp_rate)
    if r and r[1] == 1:
        steps.append(F.stage_geometry(r[0].size, r[2])[4])
    if cs.nbp_run:
        nc_max = max(nc_of(cs, c) for c in range(nch))
        if nc_max > 4096:
            steps.append(8192 - 4095)
        elif form in (6144, 8192) and nc_max <= 2048:
            steps.append(form - 2048)
        else:
            P = (nc_max - 1 + 255) // 256 * 256 if meters else nc_max - 1
            steps.append((4096 if nc_max <= 2048 else 8192) - P)
    marks, m = [], 0
    for nb in blocks:
        for s in steps:
            marks.extend(int((m + t) * out_per_mid) for t in range(0, nb * cs.dsp_size, s))
        m += nb * cs.dsp_size
    return np.unique(np.array(marks, dtype=np.int64))


# ---------------------------------------------------------------------------------------------------------------------------
# running a case: on the engine, and on the oracle
# ---------------------------------------------------------------------------------------------------------------------------
def _apply(call, ev, channels):
    for what, v in ev:
        for c in channels:
            if what == "run":
                call("SetRXAShiftRun", c, v)
            else:
                call("SetRXAShiftFreq", c, freq_value(c, v))


def _setup(call, cs, c):
    call("SetRXAShiftRun", c, 0 if cs.schedule == "off" else 1)
    call("SetRXAShiftFreq", c, shift_freq(c, 0))
    call("RXANBPSetRun", c, cs.nbp_run)
    call("SetRXAMode", c, USB if cs.mode != USB else LSB)       # leave the mode and come back: bp1, on since the channel's creation,
    call("SetRXAMode", c, cs.mode)                              # is switched off by a CHANGE of mode only (RXA.c:748-787)
    call("RXASetPassband", c, cs.band[0], cs.band[1])
    call("RXASetNC", c, nc_of(cs, c))
    call("SetRXAAGCMode", c, 0)
    call("SetRXAAGCFixed", c, cs.agc_db)


def run_engine(qh, cs, nch, form=0, meters=False, replay=None, info=None):
    """The case on a fresh RxaEngine, call by call.  replay None: through process_host (which never replays).  True / False: through
    process_ptr on fixed device buffers (the replay key holds the pointers and the block count, so every call has the same size) with
    set_graph_replay on / off.  info: a dict that takes graph_launches and band_tile.  Returns y [nch, m]."""
    rec = case_ref(cs, nch)
    e = qh.RxaEngine(nch, dsp_size=cs.dsp_size, in_rate=cs.in_rate, dsp_rate=cs.dsp_rate, out_rate=cs.out_rate)
    try:
        def call(name, c, *args):
            getattr(e, name)(c, *args)
        for c in range(nch):
            _setup(call, cs, c)
        if form:
            e.set_band_tile(form)
        if meters:
            e.enable_meters(True)
        if replay is not None:
            import torch
            e.set_graph_replay(bool(replay))
            nb = rec["blocks"][0]
            assert all(b == nb for b in rec["blocks"]), "process_ptr runs on fixed buffers: one call size"
            ni, no = nb * e.dsp_insize, nb * e.dsp_outsize
            dev = torch.device("cuda:0")
            d_in = torch.zeros((nch, ni), dtype=torch.complex128, device=dev)
            d_out = torch.zeros((nch, no), dtype=torch.complex128, device=dev)
        out, pos = [], 0
        for j, n in enumerate(rec["sizes"]):
            _apply(call, rec["events"].get(j, ()), range(nch))
            seg = np.ascontiguousarray(rec["x"][:, pos:pos + n])
            if replay is None:
                out.append(e.process_host(seg))
            else:
                d_in.copy_(torch.from_numpy(seg))
                torch.cuda.synchronize()
                e.process_ptr(d_in.data_ptr(), ni, d_out.data_ptr(), no, nb)
                e.synchronize()
                out.append(d_out.cpu().numpy())
            pos += n
        assert pos == rec["x"].shape[1]
        if form:
            assert e.band_tile() == form, "the engine did not take the tile form asked for"
        if info is not None:
            info.update(graph_launches=e.graph_launches(), band_tile=e.band_tile())
        return np.concatenate(out, axis=1)
    finally:
        e.close()


def run_oracle(po, cs, c):
    """Channel c of the case on oracle.WdspChannel.xrxa, call by call."""
    rec = channel_ref(cs, c)
    blocks = call_blocks(cs)
    per_in = cs.dsp_size * cs.in_rate // cs.dsp_rate
    o = po.WdspChannel(per_in, cs.dsp_size, cs.in_rate, cs.dsp_rate, cs.out_rate)

    def call(name, _c, *args):
        getattr(o, name)(*args)
    _setup(call, cs, c)
    ev = events(cs, len(blocks))
    out, pos = [], 0
    for j, nb in enumerate(blocks):
        _apply(call, ev.get(j, ()), [c])
        out.append(o.xrxa(rec["x"][pos:pos + nb * per_in]))
        pos += nb * per_in
    o.close()
    return np.concatenate(out)


def margins(got, rec):
    """The worst sample of got against the record's bound, with its distances; and the largest error over E."""
    w = worst_sample(got, rec["want"], rec["bound"], rec["tiles"], rec["calls"])
    w["to_retune"] = int(np.min(np.abs(rec["retunes"] - w["index"]))) if rec["retunes"].size else None
    g = np.asarray(got).astype(np.complex128)
    err = np.maximum(np.abs(g.real - rec["want"].real), np.abs(g.imag - rec["want"].imag)).max(axis=1)
    w["err_over_E"] = float(max(float(e) / E for e, E in zip(err, rec["E"])))
    return w


# ---------------------------------------------------------------------------------------------------------------------------
# the cases
# ---------------------------------------------------------------------------------------------------------------------------
REFERENCE_CASES = [                                 # the six configurations the reference and the oracle are compared in (CPU)
    case("192k usb 2048", kind="clean"),
    case("96k lsb 1024", in_rate=96000, mode=LSB, band=(-3000.0, -300.0), nc=1024, kind="clean"),
    case("384k cw 2048", in_rate=384000, mode=CWU, band=(500.0, 900.0), kind="clean"),
    case("48k 4096", in_rate=48000, nc=4096, kind="clean"),
    case("192k 8192 out 96k", out_rate=96000, nc=8192, kind="clean"),
    case("192k dsp 96k", dsp_rate=96000, out_rate=96000, kind="clean"),
]
BLOCKER_CASE = case("192k usb 2048 blocker")
