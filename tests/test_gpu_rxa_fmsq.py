"""xfmsq in the batched RXA engine (RXA.c:575) against the restatement (tests/wdsp_fmsq_ref.py).

Three engines with the same settings and AGC mode 0: A runs FM with the squelch, C runs FM without it, B runs mode SPEC with the same
passband and an identity panel, so B's output is nbp0's output.  The restatement runs xfmd's loop on B's output (the trigger), the noise
filter, the averages and the state machine, and multiplies C's output by the gain it finds: A is held to g C.  Samples with g = 0 are
exactly 0 in A, the state and count of qh_rxa_debug_fmsq equal the restatement's at every call's end, and the rest is under 1e-9 relative
RMS, the chain's bound.  The margins of the trigger actually used (tests/test_fmsq_restatement.py has them for the recipes alone) are
checked before the comparison: no threshold crossing closer than 1e-6, no tail count closer than 1e-3 to an integer.  -m gpu.

Inputs: a carrier keyed off 0.5 s / on 0.9 s with a 1 kHz tone at +-3 kHz deviation over band-limited noise (keyed_fm), about 4 s."""
import functools

import numpy as np
import pytest

from conftest import rel_rms
from quisk_amd import synth
from wdsp_fmsq_ref import DECREASE, INCREASE, MUTED, TAIL, UNMUTED, FmLoop, Fmsq, keyed_fm, margins, ready_count

pytestmark = pytest.mark.gpu

FS = 192000
TOL = 1e-9
FM, SPEC, USB = 5, 8, 1
# blocks of 1024 input samples: short calls through the first off / on / off of the carrier (1.4 s = 263 blocks), so that the ramp up and
# the tail straddle call boundaries, then one long call of many tiles
CALLS = (3, 1, 17) + (7,) * 40 + (480, 5, 2)
SEEDS = (3, 7, 11, 17)               # (13 put a tail count 3e-4 from an integer: replaced)


@functools.lru_cache(maxsize=None)
def _signal(ch, n, start_on):
    t = np.arange(n) / FS
    z = keyed_fm(n, FS, seed=SEEDS[ch], start_on=start_on)
    z = z * np.exp(-2j * np.pi * ((synth.shift_freq(ch) * t) % 1.0))
    z.setflags(write=False)
    return z


def _input(nch, n, start_on=()):
    return np.stack([_signal(c, n, c in start_on) for c in range(nch)])


def _engine(qh, modes, dsp_rate=48000):
    e = qh.RxaEngine(len(modes), dsp_rate=dsp_rate, out_rate=dsp_rate)
    for c, m in enumerate(modes):
        e.SetRXAShiftRun(c, 1); e.SetRXAShiftFreq(c, synth.shift_freq(c)); e.RXANBPSetRun(c, 1)
        e.SetRXAMode(c, m)
        e.RXASetPassband(c, *((300.0, 3000.0) if m == USB else (-8000.0, 8000.0)))
        e.SetRXAAGCMode(c, 0); e.SetRXAAGCFixed(c, 0.0)
    return e


class _Both:
    """a setter on engine A's channel and on its restatement"""

    def __init__(self, e, refs):
        self.e, self.refs = e, refs

    def __getattr__(self, name):
        def call(c, *a):
            getattr(self.e, name)(c, *a)
            getattr(self.refs[c], name)(*a)
        return call


def _run(qh, modes, on, calls=CALLS, dsp_rate=48000, between=None, prep=None, start_on=(), ref_kw=None, compare=True, prep_b=False):
    """A, B and C over the calls.  Returns a dict: ya / yc [nch, n], per FMSQ channel the restated output, gain, the ends
    [(state, count) per call] of the engine and of the restatement, and the margins of the trigger used."""
    nch = len(modes)
    a, c_, b = _engine(qh, modes, dsp_rate), _engine(qh, modes, dsp_rate), _engine(qh, [SPEC if m == FM else m for m in modes], dsp_rate)
    b.SetRXAPanelGain1(-1, 1.0)
    if prep:
        prep(a); prep(c_)
        if prep_b:
            prep(b)
    refs = {c: Fmsq(dsp_rate, **(ref_kw or {})) for c in on}
    loops = {c: FmLoop(float(dsp_rate)) for c in on}
    both = _Both(a, refs)
    for c in on:
        both.SetRXAFMSQRun(c, 1)
    x = _input(nch, sum(calls) * a.dsp_insize, start_on)
    r = dict(ya=[], yc=[], yr={c: [] for c in on}, g={c: [] for c in on}, ends={c: [] for c in on}, rends={c: [] for c in on},
             cross={c: np.inf for c in on}, tail={c: np.inf for c in on}, ntails={c: 0 for c in on})
    last_av = {c: None for c in on}
    pos = 0
    try:
        for k, nb in enumerate(calls):
            if between:
                between(k, a, c_, b, both, refs, loops)
            xa = np.ascontiguousarray(x[:, pos:pos + nb * a.dsp_insize])
            pa, pc, pb = a.process_host(xa), c_.process_host(xa), b.process_host(xa)
            r["ya"].append(pa); r["yc"].append(pc)
            for c in on:
                ref = refs[c]
                out = ref.process(loops[c].process(pb[c]), pc[c])
                r["yr"][c].append(out); r["g"][c].append(ref.gain)
                d = a.debug_fmsq(c)
                r["ends"][c].append((d[2], d[3], d[4]))
                r["rends"][c].append((ref.state, ref.count, ref.ready))
                if ref.run:
                    av = ref.av if last_av[c] is None else np.concatenate([[last_av[c]], ref.av])
                    cr, tl = margins(av, (ref.tail_thresh, ref.unmute_thresh), ref.tails)
                    r["cross"][c] = min(r["cross"][c], cr); r["tail"][c] = min(r["tail"][c], tl); r["ntails"][c] += len(ref.tails)
                    last_av[c] = ref.av[-1]
                    # the averages themselves, to the margin the decisions are held to, from 1.5 s on: nbp0's first outputs are
                    # rounding-sized and the loop's phase detector takes their angle, so where A's tiles are not B's (nc 4096: 8192
                    # points) a few of B's first trigger samples are not A's; they pass the filter's main lobe once (seen: longnoise
                    # 3e-2 apart there) and longnoise forgets them with tau 0.1 s (e^-14 by 1.5 s)
                    if pos // (FS // dsp_rate) >= 3 * dsp_rate // 2:
                        assert abs(d[0] - ref.avnoise) <= 1e-6 * ref.avnoise and abs(d[1] - ref.longnoise) <= 1e-6 * ref.longnoise, (c, k, d)
            pos += nb * a.dsp_insize
    finally:
        a.close(); c_.close(); b.close()
    r["ya"], r["yc"] = np.concatenate(r["ya"], 1), np.concatenate(r["yc"], 1)
    for c in on:
        r["yr"][c], r["g"][c] = np.concatenate(r["yr"][c]), np.concatenate(r["g"][c])
    if compare:
        _check(r, on)
    return r


def _check(r, on, min_opens=2):
    for c in on:
        # the margins of the trigger actually used, first: a near miss there would make the comparison below a coin toss
        print("channel %d: crossing margin %.3g, tail margin %.3g over %d tails" % (c, r["cross"][c], r["tail"][c], r["ntails"][c]))
        assert r["cross"][c] > 1e-6 and r["tail"][c] > 1e-3, (c, r["cross"][c], r["tail"][c])
        g = r["g"][c]
        opens = int(np.sum((g[:-1] == 0.0) & (g[1:] != 0.0)))
        assert opens >= min_opens and r["ntails"][c] >= 1, (c, opens, r["ntails"][c])
        assert r["ends"][c] == r["rends"][c], (c, [(k, e, f) for k, (e, f) in enumerate(zip(r["ends"][c], r["rends"][c])) if e != f][:3])
        muted = g == 0.0
        ya = r["ya"][c]
        assert not np.any(ya[muted]), (c, int(np.sum(ya[muted] != 0)), np.flatnonzero(ya[muted] != 0)[:5])
        err = rel_rms(ya, r["yr"][c])
        print("channel %d: A against g C, relative RMS %.3g" % (c, err))
        assert err < TOL, (c, err)


def test_ragged_calls_in_a_mixed_engine(qh):
    """two FMSQ channels (one tile pair), an FM channel without it and a USB channel beside them: the engine's two-stream path, where the
    CTCSS notch stores the caller's rows itself and the squelch follows there.  The calls around the first carrier's end are one block
    (256 samples) long, so the 481-sample ramp down cannot pass between two call ends: both ramps' and the tail's states are met there."""
    modes = [FM, FM, FM, USB]
    calls = (3, 1, 17) + (7,) * 30 + (1,) * 70 + (480, 5, 2)         # blocks 231 .. 301 (1.23 .. 1.61 s) one by one
    r = _run(qh, modes, (0, 1), calls=calls, start_on=(1,))
    states = {s for c in (0, 1) for s, _, _ in r["ends"][c][:-1]}
    assert {MUTED, INCREASE, UNMUTED, TAIL, DECREASE} <= states, states
    assert np.array_equal(r["ya"][2], r["yc"][2]) and np.array_equal(r["ya"][3], r["yc"][3])      # the channels beside them: the same bits


def test_threshold_changed_mid_stream(qh):
    def between(k, a, c, b, both, refs, loops):
        if k == 20:
            both.SetRXAFMSQThreshold(0, 0.5)
        elif k == 43:
            both.SetRXAFMSQThreshold(0, 1.0)

    _run(qh, [FM], (0,), between=between)


def test_run_off_and_on_with_the_state_frozen(qh):
    """off while the carrier is away (MUTED), on again in mid-carrier: nothing of the stage moved meanwhile, the delay line included, so
    the squelch opens from the old averages; while off the channel's output is C's"""
    cuts = {}

    def between(k, a, c, b, both, refs, loops):
        if k == 2:                       # 21 blocks = 0.11 s: still off the carrier, muted
            both.SetRXAFMSQRun(0, 0)
            cuts["state"] = (refs[0].state, refs[0].avnoise, refs[0].count)
        elif k == 30:                    # 0.11 + 27 * 7 * 5.33 ms = 1.12 s: on the carrier
            assert (refs[0].state, refs[0].avnoise, refs[0].count) == cuts["state"]
            assert a.debug_fmsq(0)[2] == MUTED
            both.SetRXAFMSQRun(0, 1)

    r = _run(qh, [FM, FM], (0,), between=between)
    starts = np.cumsum((0,) + CALLS) * 256
    assert np.array_equal(r["ya"][0, starts[2]:starts[30]], r["yc"][0, starts[2]:starts[30]])
    assert np.any(r["yc"][0, starts[2]:starts[30]] != 0)


def test_flush_in_mid_carrier(qh):
    """qh_rxa_flush with the squelch open: muted again for the ready delay, then the ramp up"""
    def between(k, a, c, b, both, refs, loops):
        if k == 30:
            assert refs[0].state == UNMUTED
            for e in (a, c, b):
                e.flush()
            refs[0].flush(); loops[0].flush()

    r = _run(qh, [FM], (0,), between=between)
    s = int(np.cumsum((0,) + CALLS)[30]) * 256
    n = ready_count(48000)
    assert not np.any(r["ya"][0, s:s + n - 1]) and np.any(r["ya"][0, s + n:s + n + 4800])


def _library_mp_taps(tmp_path, nc, rate, size):
    """qh::mp_imp of qh::fmsq_impulse, from the library's host design unit compiled here (as tests/test_design_eq_host.py does): see Fmsq's
    `taps` for why a minimum-phase case cannot take its taps from anywhere else.  What the case then holds is the stage's use of them."""
    import ctypes as C
    import os
    import shutil
    import subprocess
    assert shutil.which("g++"), "the minimum-phase case compiles qh_design.cpp"
    csrc = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "quisk_amd", "csrc")
    (tmp_path / "shim.cpp").write_text('''
#include <cstring>
#include "qh_design.hpp"
extern "C" void t_fmsq_mp(int nc, double fs, double scale, double *out)
{ auto h = qh::mp_imp(qh::fmsq_impulse(nc, fs, scale), 16, 0); std::memcpy(out, h.data(), h.size() * 16); }
''')
    so = tmp_path / "libfmsqmp.so"
    subprocess.run(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-I", csrc, str(tmp_path / "shim.cpp"), os.path.join(csrc, "qh_design.cpp"), "-o", str(so)], check=True)
    out = np.zeros(nc, dtype=np.complex128)
    C.CDLL(str(so)).t_fmsq_mp(C.c_int(nc), C.c_double(rate), C.c_double(1.0 / (2.0 * size)), out.ctypes.data_as(C.c_void_p))
    return out * (2.0 * size)


@pytest.mark.parametrize("nc,mp", [(256, 0), (4096, 0), (2048, 1)])
def test_noise_filter_lengths_and_minimum_phase(qh, tmp_path, nc, mp):
    """nc 256 (= dsp_size) and minimum phase through the squelch's own setters, nc 4096 through RXASetNC on all three engines: an engine
    takes 8192-point tiles as soon as one running stage has nc > 2048, and with the squelch alone at 4096 A's FM chain would run on
    other tiles than C's -- the two then differ by what the loop's acquisition leaves ringing (4.6e-9 seen), which is not the squelch's"""
    def prep(e):
        if nc > 2048:
            e.RXASetNC(-1, nc)
        else:
            e.SetRXAFMSQNC(-1, nc)
        e.SetRXAFMSQMP(-1, mp)

    kw = dict(nc=nc, mp=mp)
    if mp:
        kw["taps"] = _library_mp_taps(tmp_path, nc, 48000.0, 256)
    _run(qh, [FM, FM], (0, 1), prep=prep, prep_b=True, ref_kw=kw, calls=(3, 1, 17) + (21,) * 14 + (470, 3), start_on=(1,))


def test_96k(qh):
    calls = (5, 2) + (19,) * 30 + (1000, 3)                  # blocks of 512 input samples, 256 at 96 kHz: 4.2 s
    r = _run(qh, [FM, USB], (0,), calls=calls, dsp_rate=96000)
    assert INCREASE in {s for s, _, _ in r["ends"][0]}


def test_limiter_on(qh):
    """the detector limiter (fmd.c:179-184) ahead of the squelch, on A and C alike"""
    def prep(e):
        e.SetRXAFMLimRun(0, 1)

    _run(qh, [FM, FM], (0,), prep=prep, calls=(3, 1, 17) + (21,) * 14 + (470, 3))


def test_agc_mode_3_behind_the_squelch(qh):
    """AGC mode 3 set on the squelched channel.  (SetRXAMode (FM) holds xwcpagc's run flag at 0, RXA.c:777, and no setter raises it, so
    the mode is kept for the next mode change and the AGC does not run here; were it to run, the squelch's output, zeros included, would
    feed it, RXA.c:575-583 -- the squelch works in place ahead of it.)  No oracle claim: the calls A's own state says were muted throughout
    are exactly 0, everything is finite, the channel is heard once the squelch opens and the channel beside it is never silent."""
    modes = [FM, FM]
    a = _engine(qh, modes)
    x = _input(2, sum(CALLS) * 1024)
    a.SetRXAAGCMode(0, 3); a.SetRXAFMSQRun(0, 1)
    pos, outs, states = 0, [], []
    try:
        for nb in CALLS:
            outs.append(a.process_host(np.ascontiguousarray(x[:, pos:pos + nb * 1024])))
            states.append(a.debug_fmsq(0)[2])
            pos += nb * 1024
    finally:
        a.close()
    assert np.all(np.isfinite(np.concatenate(outs, 1)))
    muted = [k for k in range(1, len(CALLS)) if states[k - 1] == MUTED and states[k] == MUTED and CALLS[k] < 100]
    assert len(muted) >= 5 and all(not np.any(outs[k][0]) for k in muted)
    assert UNMUTED in states and any(np.any(o[0]) for o in outs) and all(np.any(o[1]) for o in outs[3:])


def test_refusals_leave_the_next_valid_call_working(qh):
    lib = qh.load()
    x = _input(2, 8 * 1024)
    e, ref = _engine(qh, [FM, FM]), _engine(qh, [FM, FM])
    try:
        for g in (e, ref):
            g.SetRXAFMSQRun(0, 1)
        want = ref.process_host(x)
        for bad in (float("nan"), float("inf"), -float("inf")):
            assert lib.qh_rxa_SetRXAFMSQThreshold(e._h, 0, bad) == -2          # QH_ERR_INVALID, nothing changed
        # FMSQ on a channel whose FM detector is off
        e.SetRXAMode(1, USB); e.SetRXAFMSQRun(1, 1)
        with pytest.raises(qh.QuiskHipError, match="FM detector is off"):
            e.process_host(x)
        e.SetRXAFMSQRun(1, 0); e.SetRXAMode(1, FM)
        # nc above 4096 while the stage runs; differing nc / mp among FMSQ channels
        e.SetRXAFMSQNC(0, 8192)
        with pytest.raises(qh.QuiskHipError, match="exceeds 4096"):
            e.process_host(x)
        e.SetRXAFMSQNC(0, 2048); e.SetRXAFMSQRun(1, 1); e.SetRXAFMSQNC(1, 1024)
        with pytest.raises(qh.QuiskHipError, match="different nc or mp"):
            e.process_host(x)
        e.SetRXAFMSQNC(1, 2048); e.SetRXAFMSQMP(1, 1)
        with pytest.raises(qh.QuiskHipError, match="different nc or mp"):
            e.process_host(x)
        e.SetRXAFMSQMP(1, 0); e.SetRXAFMSQRun(1, 0)
        assert lib.qh_rxa_SetRXAFMSQNC(e._h, 0, 100) == -3 and lib.qh_rxa_SetRXAFMSQNC(e._h, 0, 128) == -3   # QH_ERR_UNSUPPORTED: not a power of two, below dsp_size
        got = e.process_host(x)                                  # nothing of the refused calls ran: the first block of the stream
        assert np.array_equal(got[0], want[0]) and rel_rms(got[1], want[1]) < 1e-12
    finally:
        e.close(); ref.close()
    # a dsp rate at or below twice the loop's pole frequency (15.8 kHz)
    low = qh.RxaEngine(1, dsp_size=64, in_rate=48000, dsp_rate=12000, out_rate=12000)
    try:
        low.SetRXAMode(0, FM); low.SetRXAFMSQRun(0, 1)
        with pytest.raises(qh.QuiskHipError, match="pole"):
            low.process_host(np.zeros((1, 4 * low.dsp_insize), dtype=np.complex128))
        low.SetRXAFMSQRun(0, 0)
        assert low.process_host(np.zeros((1, 4 * low.dsp_insize), dtype=np.complex128)).shape == (1, 4 * low.dsp_outsize)
    finally:
        low.close()
