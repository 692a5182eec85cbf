"""The composed whole-chain reference (tests/rxa_chain_ref.py) on the CPU: without its hooks it is the oracle bit for bit; in each stage's
isolating configuration it reproduces the identity that stage's GPU test rests on (tests/test_gpu_rxa_eqp.py, test_gpu_rxa_ssql.py,
test_gpu_rxa_audio_peak.py, test_gpu_rxa_fmsq.py), to 1e-12 relative RMS over the run; and whole runs and block-by-block feeding give the
same bits.  Call by call the same 1e-12 is held against the RMS of the stage's output or of its input, whichever is larger: a filter
rounds at 1e-16 of what it is fed, and in its first calls a filter of 2048 taps puts out 1e-6 of that (its leading tail alone)."""
import numpy as np
import pytest

from conftest import rel_rms
from quisk_amd import synth
from rxa_audio_peak_ref import AudioPeakChain
from rxa_chain_ref import RxaChainRef, count_cycles
from rxa_ssql_ref import Ssql, syllabic
from wdsp_eqp_ref import Eqp
from wdsp_fmsq_ref import keyed_fm

FS = 192000
TOL = 1e-12
CALLS = (1, 3, 9, 1, 40, 17, 2)
G10 = [3, -12, 12, -6, 9, 0, -12, 12, 4, -9, 7]


def _setup(t, mode=1, agc=0, gain1=None, c=0):
    t.SetRXAShiftRun(1); t.SetRXAShiftFreq(synth.shift_freq(c)); t.RXANBPSetRun(1)
    t.SetRXAMode(mode)
    t.RXASetPassband(*((-8000.0, 8000.0) if mode == 5 else (-4000.0, 4000.0) if mode == 6 else (300.0, 3000.0)))
    t.SetRXAAGCMode(agc)
    if agc == 0:
        t.SetRXAAGCFixed(10.0)
    if gain1 is not None:
        t.SetRXAPanelGain1(gain1)
    return t


def _carrier(z, c=0):
    t = np.arange(len(z)) / FS
    return z * np.exp(-2j * np.pi * ((synth.shift_freq(c) * t) % 1.0))


class _Held:
    """err < 1e-12 of max(rms(want), rms(fed)) for every call, and relative RMS < 1e-12 over the run"""

    def __init__(self):
        self.e2 = self.w2 = 0.0

    def call(self, got, want, fed, k):
        e2, w2 = float(np.sum(np.abs(got - want) ** 2)), float(np.sum(np.abs(want) ** 2))
        assert np.sqrt(e2) <= TOL * np.sqrt(max(w2, float(np.sum(np.abs(fed) ** 2)))), (k, np.sqrt(e2), np.sqrt(w2))
        self.e2 += e2; self.w2 += w2

    def run(self):
        assert self.w2 > 0.0 and np.sqrt(self.e2 / self.w2) < TOL, np.sqrt(self.e2 / max(self.w2, 1e-300))


def _calls(x, calls=CALLS):
    pos = 0
    for nb in calls:
        yield x[pos * 1024:(pos + nb) * 1024]
        pos += nb


def test_without_hooks_it_is_the_oracle_over_a_walk_of_the_existing_menu(oracle):
    """also with the hooks set and every hooked stage off: the call sites alone move no bit"""
    from test_gpu_rxa_fuzz import _apply
    rng = np.random.default_rng(7)
    seglen = [int(rng.integers(1, 6)) for _ in range(30)]
    x = synth.make_input_numpy(1, sum(seglen) * 1024)[0]
    plain = _setup(oracle.WdspChannel(1024, 256, FS, 48000, 48000), agc=3)
    unset, idle = _setup(RxaChainRef(hooks=False), agc=3), _setup(RxaChainRef(), agc=3)
    pos = 0
    for s, n in enumerate(seglen):
        if s:
            _apply(rng, [(plain, ()), (unset, ()), (idle, ())])
        seg = x[pos * 1024:(pos + n) * 1024]
        want = plain.xrxa(seg)
        assert np.array_equal(unset.xrxa(seg), want), s
        assert np.array_equal(idle.xrxa(seg), want), s
        pos += n
    assert not any(idle.ran.values()) and idle.live_max == 0 and all(np.isinf(v) for v in idle.margins().values())


def test_eqp_is_the_restatement_behind_the_chain_without_it():
    """USB, a fixed gain, the default panel: composed(EQ on) = Eqp(oracle(EQ off)), call by call, setters between calls"""
    x = synth.make_input_numpy(1, sum(CALLS) * 1024)[0]
    a, b, eq = _setup(RxaChainRef()), _setup(RxaChainRef(hooks=False)), Eqp(48000)
    for t in (a, eq):
        t.SetRXAEQRun(1); t.SetRXAGrphEQ10(G10)
    held = _Held()
    for k, seg in enumerate(_calls(x)):
        if k == 3:
            for t in (a, eq):
                t.SetRXAEQWintype(1); t.SetRXAEQNC(1024)
        if k == 5:
            for t in (a, eq):
                t.SetRXAEQProfile(3, [0.0, 400.0, 1500.0, 5000.0], [-2.0, 6.0, -9.0, 3.0]); t.SetRXAEQCtfmode(1)
        fed = b.xrxa(seg)
        held.call(a.xrxa(seg), eq.process(fed), fed, k)
    held.run()
    assert a.ran["eqp"] == sum(CALLS) and a.live_max == 1


def test_rxasetnc_and_rxasetmp_reach_the_equalizer_and_the_fm_squelch():
    a = RxaChainRef()
    a.RXASetNC(1024)
    assert a.eqp.nc == 1024 and a.fmsq.nc == 1024 and len(a.eqp.delay) == 1023
    a.RXASetMP(1)
    assert a.eqp.mp == 1 and a.fmsq.mp == 1 and np.iscomplexobj(a.fmsq.h) and len(a.fmsq.h) == 1024
    a.RXASetNC(512); a.RXASetMP(0)
    assert (a.eqp.nc, a.eqp.mp, a.fmsq.nc, a.fmsq.mp) == (512, 0, 512, 0) and len(a.fmsq.h) == 512 and not np.iscomplexobj(a.fmsq.h)


@pytest.mark.parametrize("mode", [1, 6])
def test_ssql_behind_an_identity_panel(mode):
    """composed(SSQL on) = Ssql(oracle(SSQL off)) with gain1 = 1: the squelch is the last stage ahead of the panel"""
    n = 230 * 1024
    z = syllabic(n, FS, seed=1, on=0.3, off=0.3, rest=1100.0)
    x = _carrier((0.1 + 0.05 * z.real) if mode == 6 else 0.3 * np.conj(z))     # (the chain's upper sideband is the input's negative frequencies)
    agc = 3 if mode == 6 else 0         # (xftov counts a zero crossing from a step of 0.01 up, ssql.c:86: USB with the fixed gain, so that every tone counts)
    a, b, sq = _setup(RxaChainRef(), mode, agc=agc, gain1=1.0), _setup(RxaChainRef(hooks=False), mode, agc=agc, gain1=1.0), Ssql(48000)
    a.SetRXASSQLRun(1); sq.SetRXASSQLRun(1)
    gains, held = [], _Held()
    for k, seg in enumerate(_calls(x, (3, 1, 17) + (7,) * 29 + (6,))):
        if k == 12:
            a.SetRXASSQLTauMute(0.05); sq.SetRXASSQLTauMute(0.05)
        fed = b.xrxa(seg)
        want = sq.process(fed)
        got = a.xrxa(seg)
        held.call(got, want, fed, k)
        assert np.array_equal(a.ssql_gain, sq.gain)
        assert not np.any(got[a.ssql_gain == 0.0])
        gains.append(sq.gain)
    held.run()
    assert a.cycles()["ssql"] == count_cycles(np.concatenate(gains)) >= 1
    m = a.margins()
    assert np.isfinite(m["ssql_trigger"]) and np.isfinite(m["ssql_window"]) and np.isinf(m["fmsq_cross"])


def test_the_peak_chain_behind_an_identity_panel():
    x = synth.make_input_numpy(1, sum(CALLS) * 1024)[0]
    a, b, pk = _setup(RxaChainRef(), 4, agc=3, gain1=1.0), _setup(RxaChainRef(hooks=False), 4, agc=3, gain1=1.0), AudioPeakChain(48000)
    for t in (a, pk):
        t.SetRXACBLRun(1); t.SetRXASPCWRun(1); t.SetRXASPCWFreq(700.0)
    held = _Held()
    for k, seg in enumerate(_calls(x)):
        if k == 4:
            for t in (a, pk):
                t.SetRXAmpeakRun(1); t.SetRXAmpeakFilFreq(0, 650.0); t.SetRXASPCWRun(0)
        fed = b.xrxa(seg)
        held.call(a.xrxa(seg), pk.process(fed), fed, k)
    held.run()
    assert a.ran["cbl"] == a.ran["peaks"] == sum(CALLS) and a.live_max == 2


def test_fmsq_is_its_gain_times_the_fm_channel_without_it():
    """FM: nothing with memory follows the squelch (the AGC is off in FM, RXA.c:777), so composed = g * oracle(without)"""
    calls = (3, 1, 17) + (7,) * 40
    x = _carrier(keyed_fm(sum(calls) * 1024, FS, seed=3, off=0.25, on=0.45))
    a, b = _setup(RxaChainRef(), 5), _setup(RxaChainRef(hooks=False), 5)
    a.SetRXAFMSQRun(1)
    held = _Held()
    for k, seg in enumerate(_calls(x, calls)):
        if k == 20:
            a.SetRXAFMSQThreshold(0.6)
        got, plain = a.xrxa(seg), b.xrxa(seg)
        want = plain * a.fmsq_gain
        want[a.fmsq_gain == 0.0] = 0.0
        held.call(got, want, plain, k)
    held.run()
    assert a.cycles()["fmsq"] >= 1 and a.ran["fmsq"] == sum(calls)
    m = a.margins()
    assert np.isfinite(m["fmsq_cross"]) and np.isfinite(m["fmsq_tail"]) and m["fmsq_cross"] > 0.0


def test_whole_runs_and_single_blocks_give_the_same_bits():
    """every hooked stage on at once (AM: equalizer, carrier block, multi-peak filter, SSQL behind AGC mode 3)"""
    n = 60 * 1024
    x = _carrier(0.1 + 0.05 * syllabic(n, FS, seed=2, on=0.1, off=0.08).real)
    outs = []
    for calls in ((60,), (1,) * 60, (1, 3, 9, 1, 40, 6)):
        a = _setup(RxaChainRef(), 6, agc=3)
        a.SetRXAEQRun(1); a.SetRXAGrphEQ10(G10); a.SetRXACBLRun(1); a.SetRXAmpeakRun(1); a.SetRXASSQLRun(1)
        outs.append((np.concatenate([a.xrxa(seg) for seg in _calls(x, calls)]), a.margins(), a.cycles(), a.ran, a.live_max))
    for o in outs[1:]:
        assert np.array_equal(o[0], outs[0][0]) and o[1:] == outs[0][1:]
    assert outs[0][4] == 4 and np.any(outs[0][0])


def test_a_minimum_phase_fm_squelch_on_an_fm_channel():
    """the library's minimum-phase noise filter in the composed chain: the squelch still opens on the carrier"""
    calls = (40,) * 4
    x = _carrier(keyed_fm(sum(calls) * 1024, FS, seed=7, off=0.25, on=0.45))
    a = _setup(RxaChainRef(), 5)
    a.RXASetNC(1024); a.RXASetMP(1); a.SetRXAFMSQRun(1)
    g = np.concatenate([(a.xrxa(seg), a.fmsq_gain)[1] for seg in _calls(x, calls)])
    assert np.any(g == 0.0) and np.any(g == 1.0)


def test_a_hook_that_raises_stops_the_call(oracle):
    o = oracle.WdspChannel(1024, 256, FS, 48000, 48000)

    def bad(where, z, aux):
        raise ValueError("from the hook")
    o.set_stage_hook(bad)
    with pytest.raises(ValueError, match="from the hook"):
        o.xrxa(np.zeros(1024, dtype=np.complex128))
    o.set_stage_hook(None)
    assert o.xrxa(np.zeros(1024, dtype=np.complex128)).shape == (256,)
