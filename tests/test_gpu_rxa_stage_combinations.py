"""The stages the whole-chain oracle leaves out (xfmsq, xeqp, xcbl / xspeak / xmpeak, xssql) beside one live neighbour each, and all of
them at once, against the composed whole-chain reference (tests/rxa_chain_ref.py).  -m gpu.

The stages' own tests (test_gpu_rxa_eqp.py, test_gpu_rxa_audio_peak.py, test_gpu_rxa_ssql.py, test_gpu_rxa_fmsq.py) hold each in a
configuration built to isolate it: a fixed gain, an identity panel, nothing non-linear behind it or time-varying ahead of it.  Here the
neighbour is what those leave out: an AGC that works (mode 3; mode 1 with its hang), ANF at either position, ANR, EMNR at either position,
AMSQ, bp1 forced on, a notch in nbp0 -- on every channel of a 3-channel engine (USB, AM, LSB; FM, USB, FM for the FM squelch, where the
AGC pairings are left out: SetRXAMode holds xwcpagc off in FM, RXA.c:777), over 114 blocks of 1024 input samples in ragged calls.

Gates, the setter walks' (test_gpu_rxa_fuzz.py): relative RMS over the run per channel under 1e-6, 1e-4 where ANF or ANR runs.  Where the
SSQL restatement's gain is exactly 0 the engine's output is exactly 0 (out_rate = dsp_rate; the panel and AMSQ are real scalar gains).
Before anything is compared the reference's own margins are asserted: no squelch threshold crossing closer than 1e-6, no tail count
closer than 1e-3 to an integer (test_gpu_rxa_fmsq.py's figures).

DEFECT FOUND AND FIXED, by `fmsq beside bp1`: a channel whose bp1 was forced on by SetRXABandpassRun while every channel of the engine was
a linear chain (Engine::run_linear) lost bp1's delay line in the call in which other channels took the engine to the per-mode path.
run_linear flips bp1's ping-pong pair, but the record of which half holds a channel's line (Fircore::Chan, then two loose members) was
kept on the per-mode path only, so after an odd number of linear calls the first per-mode call copied the stale half over the current one.  Seen on
the MI355X before the fix, channel 1 of (USB, USB, USB) with a fixed gain, channels 0 and 2 set to FM before call 3 of (1, 3, 9, 1, 40, 17,
2, 11, 5, 25): rms error / rms of the reference per call 6.8e-14 / 0.82 (call 2), 1.1 / 1.1 (call 3, the first on the per-mode path), 0.31 /
1.1 (call 4), 2.0e-12 / 1.1 from call 5 on; 0.194 over the run.  The same with and without the FM squelch, and with AM in FM's place.
`test_bp1_forced_on_keeps_its_delay_line_when_the_engine_leaves_the_linear_path` is the smallest case."""
import numpy as np
import pytest

from conftest import rel_rms
from quisk_amd import synth
from rxa_chain_ref import RxaChainRef, keyed_fm_over_a_floor
from rxa_ssql_ref import syllabic

pytestmark = pytest.mark.gpu

FS = 192000
CALLS = (1, 3, 9, 1, 40, 17, 2, 11, 5, 25)
# An FM channel spends the first 3 calls (13 blocks) in USB and enters FM with its filters primed, as in the setter walks: nbp0's first
# outputs are rounding-sized, the loop's phase detector takes their angle, and what the detector makes of them is no one's to compare.
FM_AT = 3
LSB, USB, FM, AM = 0, 1, 5, 6
G4 = [2, -6, 5, 9]
G10 = [3, -12, 12, -6, 9, 0, -12, 12, 4, -9, 7]
P3 = (3, [0.0, 400.0, 1500.0, 5000.0], [-2.0, 6.0, -9.0, 3.0])
STAGES = ("eqp", "peaks", "ssql", "fmsq")
NEIGHBOURS = ("agc3", "agc1_hang", "anf0", "anf1", "anr", "emnr0", "emnr1", "amsq", "bp1", "notch")
CASES = [(s, n) for s in STAGES for n in NEIGHBOURS if not (s == "fmsq" and n.startswith("agc"))]
# (tried and replaced, by the reference's margins alone: ("emnr1", "anf0") -- behind the muted FM squelch EMNR at position 1 hands SSQL's
# crossing counter a sample of 8e-21 ahead of a step over 0.01, whose sign is rounding's; and without an AGC the AM channel's SSQL
# stays shut behind EMNR or ANF)
ALL_ON = (("agc3",), ("agc1_hang", "amsq"), ("agc3", "emnr0", "anf1"))


def _input(modes, n, fs=FS):
    """what makes the squelches work: a hopping tone 0.15 s on, a steady one 0.2 s in between (syllabic); an FM carrier keyed 0.3 s high /
    0.22 s low over noise (keyed_fm_over_a_floor); each on its channel's carrier"""
    t = np.arange(n) / fs
    x = np.empty((len(modes), n), dtype=np.complex128)
    for c, m in enumerate(modes):
        car = np.exp(-2j * np.pi * ((synth.shift_freq(c) * t) % 1.0))
        if m == FM:
            x[c] = keyed_fm_over_a_floor(n, fs, seed=3 + 4 * c) * car
            continue
        z = syllabic(n, fs, seed=40 + c, on=0.15, off=0.2, rest=1100.0)
        x[c] = ((0.1 + 0.05 * z.real) if m == AM else 0.3 * (np.conj(z) if m == USB else z)) * car     # (USB: the input's negative side)
    return x


class _Both:
    """a setter on the engine's channel c and on that channel's reference"""

    def __init__(self, e, refs):
        self.e, self.refs = e, refs

    def __getattr__(self, name):
        def call(c, *a):
            getattr(self.e, name)(c, *a)
            getattr(self.refs[c], name)(*a)
        return call


def _base(b, c, mode):
    b.SetRXAShiftRun(c, 1); b.SetRXAShiftFreq(c, synth.shift_freq(c)); b.RXANBPSetRun(c, 1)
    b.SetRXAMode(c, USB if mode == FM else mode)        # (FM is entered FM_AT calls in, run_case)
    b.RXASetPassband(c, *{USB: (300.0, 3000.0), LSB: (-3000.0, -300.0), AM: (-4000.0, 4000.0), FM: (-8000.0, 8000.0)}[mode])
    b.SetRXAAGCMode(c, 0); b.SetRXAAGCFixed(c, 10.0)


def _stage(b, c, mode, stage):
    if stage == "eqp":
        b.SetRXAEQRun(c, 1)
        (lambda: b.SetRXAGrphEQ10(c, G10), lambda: b.SetRXAEQProfile(c, *P3), lambda: b.SetRXAGrphEQ(c, G4))[c]()
    elif stage == "cbl_spcw":
        b.SetRXACBLRun(c, 1); b.SetRXASPCWRun(c, 1); b.SetRXASPCWFreq(c, 900.0 + 200.0 * c); b.SetRXASPCWBandwidth(c, 300.0)
    elif stage == "mpeak":
        b.SetRXAmpeakRun(c, 1); b.SetRXAmpeakFilFreq(c, 0, 500.0 + 100.0 * c); b.SetRXAmpeakFilFreq(c, 1, 1700.0); b.SetRXAmpeakFilBw(c, 1, 250.0)
    elif stage == "peaks":
        _stage(b, c, mode, "cbl_spcw"); _stage(b, c, mode, "mpeak")
    elif stage == "ssql":
        b.SetRXASSQLRun(c, 1); b.SetRXASSQLTauMute(c, 0.05)
    elif stage == "fmsq" and mode == FM:
        b.SetRXAFMSQRun(c, 1)


def _neighbour(b, c, mode, nb):
    if nb == "agc3":
        b.SetRXAAGCMode(c, 3)
    elif nb == "agc1_hang":
        b.SetRXAAGCMode(c, 1); b.SetRXAAGCHang(c, 100); b.SetRXAAGCHangThreshold(c, 20)
    elif nb in ("anf0", "anf1"):
        b.SetRXAANFRun(c, 1); b.SetRXAANFPosition(c, int(nb[-1]))
    elif nb == "anr":
        b.SetRXAANRRun(c, 1)
    elif nb in ("emnr0", "emnr1"):
        b.SetRXAEMNRRun(c, 1); b.SetRXAEMNRPosition(c, int(nb[-1]))
    elif nb == "amsq":
        b.SetRXAAMSQRun(c, 1); b.SetRXAAMSQThreshold(c, -40.0)
    elif nb == "bp1":
        b.SetRXABandpassRun(c, 1)
    elif nb == "notch":
        b.RXANBPSetNotchesRun(c, 1); b.RXANBPAddNotch(c, 0, -1000.0 if mode == LSB else 1000.0, 200.0, 1)


def run_case(engine, modes, stages, neighbours, calls=CALLS):
    """engine: the 3-channel engine, or None for the reference alone (margins without a GPU).  stages: per channel, the stages to switch
    on.  Returns (engine output or None, reference output, per-channel SSQL gain, the references)."""
    refs = [RxaChainRef() for _ in modes]

    class _RefOnly:
        def __getattr__(self, name):
            return lambda c, *a: None
    b = _Both(engine if engine is not None else _RefOnly(), refs)
    for c, m in enumerate(modes):
        _base(b, c, m)
        for nb in neighbours:
            _neighbour(b, c, m, nb)
        for s in stages[c]:
            if s != "fmsq":
                _stage(b, c, m, s)
    x = _input(modes, sum(calls) * 1024)
    ys, rs, gs, pos = [], [], [], 0
    for k, nb in enumerate(calls):
        if k == FM_AT:
            for c, m in enumerate(modes):
                if m == FM:
                    b.SetRXAMode(c, FM)
                    _stage(b, c, m, "fmsq" if "fmsq" in stages[c] else "")
        seg = np.ascontiguousarray(x[:, pos * 1024:(pos + nb) * 1024])
        pos += nb
        if engine is not None:
            ys.append(engine.process_host(seg))
        rs.append(np.stack([r.xrxa(seg[c]) for c, r in enumerate(refs)]))
        gs.append(np.stack([r.ssql_gain for r in refs]))
    return (np.concatenate(ys, 1) if ys else None), np.concatenate(rs, 1), np.concatenate(gs, 1), refs


def hold(y, ref, gain, refs, lms, what):
    for c, r in enumerate(refs):                        # the reference's own conditioning first: an assertion, not a skip
        m = r.margins()
        assert r.margins_ok(), (what, c, m)
    for c, r in enumerate(refs):
        assert np.all(np.isfinite(ref[c])), (what, c)
        muted = gain[c] == 0.0
        assert not np.any(y[c][muted]), (what, c, int(np.sum(y[c][muted] != 0)), np.flatnonzero(y[c][muted] != 0)[:5])
        if np.abs(ref[c]).max() < 1e-9:                 # (a squelch that stays shut: nothing to take a ratio of, as in the walks)
            continue
        err, tol = rel_rms(y[c], ref[c]), 1e-4 if lms else 1e-6
        print("%s, channel %d: relative RMS %.3g (tolerance %.0e); ran %r, cycles %r, margins %r" % (what, c, err, tol, r.ran, r.cycles(), r.margins()))
        assert err < tol, (what, c, err)


def case_setup(stage, neighbours):
    """(modes, per-channel stages)"""
    if stage == "fmsq":
        return (FM, USB, FM), (("fmsq",), (), ("fmsq",))
    if stage == "all":
        return (USB, AM, FM), (("eqp", "cbl_spcw", "ssql"), ("eqp", "mpeak", "ssql"), ("fmsq", "eqp", "ssql"))
    return (USB, AM, LSB), ((stage,),) * 3


def _case(qh, stage, neighbours):
    modes, stages = case_setup(stage, neighbours)
    e = qh.RxaEngine(3)
    try:
        e.load_emnr_tables()
        y, ref, gain, refs = run_case(e, modes, stages, neighbours)
    finally:
        e.close()
    what = "%s beside %s" % (stage, "+".join(neighbours))
    hold(y, ref, gain, refs, any(n in ("anf0", "anf1", "anr") for n in neighbours), what)
    want = {"eqp": "eqp", "peaks": "peaks", "cbl_spcw": "peaks", "mpeak": "peaks", "ssql": "ssql", "fmsq": "fmsq"}
    for c, r in enumerate(refs):                        # the case is what it says: every stage asked for ran on every block
        for s in stages[c]:
            assert r.ran[want[s]] == sum(CALLS[FM_AT:] if s == "fmsq" else CALLS), (what, c, s, r.ran)
    return refs, gain


@pytest.mark.parametrize("stage,neighbour", CASES)
def test_stage_beside_a_live_neighbour(qh, stage, neighbour):
    refs, gain = _case(qh, stage, (neighbour,))
    if stage in ("ssql", "fmsq"):                       # a squelch that never moved would make its case an empty one: shut and open on two channels
        worked = [c for c, r in enumerate(refs) if r.ran[stage] and np.any(r.run_gain(stage) == 0.0) and np.any(r.run_gain(stage) == 1.0)]
        assert len(worked) >= 2, (stage, neighbour, worked)


@pytest.mark.parametrize("neighbours", ALL_ON, ids=["+".join(n) for n in ALL_ON])
def test_every_stage_a_mode_allows_at_once(qh, neighbours):
    """USB: EQP + CBL + SPCW + SSQL; AM: EQP + mpeak + SSQL; FM: FMSQ + EQP + SSQL, in one engine"""
    refs, _ = _case(qh, "all", neighbours)
    assert [r.live_max for r in refs] == [4, 3, 3]


@pytest.mark.parametrize("calls,fm_at", [((1, 3, 9, 1, 12), 3), ((4, 9, 1, 12), 2)], ids=["three_linear_calls", "two_linear_calls"])
def test_bp1_forced_on_keeps_its_delay_line_when_the_engine_leaves_the_linear_path(qh, oracle, calls, fm_at):
    """Three USB channels with a fixed gain, bp1 forced on (SetRXABandpassRun, bandpass.c:385-390: no flush) on channel 1; after 13 blocks
    channels 0 and 2 go to FM, which takes the engine from the linear path to the per-mode one.  Channel 1 has seen no setter: its
    output is the oracle's throughout.  (Found by `fmsq beside bp1` above, 0.194 over that case's run.  Before the fix this case gave
    0.475 over the run on the MI355X; rms error / rms of the reference per call 7.3e-22/9.8e-14, 2.5e-18/6.8e-07, 6.8e-14/0.82, 1.1/1.1,
    0.57/1.1 -- the whole of the first per-mode call wrong; see the module's docstring.)  Both parities of the number of linear calls:
    the stale half was the current one after an odd number only."""
    x = _input((USB, USB, USB), sum(calls) * 1024)
    e = qh.RxaEngine(3)
    o = oracle.WdspChannel(1024, 256, FS, 48000, 48000)
    try:
        for c in range(3):
            for t, lead in ((e, (c,)),) + (((o, ()),) if c == 1 else ()):
                t.SetRXAShiftRun(*lead, 1); t.SetRXAShiftFreq(*lead, synth.shift_freq(c)); t.RXANBPSetRun(*lead, 1)
                t.SetRXAMode(*lead, USB); t.RXASetPassband(*lead, 300.0, 3000.0); t.SetRXAAGCMode(*lead, 0); t.SetRXAAGCFixed(*lead, 10.0)
        e.SetRXABandpassRun(1, 1); o.SetRXABandpassRun(1)
        ys, rs, pos = [], [], 0
        for k, nb in enumerate(calls):
            if k == fm_at:
                e.SetRXAMode(0, FM); e.SetRXAMode(2, FM)
            seg = np.ascontiguousarray(x[:, pos * 1024:(pos + nb) * 1024])
            pos += nb
            ys.append(e.process_host(seg)[1]); rs.append(o.xrxa(seg[1]))
    finally:
        e.close()
    per = ["%.1e/%.1e" % (np.sqrt(np.mean(np.abs(a - b) ** 2)), np.sqrt(np.mean(np.abs(b) ** 2))) for a, b in zip(ys, rs)]
    err = rel_rms(np.concatenate(ys), np.concatenate(rs))
    print("channel 1: relative RMS %.3g; per call rms error / rms of the reference %r" % (err, per))
    assert err < 1e-6, (err, per)
