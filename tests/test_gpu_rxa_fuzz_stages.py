"""The seeded setter walks of test_gpu_rxa_fuzz.py with the FM squelch, the equalizer, the carrier block, the peak filters and SSQL in the
chain: a third menu (_apply3) draws their setters under the WDSP names beside the two existing menus (_apply, _apply2, imported), on four
channels (USB, AM, LSB and one that enters FM early in the walk and may leave it), against the composed whole-chain reference (tests/rxa_chain_ref.py),
one reference per channel.  -m gpu.

Gates: _walk's.  Relative RMS over the whole run per channel under 1e-6, under 1e-4 for a channel on which ANF or ANR ever ran, under
1e-5 for a long minimum-phase channel; channels whose reference stays under 1e-9 are skipped.  Every sample for which the SSQL
restatement's gain is exactly 0 is exactly 0 in the engine's output.  Before a walk compares anything it asserts from the reference's own
margins() that no squelch threshold crossing is closer than 1e-6 and no tail count closer than 1e-3 to an integer, and that the stages
that ran and the squelches' close / open cycles are those of the table below (what tools/vet_stage_walks.py found without a GPU).

Three families: plain walks; walks fed one DSP block per call from fixed device buffers with graph replay and the meters on; walks with
_apply's wide menu (the AGC's time constants, RXASetNC drawn up to 16384) and two calls of 70 - 90 blocks.  RXASetNC is capped at 4096 in
all of them: it reaches the equalizer and the FM squelch (RXA.c:941-942), which the engine runs up to 4096 taps.  A minimum-phase
equalizer takes the taps the engine uploaded (rxa_chain_ref.take_mp_taps); the minimum-phase FM squelch filter comes from the library's
host design unit.  Channel 3 alone draws the FM squelch's setters, while it is in FM, and the squelch is switched off ahead of a mode
change out of FM (the engine refuses it while the detector is off).

Inputs that make the squelches work within a walk's 0.7 s: a tone hopping between 400 and 1800 Hz for 0.15 s, a steady 1100 Hz tone for
0.2 s, in turn (rxa_ssql_ref.syllabic: SSB as it is, AM as the envelope); an FM carrier keyed 0.3 s high / 0.22 s low
(rxa_chain_ref.keyed_fm_over_a_floor, which says why not off / on).  Channel 3 enters FM with its filters primed, 12 blocks or more into
the walk, as in test_gpu_rxa_fuzz.py's FM walks (the pull-in from rounding-sized samples is no one's to compare).

VETTED (tools/vet_stage_walks.py, which needs no GPU and prints REJECTED, TABLE and SHARES below in the form they have here).  A seed is
replaced when a margin fails or when a channel's twin distance -- the reference against itself fed 1e-13 relative noise -- exceeds a
tenth of that channel's tolerance.  46 seeds tried, 8 replaced (REJECTED says why: seven on a margin, most often SSQL's trigger voltage
within 1e-6 of its threshold on the FM channel, one on its twin); 38 walks left: 24 plain, 8 replayed, 6 wide.  Before the inputs were
narrowed 31 of 38 failed: an FM carrier keyed fully off leaves the detector's loop on noise alone (twin distances of 1e-4 .. 0.9 on
channel 3), and FM entered on the first block starts the loop on rounding-sized samples; hence the carrier over a floor and FM entered
with primed filters.  Over the 38 walks (SHARES): the FM squelch ran in 29, the equalizer in 36, the carrier block in 37, a peak filter
in 38, SSQL in 36; SSQL went through a close-and-open while running in 12, the FM squelch in 14; two or more of the new stages were
live on one channel at once in all 38.

Largest relative RMS seen on the MI355X: 1.5e-8 in the 1e-6 class (seed 1014, channel 2), 1.7e-5 in the 1e-4 class (seed 3004, channel
0); no walk produced a long minimum-phase channel (RXASetNC is capped at 4096 here and RXASetMP 1 never met it).  No walk needed an
engine or restatement change to pass.
"""
import os

import numpy as np
import pytest
import torch          # before libquiskhip: one HIP runtime per process (torch's), as in bench.py

from conftest import rel_rms
from quisk_amd import synth
from rxa_chain_ref import STAGES, RxaChainRef, keyed_fm_over_a_floor
from rxa_ssql_ref import syllabic
from test_gpu_rxa_fuzz import _apply, _apply2

pytestmark = pytest.mark.gpu

NCH = 4
FS = 192000
FM = 5
MODES = (1, 6, 0, 1)                # channel 3: FM from FM_AFTER blocks on
FM_AFTER = 12
PASSBANDS = ((300.0, 3000.0), (-4000.0, 4000.0), (-3000.0, -300.0), (-8000.0, 8000.0))

# seeds tried, in order, per family; REJECTED: the ones the vetting replaced and why
TRIED = {"plain": list(range(1001, 1027)), "replay": list(range(2001, 2014)), "wide": list(range(3001, 3008))}
REJECTED = {
    1001: 'channel 3 margins ssql_window 7.0e-07, ssql_trigger 7.4e-06, ssql_crossings 7.4e-03',
    1010: 'channel 3 margins fmsq_cross 1.5e-03, fmsq_tail 3.6e-01, ssql_window 3.6e-05, ssql_trigger 5.5e-07, ssql_crossings 4.5e-03',
    2005: 'channel 3 margins ssql_window 6.4e-05, ssql_trigger 5.6e-07, ssql_crossings 4.5e-03',
    2006: 'channel 0 margins ssql_window 1.2e-04, ssql_trigger 5.7e-05, ssql_crossings 1.6e-36',
    2007: 'channel 3 margins fmsq_cross 3.0e-03, fmsq_tail 5.8e-02, ssql_window 1.2e-04, ssql_trigger 7.7e-07, ssql_crossings 9.0e-02',
    2008: 'channel 3 twin 2.0e-05 against tolerance 1e-04',
    2012: 'channel 3 margins fmsq_cross 2.3e-03, fmsq_tail 0.0e+00, ssql_window 9.9e-05, ssql_trigger 1.6e-05, ssql_crossings 1.9e-04',
    3001: 'channel 3 margins fmsq_cross 3.0e-03, ssql_window 8.1e-07, ssql_trigger 1.2e-06, ssql_crossings 6.3e-03',
}
SEEDS = {f: [s for s in t if s not in REJECTED] for f, t in TRIED.items()}
# per seed: (the new stages that ran on some channel, SSQL close/open cycles per channel, FMSQ cycles on channel 3, channels that had two or
# more new stages live on one block)
TABLE = {
    1002: (('fmsq', 'eqp', 'cbl', 'peaks', 'ssql'), (0, 0, 0, 0), 0, (0, 1, 2, 3)),
    1003: (('eqp', 'cbl', 'peaks', 'ssql'), (0, 0, 0, 0), 0, (2, 3)),
    1004: (('fmsq', 'cbl', 'peaks', 'ssql'), (0, 0, 0, 0), 0, (0, 1, 2, 3)),
    1005: (('fmsq', 'eqp', 'cbl', 'peaks', 'ssql'), (0, 0, 0, 0), 0, (1, 2, 3)),
    1006: (('fmsq', 'eqp', 'cbl', 'peaks', 'ssql'), (0, 0, 0, 0), 0, (0, 1, 2, 3)),
    1007: (('fmsq', 'eqp', 'cbl', 'peaks', 'ssql'), (0, 0, 0, 0), 0, (0, 3)),
    1008: (('fmsq', 'eqp', 'cbl', 'peaks', 'ssql'), (0, 0, 0, 0), 1, (0, 1, 2, 3)),
    1009: (('eqp', 'cbl', 'peaks', 'ssql'), (0, 0, 0, 0), 0, (0, 2)),
    1011: (('fmsq', 'eqp', 'cbl', 'peaks', 'ssql'), (0, 0, 0, 1), 1, (1, 2, 3)),
    1012: (('fmsq', 'eqp', 'cbl', 'peaks', 'ssql'), (0, 0, 0, 0), 1, (0, 1, 2, 3)),
    1013: (('cbl', 'peaks', 'ssql'), (0, 0, 0, 2), 0, (1, 3)),
    1014: (('fmsq', 'eqp', 'cbl', 'peaks', 'ssql'), (0, 0, 0, 1), 0, (0, 1, 2, 3)),
    1015: (('fmsq', 'eqp', 'cbl', 'peaks', 'ssql'), (0, 0, 0, 0), 0, (0, 1, 2, 3)),
    1016: (('fmsq', 'eqp', 'cbl', 'peaks', 'ssql'), (0, 0, 0, 0), 1, (0, 1, 2, 3)),
    1017: (('eqp', 'cbl', 'peaks', 'ssql'), (0, 0, 0, 0), 0, (0, 2, 3)),
    1018: (('fmsq', 'eqp', 'cbl', 'peaks', 'ssql'), (0, 0, 0, 0), 0, (0, 1, 2, 3)),
    1019: (('eqp', 'cbl', 'peaks', 'ssql'), (0, 0, 0, 0), 0, (0, 1, 2, 3)),
    1020: (('fmsq', 'eqp', 'cbl', 'peaks', 'ssql'), (2, 0, 0, 0), 1, (0, 1, 3)),
    1021: (('fmsq', 'eqp', 'cbl', 'peaks', 'ssql'), (0, 0, 0, 0), 1, (0, 1, 2, 3)),
    1022: (('fmsq', 'eqp', 'cbl', 'peaks', 'ssql'), (0, 0, 0, 0), 1, (2, 3)),
    1023: (('fmsq', 'eqp', 'cbl', 'peaks', 'ssql'), (0, 0, 0, 0), 0, (0, 1, 2, 3)),
    1024: (('eqp', 'cbl', 'peaks'), (0, 0, 0, 0), 0, (0, 2, 3)),
    1025: (('fmsq', 'eqp', 'cbl', 'peaks', 'ssql'), (1, 0, 0, 0), 1, (0, 1, 2, 3)),
    1026: (('fmsq', 'eqp', 'cbl', 'peaks', 'ssql'), (0, 0, 0, 0), 0, (0, 1, 2, 3)),
    2001: (('eqp', 'peaks', 'ssql'), (0, 0, 0, 1), 0, (2, 3)),
    2002: (('fmsq', 'eqp', 'cbl', 'peaks', 'ssql'), (0, 0, 0, 1), 1, (0, 2, 3)),
    2003: (('fmsq', 'eqp', 'cbl', 'peaks', 'ssql'), (0, 0, 0, 0), 0, (0, 1, 2, 3)),
    2004: (('fmsq', 'eqp', 'cbl', 'peaks', 'ssql'), (0, 0, 0, 1), 0, (0, 1, 3)),
    2009: (('fmsq', 'eqp', 'cbl', 'peaks', 'ssql'), (0, 0, 0, 0), 1, (2, 3)),
    2010: (('fmsq', 'eqp', 'cbl', 'peaks'), (0, 0, 0, 0), 0, (2, 3)),
    2011: (('fmsq', 'eqp', 'cbl', 'peaks', 'ssql'), (0, 0, 0, 0), 0, (0, 1, 3)),
    2013: (('fmsq', 'eqp', 'cbl', 'peaks', 'ssql'), (0, 0, 0, 0), 1, (0, 1, 2, 3)),
    3002: (('fmsq', 'eqp', 'cbl', 'peaks', 'ssql'), (1, 0, 0, 0), 1, (0, 1, 3)),
    3003: (('fmsq', 'eqp', 'cbl', 'peaks', 'ssql'), (0, 0, 0, 0), 1, (0, 1, 3)),
    3004: (('fmsq', 'eqp', 'cbl', 'peaks', 'ssql'), (1, 0, 0, 1), 1, (0, 1, 2, 3)),
    3005: (('eqp', 'cbl', 'peaks', 'ssql'), (1, 1, 1, 0), 0, (0, 1, 2, 3)),
    3006: (('eqp', 'cbl', 'peaks', 'ssql'), (0, 0, 1, 0), 0, (1, 3)),
    3007: (('fmsq', 'eqp', 'cbl', 'peaks', 'ssql'), (0, 0, 0, 0), 0, (0, 1, 2, 3)),
}
# over the committed seeds: walks in which each stage ran, in which a squelch went through a close-and-open while it ran, and in which two
# or more new stages were live on one channel at once
SHARES = {'fmsq': 29, 'eqp': 36, 'cbl': 37, 'peaks': 38, 'ssql': 36, 'ssql_cycle': 12, 'fmsq_cycle': 14, 'two_live': 38, 'walks': 38, 'tried': 46, 'replaced': 8}


def _apply3(rng, targets, fm):
    """one setter (or a pair) of the stages the first two menus leave out; fm: the channel is channel 3 and in FM now"""
    k = int(rng.integers(0, 20 if fm else 15))
    done = []

    def call(name, *args):
        done.append((name,) + args)
        for t, lead in targets:
            getattr(t, name)(*lead, *args)

    def on():
        return int(rng.random() < 0.7)
    if k == 0:
        call("SetRXAEQRun", on())
    elif k == 1:
        call("SetRXAEQNC", int(rng.choice([256, 512, 1024, 2048, 4096])))
    elif k == 2:
        call("SetRXAEQMP", int(rng.integers(0, 2)))
    elif k == 3:                    # distinct frequencies: the engine refuses ties with a stated reason (the reference's qsort leaves their order open)
        nf = int(rng.integers(2, 7))
        F = [0.0] + sorted(float(f) for f in rng.choice(np.arange(50, 8000, 50), nf, replace=False))
        G = [float(rng.uniform(-3, 3))] + [float(g) for g in rng.uniform(-12, 12, nf)]
        call("SetRXAEQProfile", nf, F, G)
    elif k == 4:
        call("SetRXAEQCtfmode", int(rng.integers(0, 2))); call("SetRXAEQWintype", int(rng.integers(0, 2)))
    elif k == 5:
        call("SetRXAGrphEQ", [int(v) for v in rng.integers(-12, 13, 4)])
    elif k == 6:
        call("SetRXAGrphEQ10", [int(v) for v in rng.integers(-12, 13, 11)])
    elif k == 7:
        call("SetRXACBLRun", on())
    elif k == 8:
        call("SetRXASPCWRun", on())
    elif k == 9:
        which = int(rng.integers(0, 3))
        if which == 0: call("SetRXASPCWFreq", float(rng.uniform(300, 2500)))
        elif which == 1: call("SetRXASPCWBandwidth", float(rng.uniform(50, 400)))
        else: call("SetRXASPCWGain", float(rng.uniform(0.5, 3.0)))
    elif k == 10:
        call("SetRXAmpeakRun", on())
    elif k == 11:
        if rng.integers(0, 2): call("SetRXAmpeakNpeaks", int(rng.integers(1, 3)))
        else: call("SetRXAmpeakFilEnable", int(rng.integers(0, 2)), int(rng.integers(0, 2)))
    elif k == 12:
        which, fil = int(rng.integers(0, 3)), int(rng.integers(0, 2))
        if which == 0: call("SetRXAmpeakFilFreq", fil, float(rng.uniform(300, 2500)))
        elif which == 1: call("SetRXAmpeakFilBw", fil, float(rng.uniform(50, 400)))
        else: call("SetRXAmpeakFilGain", fil, float(rng.uniform(0.5, 3.0)))
    elif k == 13:
        call("SetRXASSQLRun", on())
    elif k == 14:
        which = int(rng.integers(0, 3))
        if which == 0: call("SetRXASSQLThreshold", float(rng.uniform(0.10, 0.30)))
        elif which == 1: call("SetRXASSQLTauMute", float(rng.uniform(0.02, 0.15)))
        else: call("SetRXASSQLTauUnMute", float(rng.uniform(0.02, 0.15)))
    elif k <= 16:
        call("SetRXAFMSQRun", on())
    elif k == 17:
        call("SetRXAFMSQThreshold", float(rng.uniform(0.5, 1.0)))
    elif k == 18:
        call("SetRXAFMSQNC", int(rng.choice([256, 1024, 2048, 4096])))
    else:
        call("SetRXAFMSQMP", int(rng.integers(0, 2)))
    return done


class _Guard:
    """the target with the walks' three rules: RXASetNC capped at 4096; on channel 3 no SetRXAAMDRun (the engine refuses the AM detector
    forced on beside the FM one) and SetRXAFMSQRun 0 ahead of a mode change out of FM.  Keeps the channel's mode in `mode` (a list of one)."""

    def __init__(self, t, lead, ch3, mode):
        self._t, self._lead, self._ch3, self._mode = t, lead, ch3, mode

    def __getattr__(self, name):
        f = getattr(self._t, name)
        if name == "RXASetNC":
            return lambda *a: f(*a[:-1], min(a[-1], 4096))
        if self._ch3 and name == "SetRXAAMDRun":
            return lambda *a: None
        if name == "SetRXAMode":
            def call(*a):
                if self._ch3 and a[-1] != FM:
                    self._t.SetRXAFMSQRun(*self._lead, 0)
                self._mode[0] = a[-1]
                f(*a)
            return call
        return f


def make_input(nblk):
    n = nblk * 1024
    t = np.arange(n) / FS
    x = np.empty((NCH, n), dtype=np.complex128)
    noise = synth.make_input_numpy(NCH, n)
    for c in range(NCH):
        car = np.exp(-2j * np.pi * ((synth.shift_freq(c) * t) % 1.0))
        if c == 3:
            x[c] = keyed_fm_over_a_floor(n, FS, seed=3) * car
            continue
        z = syllabic(n, FS, seed=70 + c, on=0.15, off=0.2, rest=1100.0)
        x[c] = ((0.1 + 0.05 * z.real) if MODES[c] == 6 else 0.3 * (np.conj(z) if MODES[c] == 1 else z)) * car + 0.02 * noise[c]
    return x


def walk(seed, family, engine=None, twin=False):
    """One walk on the references (and on `engine` when given).  Returns a dict: y (None without an engine), ref, gain [NCH, n] (SSQL's),
    refs, tol [NCH], log, nblk, seglen, twin_dist [NCH] (None unless twin), x."""
    wide, replay = family == "wide", family == "replay"
    rng = np.random.default_rng(seed)
    nseg = 30 if wide else int(rng.integers(30, 46))
    seglen = [int(rng.integers(1, 7)) for _ in range(nseg)]
    if wide:
        for k in rng.choice(nseg, 2, replace=False):
            seglen[int(k)] = int(rng.integers(70, 91))
    nblk = sum(seglen)
    x = make_input(nblk)
    refs = [RxaChainRef() for _ in range(NCH)]
    twins = [RxaChainRef() for _ in range(NCH)] if twin else []
    e = engine
    if replay and e is not None:
        e.set_graph_replay(True)
        e.enable_meters(True)
        dev = torch.device("cuda:0")
        d_in = torch.zeros((NCH, 1024), dtype=torch.complex128, device=dev)
        d_out = torch.zeros((NCH, 256), dtype=torch.complex128, device=dev)
    modes = [[m] for m in MODES]

    def targets(c):
        tg = [(refs[c], ())] + ([(twins[c], ())] if twin else []) + ([(e, (c,))] if e is not None else [])
        return [(_Guard(t, lead, c == 3, modes[c]), lead) for t, lead in tg]
    for c in range(NCH):
        for t, lead in targets(c):
            t.SetRXAShiftRun(*lead, 1); t.SetRXAShiftFreq(*lead, synth.shift_freq(c)); t.RXANBPSetRun(*lead, 1)
            t.SetRXAMode(*lead, MODES[c]); t.RXASetPassband(*lead, *PASSBANDS[c])
            t.SetRXAAGCMode(*lead, (0, 3, 4, 0)[c])
            t.SetRXASSQLTauMute(*lead, 0.05)
        for name in ("SetRXAEQRun", "SetRXACBLRun", "SetRXASPCWRun" if MODES[c] != 6 else "SetRXAmpeakRun", "SetRXASSQLRun"):
            if rng.random() < 0.4:                       # some stages on from the first block: a squelch needs most of a walk for one cycle
                for t, lead in targets(c):
                    getattr(t, name)(*lead, 1)
    fm_start = [rng.random() < 0.6]                      # channel 3 enters FM, with or without its squelch
    ys, rs, gs, tws, log, pos = [], [[] for _ in range(NCH)], [[] for _ in range(NCH)], [[] for _ in range(NCH)], [], 0
    pert = np.random.default_rng(11)
    lms_used, mp_now, nc_now, mp_long, notches = [False] * NCH, [0] * NCH, [2048] * NCH, [False] * NCH, [[0] for _ in range(NCH)]
    for s, n in enumerate(seglen):
        if fm_start and pos >= FM_AFTER:
            for t, lead in targets(3):
                t.SetRXAMode(*lead, FM); t.SetRXAFMSQRun(*lead, int(fm_start[0]))
            log.append((s, 3, [("SetRXAMode", FM), ("SetRXAFMSQRun", int(fm_start[0]))]))
            fm_start = []
        if s:
            for _ in range(int(rng.integers(1, 3))):
                c = int(rng.integers(0, NCH))
                tg = targets(c)
                menu = int(rng.integers(0, 4))
                if menu >= 2:
                    d = _apply3(rng, tg, fm=(c == 3 and modes[c][0] == FM))
                elif menu == 1:
                    d = _apply2(rng, tg, notches[c], fm=(c == 3))
                else:
                    d = _apply(rng, tg, wide)
                    notches[c][0] += sum(1 for q in d if q[0] == "RXANBPAddNotch")
                log.append((s, c, d))
                lms_used[c] = lms_used[c] or any(q[0] in ("SetRXAANFRun", "SetRXAANRRun") and q[1] for q in d)
                for q in d:
                    if q[0] == "RXASetMP": mp_now[c] = q[1]
                    if q[0] == "RXASetNC": nc_now[c] = min(q[1], 4096)
                mp_long[c] = mp_long[c] or bool(mp_now[c] and nc_now[c] >= 4096)
        seg = x[:, pos * 1024:(pos + n) * 1024]
        pos += n
        for b0, b1 in ([(b, b + 1) for b in range(n)] if replay else [(0, n)]):      # engine first: a minimum-phase equalizer takes the engine's taps
            part = np.ascontiguousarray(seg[:, b0 * 1024:b1 * 1024])
            if e is not None:
                if replay:
                    d_in.copy_(torch.from_numpy(part))
                    torch.cuda.synchronize()
                    e.process_ptr(d_in.data_ptr(), 1024, d_out.data_ptr(), 256, 1)
                    e.synchronize()
                    ys.append(d_out.cpu().numpy())
                else:
                    ys.append(e.process_host(part))
            for c in range(NCH):
                if e is not None:
                    refs[c].take_mp_taps(e, c)
                rs[c].append(refs[c].xrxa(part[c]))
                gs[c].append(refs[c].ssql_gain)
                if twin:
                    tws[c].append(twins[c].xrxa(part[c] * (1.0 + 1e-13 * pert.standard_normal(part.shape[1]))))
    ref = np.stack([np.concatenate(r) for r in rs])
    tol = [1e-4 if lms_used[c] else 1e-5 if mp_long[c] else 1e-6 for c in range(NCH)]
    return dict(y=np.concatenate(ys, 1) if ys else None, ref=ref, gain=np.stack([np.concatenate(g) for g in gs]), refs=refs, tol=tol, log=log, nblk=nblk,
                seglen=seglen, x=x, twin_dist=[rel_rms(np.concatenate(tws[c]), ref[c]) if np.abs(ref[c]).max() >= 1e-9 else 0.0 for c in range(NCH)] if twin else None)


def facts(w):
    """what the table holds of a walk: (stages that ran, SSQL cycles per channel, FMSQ cycles of channel 3, channels with >= 2 new stages live at once)"""
    refs = w["refs"]
    return (tuple(s for s in STAGES if any(r.ran[s] for r in refs)), tuple(r.cycles()["ssql"] for r in refs), refs[3].cycles()["fmsq"],
            tuple(c for c, r in enumerate(refs) if r.live_max >= 2))


def _run(qh, seed, family):
    e = qh.RxaEngine(NCH)
    try:
        e.load_emnr_tables()
        w = walk(seed, family, engine=e)
        launches = e.graph_launches() if family == "replay" else None
    finally:
        e.close()
    refs, y, ref = w["refs"], w["y"], w["ref"]
    for c, r in enumerate(refs):                       # the reference's own conditioning first, and that the walk is the vetted one
        assert r.margins_ok(), "seed %d channel %d: margins %r" % (seed, c, r.margins())
    if seed in TABLE:
        assert facts(w) == TABLE[seed], (seed, facts(w), TABLE[seed])
    if launches is not None:
        assert launches > w["nblk"] // 3
    for c in range(NCH):
        assert np.all(np.isfinite(ref[c]))
        muted = w["gain"][c] == 0.0
        assert not np.any(y[c][muted]), "seed %d channel %d: %d samples not 0 under a muted SSQL, first %r" % (seed, c, int(np.sum(y[c][muted] != 0)), np.flatnonzero(y[c][muted] != 0)[:5])
        if np.abs(ref[c]).max() < 1e-9:
            continue
        if np.sqrt(np.mean(np.abs(y[c] - ref[c]) ** 2)) < 1e-12 * max(1.0, np.abs(w["x"][c]).max()):
            continue                     # (muted from the first blocks on: what is left of the start-up, as in _walk)
        err, tol = rel_rms(y[c], ref[c]), w["tol"][c]
        if os.environ.get("QH_REPORT"):
            print("seed %d channel %d: rel rms %.3e, tolerance %.0e, ran %r" % (seed, c, err, tol, refs[c].ran), flush=True)
        if err >= tol:
            per, q0 = [], 0
            for s2, n2 in enumerate(w["seglen"]):
                a, b = q0 * 256, (q0 + n2) * 256
                per.append("%d:%.1e/%.1e" % (s2, np.sqrt(np.mean(np.abs(y[c, a:b] - ref[c, a:b]) ** 2)), np.sqrt(np.mean(np.abs(ref[c, a:b]) ** 2))))
                q0 += n2
            raise AssertionError("seed %d channel %d: rel rms %.3e (tolerance %.0e); setters %r; per segment rms error / rms of the reference %r" %
                                 (seed, c, err, tol, [l for l in w["log"] if l[1] == c], per))


@pytest.mark.parametrize("seed", SEEDS["plain"])
def test_stage_setter_walk(qh, seed):
    _run(qh, seed, "plain")


@pytest.mark.parametrize("seed", SEEDS["replay"])
def test_stage_setter_walk_block_at_a_time_with_graph_replay(qh, seed):
    """one DSP block per call from fixed device buffers, replay and meters on: every new setter must invalidate the captured launches"""
    _run(qh, seed, "replay")


@pytest.mark.parametrize("seed", SEEDS["wide"])
def test_stage_setter_walk_with_long_filters_agc_windows_and_long_calls(qh, seed):
    _run(qh, seed, "wide")


def test_the_committed_seeds_cover_what_the_issue_asks():
    """from the table alone: every stage in a third of the walks, each squelch through a close-and-open in a quarter, two stages live on
    one channel in a third; no more than a quarter of the tried seeds replaced"""
    seeds = [s for f in SEEDS.values() for s in f]
    assert seeds and all(s in TABLE for s in seeds)
    n = len(seeds)
    for st in STAGES:
        assert 3 * sum(st in TABLE[s][0] for s in seeds) >= n, st
    assert 4 * sum(any(TABLE[s][1]) for s in seeds) >= n and 4 * sum(TABLE[s][2] > 0 for s in seeds) >= n
    assert 3 * sum(bool(TABLE[s][3]) for s in seeds) >= n
    assert 4 * len(REJECTED) <= sum(len(t) for t in TRIED.values())
