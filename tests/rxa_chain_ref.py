"""A whole-chain reference of xrxa (RXA.c:561-598) with every stage the engine has: the oracle's channel (oracle/wdsp_oracle.c) with the
restatements the stage tests pin on the CPU hooked in at the call sites the oracle leaves out,

    xfmsq (RXA.c:575)                    wdsp_fmsq_ref.Fmsq, its trigger the oracle xfmd's own audio buffer (RXA.c:220)
    xeqp (RXA.c:579)                     wdsp_eqp_ref.Eqp
    xcbl, xspeak, xmpeak (RXA.c:591-593) rxa_audio_peak_ref.AudioPeakChain
    xssql (RXA.c:594)                    rxa_ssql_ref.Ssql

one DSP block at a time.  `RxaChainRef` takes every WDSP setter under its WDSP name (the channel argument left out) and sends it where
the reference sends it: RXASetNC and RXASetMP reach the oracle's filters and the equalizer's and the FM squelch's too (RXA.c:934-958).

Minimum phase: mp_imp of an eq_impulse design is decided by the rounding of whichever FFT made it (wdsp_eqp_ref.Eqp, wdsp_fmsq_ref.Fmsq say
why), so such a design comes from the library: `library_mp_taps` compiles the library's host design unit (quisk_amd/csrc/qh_design.cpp, as
tests/test_gpu_rxa_fmsq.py does) and `take_mp_taps` takes the taps an engine uploaded (qh_rxa_debug_eqp).  tests/test_design_eqp_host.py
bounds the design itself.

What the squelch restatements know is kept per call and over the run: `ssql_gain` / `fmsq_gain` (per sample of the last xrxa call),
`margins()` (the smallest distance of any threshold decision and tail count from going the other way), `cycles()` (how many times each
squelch closed and opened again while it ran) and `ran` (which of the five stages ever ran on a block).
"""
import ctypes as C
import os
import shutil
import subprocess
import tempfile

import numpy as np

from oracle import pyoracle
from rxa_audio_peak_ref import AudioPeakChain
from rxa_ssql_ref import Ssql, crossing_margin
from wdsp_eqp_ref import Eqp
from wdsp_fmsq_ref import Fmsq
from wdsp_fmsq_ref import margins as fmsq_margins

_EQP = ("SetRXAEQRun", "SetRXAEQNC", "SetRXAEQMP", "SetRXAEQProfile", "SetRXAEQCtfmode", "SetRXAEQWintype", "SetRXAGrphEQ", "SetRXAGrphEQ10")
_FMSQ = ("SetRXAFMSQRun", "SetRXAFMSQThreshold", "SetRXAFMSQNC", "SetRXAFMSQMP")
_PEAK = ("SetRXACBLRun", "SetRXASPCWRun", "SetRXASPCWFreq", "SetRXASPCWBandwidth", "SetRXASPCWGain", "SetRXAmpeakRun", "SetRXAmpeakNpeaks",
         "SetRXAmpeakFilEnable", "SetRXAmpeakFilFreq", "SetRXAmpeakFilBw", "SetRXAmpeakFilGain")
_SSQL = ("SetRXASSQLRun", "SetRXASSQLThreshold", "SetRXASSQLTauMute", "SetRXASSQLTauUnMute")
STAGES = ("fmsq", "eqp", "cbl", "peaks", "ssql")            # peaks: the CW peak filter or the multi-peak filter

_DESIGN = None


def _design_lib():
    """qh::mp_imp of qh::eq_impulse / qh::fmsq_impulse from the library's host design unit, compiled once per process"""
    global _DESIGN
    if _DESIGN is None:
        assert shutil.which("g++"), "a minimum-phase design compiles quisk_amd/csrc/qh_design.cpp"
        csrc = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "quisk_amd", "csrc")
        tmp = tempfile.mkdtemp(prefix="rxa_chain_ref_")
        with open(os.path.join(tmp, "shim.cpp"), "w") as f:
            f.write('''
#include <cstring>
#include "qh_design.hpp"
extern "C" void t_fmsq_mp(int nc, double fs, double scale, double *out)
{ auto h = qh::mp_imp(qh::fmsq_impulse(nc, fs, scale), 16, 0); std::memcpy(out, h.data(), h.size() * 16); }
extern "C" void t_eq_mp(int nc, int nfreqs, const double *F, const double *G, double fs, double scale, int ctfmode, int wintype, double *out)
{ auto h = qh::mp_imp(qh::eq_impulse(nc, nfreqs, F, G, fs, scale, ctfmode, wintype), 16, 0); std::memcpy(out, h.data(), h.size() * 16); }
''')
        so = os.path.join(tmp, "libchainrefdesign.so")
        subprocess.run(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-I", csrc, os.path.join(tmp, "shim.cpp"), os.path.join(csrc, "qh_design.cpp"),
                        "-o", so], check=True)
        _DESIGN = C.CDLL(so)
    return _DESIGN


def library_mp_taps(stage):
    """the minimum-phase taps the library designs for an Eqp or Fmsq as it stands now, scale 1 / (2 size)"""
    out = np.zeros(stage.nc, dtype=np.complex128)
    scale = 1.0 / (2.0 * stage.size)
    if isinstance(stage, Fmsq):
        _design_lib().t_fmsq_mp(C.c_int(stage.nc), C.c_double(stage.rate), C.c_double(scale), out.ctypes.data_as(C.c_void_p))
    else:
        n = stage.nfreqs + 1
        F, G = (C.c_double * n)(*stage.F[:n]), (C.c_double * n)(*stage.G[:n])
        _design_lib().t_eq_mp(C.c_int(stage.nc), C.c_int(stage.nfreqs), F, G, C.c_double(stage.rate), C.c_double(scale), C.c_int(stage.ctfmode),
                              C.c_int(stage.wintype), out.ctypes.data_as(C.c_void_p))
    return out


def keyed_fm_over_a_floor(n, rate, seed=3, lo=0.0045, hi=0.3, sigma=0.003, off=0.22, on=0.3, tone=1000.0, dev=3000.0):
    """wdsp_fmsq_ref.keyed_fm with the carrier keyed between lo and hi instead of off and on.  With no carrier at all the detector's loop
    runs on noise alone and what it puts out is no continuous function of its input; with a carrier of 1.5 times the noise's sigma it
    still is (the reference against itself fed 1e-13 relative noise: 1e-13), and the FM squelch's avnoise there is 1.6, against 0.03 on the
    full carrier and the thresholds' 0.56 / 0.75.  The carrier starts high: the tail is 1.2 s times longnoise (fmsq.c:178-181), which starts
    at 1 and comes down with tau 0.1 s while the carrier is there, so after 0.3 s of carrier the tail is 0.16 s and the squelch closes
    within the low period of 0.22 s; it opens again at 0.52 s."""
    from wdsp_fmsq_ref import keyed_fm
    t = np.arange(n) / rate
    ph = 2.0 * np.pi * np.cumsum(dev * np.sin(2.0 * np.pi * tone * t)) / rate
    return keyed_fm(n, rate, seed=seed, amp=hi - lo, off=off, on=on, tone=tone, dev=dev, sigma=sigma, start_on=True) + lo * np.exp(1j * ph)


def count_cycles(gain):
    """closes followed by an open within one running stretch: a ramp down starts behind a unit sample, a ramp up behind a muted one"""
    g = np.asarray(gain)
    if g.size < 2:
        return 0
    closes = np.flatnonzero((g[:-1] == 1.0) & (g[1:] != 1.0))
    opens = np.flatnonzero((g[:-1] == 0.0) & (g[1:] != 0.0))
    n, at = 0, -1
    for c in closes:
        if c <= at:
            continue
        later = opens[opens > c]
        if not later.size:
            break
        n, at = n + 1, int(later[0])
    return n


class RxaChainRef:
    """one RXA channel with all its stages; hooks=False leaves the oracle as it is without them"""

    def __init__(self, in_size=1024, dsp_size=256, in_rate=192000, dsp_rate=48000, out_rate=48000, hooks=True):
        self.o = pyoracle.WdspChannel(in_size, dsp_size, in_rate, dsp_rate, out_rate)
        self.dsp_insize, self.dsp_outsize, self.dsp_size = self.o.dsp_insize, self.o.dsp_outsize, dsp_size
        self.eqp = Eqp(dsp_rate, size=dsp_size)
        self.fmsq = Fmsq(dsp_rate, size=dsp_size)
        self.peak = AudioPeakChain(dsp_rate)
        self.ssql = Ssql(dsp_rate)
        self.ran = {s: 0 for s in STAGES}                   # blocks on which the stage ran
        self.live_max, self._live = 0, 0                    # the most of the five that ran on one block
        self.ssql_gain, self.fmsq_gain = np.zeros(0), np.zeros(0)
        self._g = {"ssql": [], "fmsq": []}                  # the last call's gains, block by block
        self._runs = {"ssql": [[]], "fmsq": [[]]}           # the gains of every stretch of blocks on which the squelch ran
        self._m = {"fmsq_cross": np.inf, "fmsq_tail": np.inf, "ssql_window": np.inf, "ssql_trigger": np.inf, "ssql_crossings": np.inf}
        self._last = {"av": None, "wdist": None, "trv": None}
        if hooks:
            self.o.set_stage_hook(self._hook)

    # ---- setters
    def __getattr__(self, name):
        if name in _EQP:
            return lambda *a: self._eqp_set(name, *a)
        if name in _FMSQ:
            return lambda *a: self._fmsq_set(name, *a)
        if name in _PEAK:
            return getattr(self.peak, name)
        if name in _SSQL:
            return getattr(self.ssql, name)
        return getattr(self.o, name)

    def _eqp_set(self, name, *a):
        getattr(self.eqp, name)(*a)
        if self.eqp.mp and name != "SetRXAEQRun":
            self.eqp.use_taps(library_mp_taps(self.eqp))

    def _fmsq_set(self, name, *a):
        f = self.fmsq
        if name in ("SetRXAFMSQNC", "SetRXAFMSQMP"):
            nc, mp = (a[0], f.mp) if name == "SetRXAFMSQNC" else (f.nc, a[0])
            if (nc, mp) != (f.nc, f.mp):                    # a minimum-phase case brings its taps (wdsp_fmsq_ref.Fmsq)
                f.taps = None
                if mp:
                    want = Fmsq(f.rate, size=f.size, nc=nc)
                    f.taps = library_mp_taps(want) * (2.0 * f.size)
        getattr(f, name)(*a)

    def RXASetNC(self, nc):                                 # RXA.c:934-946
        self.o.RXASetNC(nc)
        self._eqp_set("SetRXAEQNC", nc)
        self._fmsq_set("SetRXAFMSQNC", nc)

    def RXASetMP(self, mp):                                 # RXA.c:948-958
        self.o.RXASetMP(mp)
        self._eqp_set("SetRXAEQMP", mp)
        self._fmsq_set("SetRXAFMSQMP", mp)

    def take_mp_taps(self, engine, ch):
        """behind the engine's process call, ahead of this reference's: a running minimum-phase equalizer takes the taps the engine
        uploaded for that call, the delay line kept (tests/test_gpu_rxa_eqp.py's take_mp_taps)"""
        if self.eqp.mp and self.eqp.run:
            self.eqp.use_taps(engine.debug_eqp(ch))

    def flush(self):
        raise NotImplementedError("the oracle has no flush_rxa")

    # ---- the chain
    def _note(self, which, gain, running):
        self._g[which].append(gain)
        runs = self._runs[which]
        if running:
            runs[-1].append(gain)
        elif runs[-1]:
            runs.append([])

    def _carry(self, key, v):
        last = self._last[key]
        self._last[key] = v[-1]
        return v if last is None else np.concatenate([[last], v])

    def _hook(self, where, z, aux):
        if where == pyoracle.WdspChannel.HOOK_FMSQ:
            f = self.fmsq
            if f.run:
                z[:] = f.process(aux, z)
                cr, tl = fmsq_margins(self._carry("av", f.av), (f.tail_thresh, f.unmute_thresh), f.tails)
                self._m["fmsq_cross"], self._m["fmsq_tail"] = min(self._m["fmsq_cross"], cr), min(self._m["fmsq_tail"], tl)
                self.ran["fmsq"] += 1
                self._live = 1
                self._note("fmsq", f.gain, True)
            else:
                self._last["av"] = None
                self._live = 0
                self._note("fmsq", np.ones(len(z)), False)
        elif where == pyoracle.WdspChannel.HOOK_EQP:
            if self.eqp.run:
                z[:] = self.eqp.process(z)
                self.ran["eqp"] += 1
                self._live += 1
        else:
            p, s = self.peak, self.ssql
            peaks = bool(p.speak.run or p.mpeak.run)
            if p.cbl.run or peaks:
                z[:] = p.process(z)
            self.ran["cbl"] += bool(p.cbl.run)
            self.ran["peaks"] += peaks
            if s.run:
                z[:] = s.process(z)
                self._m["ssql_window"] = min(self._m["ssql_window"], crossing_margin(self._carry("wdist", s.wdist), s.wthresh))
                self._m["ssql_trigger"] = min(self._m["ssql_trigger"], crossing_margin(self._carry("trv", s.trv), s.tr_thresh))
                self._m["ssql_crossings"] = min(self._m["ssql_crossings"], s.zc)
                self.ran["ssql"] += 1
                self._note("ssql", s.gain, True)
            else:
                self._last["wdist"] = self._last["trv"] = None
                self._note("ssql", np.ones(len(z)), False)
            self.live_max = max(self.live_max, self._live + bool(p.cbl.run) + peaks + bool(s.run))

    def xrxa(self, x):
        """the chain over a whole number of DSP blocks of input"""
        self._g = {"ssql": [], "fmsq": []}
        y = self.o.xrxa(x)
        self.ssql_gain = np.concatenate(self._g["ssql"]) if self._g["ssql"] else np.zeros(0)
        self.fmsq_gain = np.concatenate(self._g["fmsq"]) if self._g["fmsq"] else np.zeros(0)
        return y

    # ---- what the squelches know
    def margins(self):
        """{decision: its smallest margin over the run}: relative distance from the threshold at a crossing (fmsq_cross: avnoise against
        the tail and unmute thresholds; ssql_window: |lp - wdaverage| against wthresh; ssql_trigger: the trigger voltage against
        tr_thresh; ssql_crossings: xftov's |step| against 0.01 at a sign change and the sample nearest 0 of a counted step, over
        0.01), and fmsq_tail: the distance of a tail count's real value from an integer.  inf: no such decision was taken."""
        return dict(self._m)

    def margins_ok(self, cross=1e-6, tail=1e-3):
        m = self._m
        return all(m[k] > cross for k in ("fmsq_cross", "ssql_window", "ssql_trigger", "ssql_crossings")) and m["fmsq_tail"] > tail

    def run_gain(self, which):
        """the gain of "ssql" or "fmsq" over every block on which it ran"""
        g = [b for r in self._runs[which] for b in r]
        return np.concatenate(g) if g else np.zeros(0)

    def cycles(self):
        """{squelch: closes followed by an open, counted inside the stretches on which it ran}"""
        return {k: sum(count_cycles(np.concatenate(r)) for r in runs if r) for k, runs in self._runs.items()}

    def close(self):
        self.o.close()
