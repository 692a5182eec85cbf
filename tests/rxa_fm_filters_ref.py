"""A reference for an RXA channel whose FM detector runs other de-emphasis / audio filters than create_rxa's (SetRXAFMAFFilter,
SetRXAFMNCde / MPde / NCaud / MPaud, wdsp/fmd.c:278-384).  The oracle's xfmd has the default pair built in, so the reference is a
composition: the oracle channel runs with a stage hook at HOOK_FMSQ, where `buf` is midbuff right behind xfmd and `aux` is xfmd's audio
ahead of the de-emphasis filter (oracle/wdsp_oracle.h), and the hook REPLACES buf for an FM channel by the restated tail of xfmd
(fmd.c:173-178):

    aux -> pde (pyoracle.Fircore, the de-emphasis impulse) -> paud (pyoracle.Fircore, the audio impulse) -> xsnotch (restated, iir.c:76-95)

The detector's limiter (fmd.c:179-184) sits behind that tail; these tests leave it off.  Where the FM squelch runs too it is applied
behind the replacement, as RxaChainRef applies it.

The impulses: pyoracle.fir_bandpass for the audio filter (fmd.c:116), a restatement of fc_impulse (fcurve.c:29-146, even nc) for the
de-emphasis filter at the arguments fmd.c:112 passes, and for minimum phase the library's own taps (mp_imp's result hangs on the rounding
of the FFT that made it: rxa_chain_ref.library_mp_taps says why).

State, as the reference keeps it (firmin.c:449-467): SetRXAFMAFFilter and the MP setters design again and KEEP the delay lines
(setImpulse_fircore / setMp_fircore), an NC setter zeroes the line of its own filter only (setNc_fircore); every setter is a no-op on an
equal value.  pyoracle.Fircore has no setImpulse, so a kept line is a fresh fircore fed the filter's last nc input samples again -- the
delay line of a fircore is a function of its last nc inputs and nothing else.

tests/test_fm_filters_ref.py pins all of it on the CPU: with the six defaults the replaced buf is the oracle's own.
"""
import ctypes as C
import functools
import os
import shutil
import subprocess
import tempfile

import numpy as np

from oracle import pyoracle
from rxa_chain_ref import RxaChainRef
from wdsp_fmsq_ref import fir_fsamp

TWOPI = 6.2831853071795864
FM = 5                  # the RXA mode number (RXA.h: LSB 0 ... FM 5)
_DESIGN = None


def fc_impulse(nc, f0, f1, g0, g1, curve, samplerate, scale, ctfmode, wintype):
    """fcurve.c:29-146 for even nc (the branch every power-of-two nc takes; the odd one needs fir_fsamp_odd)"""
    assert nc % 2 == 0
    mid = nc // 2
    A = [0.0] * (mid + 1)
    g0_lin = 10.0 ** (g0 / 20.0)
    for i in range(mid):
        fn = (i + 0.5) / mid
        f = fn * samplerate / 2.0
        if curve == 0:
            A[i] = scale * (g0_lin * f / f0) if f0 > 0.0 else 0.0
        else:
            A[i] = scale * (g0_lin * f0 / f) if f > 0.0 else 0.0
    if ctfmode == 0:
        low = int(2.0 * f0 / samplerate * mid - 0.5)
        high = int(2.0 * f1 / samplerate * mid - 0.5)
        lowmag, highmag = A[low], A[high]
        flow4 = (low / mid) ** 4.0
        fhigh4 = (high / mid) ** 4.0
        k = low
        while k - 1 >= 0:
            k -= 1
            f = k / mid
            lowmag *= (f * f * f * f) / flow4
            if lowmag < 1.0e-100:
                lowmag = 1.0e-100
            A[k] = lowmag
        k = high
        while k + 1 < mid:
            k += 1
            f = k / mid
            highmag *= fhigh4 / (f * f * f * f)
            if highmag < 1.0e-100:
                highmag = 1.0e-100
            A[k] = highmag
    return fir_fsamp(nc, np.array(A), 1.0, wintype).astype(np.complex128)


@functools.lru_cache(maxsize=None)
def de_impulse(nc, f_low, f_high, rate, size):
    """the de-emphasis impulse of create_fmd (fmd.c:112); kept per design: the frequency-sampling sum is nc^2 / 4 cosines"""
    return fc_impulse(nc, f_low, f_high, +20.0 * np.log10(f_high / f_low), 0.0, 1, float(rate), 1.0 / (2.0 * size), 0, 0)


def aud_impulse(nc, f_low, f_high, rate, size, afgain=0.5):
    """the audio filter's impulse of create_fmd (fmd.c:116; afgain: RXA.c:205)"""
    return pyoracle.fir_bandpass(nc, 0.8 * f_low, 1.1 * f_high, float(rate), 0, 1, afgain / (2.0 * size))


def design_lib():
    """qh::fc_impulse, and qh::mp_imp of the two FM designs, from the library's host design unit (compiled once per process)"""
    global _DESIGN
    if _DESIGN is None:
        assert shutil.which("g++"), "the library's designs compile quisk_amd/csrc/qh_design.cpp"
        csrc = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "quisk_amd", "csrc")
        tmp = tempfile.mkdtemp(prefix="rxa_fm_filters_ref_")
        with open(os.path.join(tmp, "shim.cpp"), "w") as f:
            f.write('''
#include <cmath>
#include <cstring>
#include "qh_design.hpp"
extern "C" void t_fc_impulse(int nc, double f0, double f1, double g0, double g1, int curve, double fs, double scale, int ctfmode, int wintype, double *out)
{ auto h = qh::fc_impulse(nc, f0, f1, g0, g1, curve, fs, scale, ctfmode, wintype); std::memcpy(out, h.data(), h.size() * 16); }
extern "C" void t_fm_de_mp(int nc, double lo, double hi, double fs, double scale, double *out)
{ auto h = qh::mp_imp(qh::fc_impulse(nc, lo, hi, +20.0 * std::log10(hi / lo), 0.0, 1, fs, scale, 0, 0), 16, 0); std::memcpy(out, h.data(), h.size() * 16); }
extern "C" void t_fm_aud_mp(int nc, double lo, double hi, double fs, double scale, double *out)
{ auto h = qh::mp_imp(qh::fir_bandpass(nc, 0.8 * lo, 1.1 * hi, fs, 0, 1, scale), 16, 0); std::memcpy(out, h.data(), h.size() * 16); }
''')
        so = os.path.join(tmp, "libfmfiltersrefdesign.so")
        subprocess.run(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-I", csrc, os.path.join(tmp, "shim.cpp"), os.path.join(csrc, "qh_design.cpp"),
                        "-o", so], check=True)
        _DESIGN = C.CDLL(so)
    return _DESIGN


def library_fc_impulse(nc, f0, f1, g0, g1, curve, rate, scale, ctfmode, wintype):
    out = np.zeros(nc, dtype=np.complex128)
    design_lib().t_fc_impulse(C.c_int(nc), C.c_double(f0), C.c_double(f1), C.c_double(g0), C.c_double(g1), C.c_int(curve), C.c_double(rate),
                              C.c_double(scale), C.c_int(ctfmode), C.c_int(wintype), out.ctypes.data_as(C.c_void_p))
    return out


def library_mp_taps(which, nc, f_low, f_high, rate, size, afgain=0.5):
    """the minimum-phase taps the library designs for the de-emphasis ("de") or the audio ("aud") filter, at the scale fircore gets"""
    out = np.zeros(nc, dtype=np.complex128)
    fn = design_lib().t_fm_de_mp if which == "de" else design_lib().t_fm_aud_mp
    scale = (1.0 if which == "de" else afgain) / (2.0 * size)
    fn(C.c_int(nc), C.c_double(f_low), C.c_double(f_high), C.c_double(rate), C.c_double(scale), out.ctypes.data_as(C.c_void_p))
    return out


class Snotch:
    """create_snotch / calc_snotch / flush_snotch / xsnotch (iir.c:35-95): the real part is filtered, the imaginary part passes"""

    def __init__(self, run, rate, f, bw):
        self.run, self.rate, self.f, self.bw = run, rate, f, bw
        self.calc()

    def calc(self):
        fn = self.f / float(self.rate)
        csn = np.cos(TWOPI * fn)
        qr = 1.0 - 3.0 * self.bw
        qk = (1.0 - 2.0 * qr * csn + qr * qr) / (2.0 * (1.0 - csn))
        self.a0, self.a1, self.a2 = +qk, -2.0 * qk * csn, +qk
        self.b1, self.b2 = +2.0 * qr * csn, -qr * qr
        self.flush()

    def flush(self):
        self.x1 = self.x2 = self.y1 = self.y2 = 0.0

    def process(self, z):
        z = np.array(z, dtype=np.complex128)
        if not self.run:
            return z
        x1, x2, y1, y2 = self.x1, self.x2, self.y1, self.y2
        a0, a1, a2, b1, b2 = self.a0, self.a1, self.a2, self.b1, self.b2
        re = z.real.copy()
        for i in range(re.size):
            x0 = re[i]
            y0 = a0 * x0 + a1 * x1 + a2 * x2 + b1 * y1 + b2 * y2
            re[i] = y0
            y2, y1, x2, x1 = y1, y0, x1, x0
        self.x1, self.x2, self.y1, self.y2 = x1, x2, y1, y2
        z.real = re
        return z


class _Line:
    """one fircore with the last inputs it took, so that a new impulse can keep the delay line"""
    KEEP = 65536

    def __init__(self, size):
        self.size, self.core, self.hist = size, None, np.zeros(0, dtype=np.complex128)

    def set_impulse(self, imp, keep):
        nc = len(imp)
        self.core = pyoracle.Fircore(self.size, nc, imp)
        if not keep:
            self.hist = np.zeros(0, dtype=np.complex128)
            return
        n = min(self.hist.size, nc) // self.size * self.size
        if n:
            self.core(self.hist[self.hist.size - n:])

    def __call__(self, x):
        self.hist = np.concatenate([self.hist, x])[-self.KEEP:]
        return self.core(x)


class FmFilters:
    """the tail of one channel's xfmd (fmd.c:173-178) with its six settings and the CTCSS notch"""

    def __init__(self, rate=48000, size=64, ctcss_run=1, ctcss_freq=254.1):
        self.rate, self.size = rate, size
        self.nc_de = self.nc_aud = max(2048, size)                      # RXA.c:209,211
        self.mp_de = self.mp_aud = 0
        self.f_low, self.f_high = 300.0, 3000.0                         # RXA.c:196-197
        self.de, self.aud = _Line(size), _Line(size)
        self.sntch = Snotch(ctcss_run, rate, ctcss_freq, 0.0002)        # fmd.c:47
        self._design("de", False)
        self._design("aud", False)

    def _design(self, which, keep):
        nc, mp = (self.nc_de, self.mp_de) if which == "de" else (self.nc_aud, self.mp_aud)
        if mp:
            imp = library_mp_taps(which, nc, self.f_low, self.f_high, self.rate, self.size)
        elif which == "de":
            imp = de_impulse(nc, self.f_low, self.f_high, self.rate, self.size)
        else:
            imp = aud_impulse(nc, self.f_low, self.f_high, self.rate, self.size)
        (self.de if which == "de" else self.aud).set_impulse(imp, keep)

    def SetRXAFMAFFilter(self, low, high):                              # fmd.c:364-384
        if (low, high) != (self.f_low, self.f_high):
            self.f_low, self.f_high = float(low), float(high)
            self._design("de", True)
            self._design("aud", True)

    def SetRXAFMNCde(self, nc):                                         # fmd.c:278-293
        if nc != self.nc_de:
            self.nc_de = nc
            self._design("de", False)

    def SetRXAFMMPde(self, mp):                                         # fmd.c:295-305
        if mp != self.mp_de:
            self.mp_de = mp
            self._design("de", True)

    def SetRXAFMNCaud(self, nc):                                        # fmd.c:307-322
        if nc != self.nc_aud:
            self.nc_aud = nc
            self._design("aud", False)

    def SetRXAFMMPaud(self, mp):                                        # fmd.c:324-334
        if mp != self.mp_aud:
            self.mp_aud = mp
            self._design("aud", True)

    def SetRXACTCSSRun(self, run):                                      # fmd.c:260-267
        self.sntch.run = run

    def SetRXACTCSSFreq(self, freq):                                    # fmd.c:248-258: calc_snotch ends with flush_snotch
        self.sntch.f = freq
        self.sntch.calc()

    def new_rate(self, rate):
        """setSamplerate_fmd (fmd.c:201-216): new impulses, the lines kept; calc_snotch flushes the notch"""
        self.rate = rate
        self._design("de", True)
        self._design("aud", True)
        self.sntch.rate = rate
        self.sntch.calc()

    def new_size(self, size):
        """setSize_fmd (fmd.c:218-237): the fircores are made anew; the notch keeps its state"""
        self.size = size
        self.de, self.aud = _Line(size), _Line(size)
        self._design("de", False)
        self._design("aud", False)

    def process(self, aux):
        a = np.asarray(aux, dtype=np.float64)
        x = a + 1j * a                                                  # fmd.c:170-171
        return self.sntch.process(self.aud(self.de(x)))


class RxaFmRef(RxaChainRef):
    """RxaChainRef with the FM detector's filter tail replaced at HOOK_FMSQ while the channel is in FM"""

    def __init__(self, in_size=64, dsp_size=64, in_rate=48000, dsp_rate=48000, out_rate=48000):
        super().__init__(in_size, dsp_size, in_rate, dsp_rate, out_rate, hooks=True)
        self.fm = FmFilters(dsp_rate, dsp_size)
        self.mode = 0

    def SetRXAMode(self, mode):
        self.mode = mode
        self.o.SetRXAMode(mode)

    def SetRXAFMAFFilter(self, low, high): self.fm.SetRXAFMAFFilter(low, high)
    def SetRXAFMNCde(self, nc): self.fm.SetRXAFMNCde(nc)
    def SetRXAFMMPde(self, mp): self.fm.SetRXAFMMPde(mp)
    def SetRXAFMNCaud(self, nc): self.fm.SetRXAFMNCaud(nc)
    def SetRXAFMMPaud(self, mp): self.fm.SetRXAFMMPaud(mp)

    def SetRXACTCSSRun(self, run):
        self.fm.SetRXACTCSSRun(run)
        self.o.SetRXACTCSSRun(run)

    def SetRXACTCSSFreq(self, freq):
        self.fm.SetRXACTCSSFreq(freq)
        self.o.SetRXACTCSSFreq(freq)

    def RXASetNC(self, nc):                                             # RXA.c:943-944
        super().RXASetNC(nc)
        self.fm.SetRXAFMNCde(nc)
        self.fm.SetRXAFMNCaud(nc)

    def RXASetMP(self, mp):                                             # RXA.c:956-957
        super().RXASetMP(mp)
        self.fm.SetRXAFMMPde(mp)
        self.fm.SetRXAFMMPaud(mp)

    def _hook(self, where, z, aux):
        if where == pyoracle.WdspChannel.HOOK_FMSQ and self.mode == FM:
            z[:] = self.fm.process(aux)
        super()._hook(where, z, aux)


def fm_tone(n, rate, carrier=0.0, tone=1000.0, dev=3000.0, amp=0.3, seed=None, sigma=0.0):
    """an FM signal: a tone at the given deviation on a carrier at `carrier` Hz, noise of sigma per component when asked for"""
    t = np.arange(n) / float(rate)
    ph = TWOPI * np.cumsum(dev * np.sin(TWOPI * tone * t)) / rate + TWOPI * carrier * t
    x = amp * np.exp(1j * ph)
    if sigma:
        r = np.random.default_rng(seed)
        x = x + sigma * (r.standard_normal(n) + 1j * r.standard_normal(n))
    return x


# the audio bands and the (low, high, nc, rate) designs of the GPU tests (tests/test_gpu_rxa_fm_filters.py and its two companions)
BAND_A, BAND_B = (300.0, 3000.0), (200.0, 5000.0)
GPU_DESIGNS = [(lo, hi, nc, rate) for (lo, hi) in (BAND_A, BAND_B) for nc in (256, 512, 1024, 2048, 4096, 8192) for rate in (48000, 96000)]
