"""Restatement of WDSP's carrier block, CW audio peak filter and multi-peak filter (xcbl, xspeak design 1, xmpeak) for the tests.

Written from the reference's semantics (wdsp/cblock.c:29-126, wdsp/iir.c:143-555, create_rxa's arguments RXA.c:403-445), not from
the HIP code: the carrier block sample by sample with its 1e-100 flush as written, every biquad of a peak filter through
scipy.signal.lfilter with its state carried from call to call.  One real filter runs on I and on Q alike.
"""
import math

import numpy as np
from scipy.signal import lfilter

TWOPI = 6.2831853071795864        # wdsp/comm.h


def speak_design(f, bw, gain, rate):
    """calc_speak, design 1, nstages 4 (iir.c:180-214): (b, a, fgain, f as stored back)"""
    if f < 200.0:
        f = 200.0
    ratio = bw / f
    bw_parm, A = 5.0, 2.5
    bw_corr = 1.13 * ratio - 0.956 * ratio * ratio
    w0 = TWOPI * f / rate
    sn = math.sin(w0)
    cbw = bw_corr * f
    c = sn * math.sinh(0.5 * math.log((f + 0.5 * cbw * bw_parm) / (f - 0.5 * cbw * bw_parm)) * w0 / sn)
    den = 1.0 + c / A
    a0 = (1.0 + c * A) / den
    a1 = -2.0 * math.cos(w0) / den
    a2 = (1 - c * A) / den
    b1 = -a1
    b2 = -(1 - c / A) / den
    # y0 = a0 x0 + a1 x1 + a2 x2 + b1 y1 + b2 y2  ->  lfilter's b = (a0, a1, a2), a = (1, -b1, -b2)
    return np.array([a0, a1, a2]), np.array([1.0, -b1, -b2]), gain / (A * A) ** 4, f


class Speak:
    """one SPEAK instance (design 1, four stages sharing one biquad); its state per stage and component as lfilter's zi"""

    def __init__(self, rate, f=600.0, bw=100.0, gain=2.0, run=0):
        self.rate, self.f, self.bw, self.gain, self.run = rate, f, bw, gain, run
        self.calc()

    def calc(self):                   # calc_speak ends in flush_speak
        self.b, self.a, self.fgain, self.f = speak_design(self.f, self.bw, self.gain, self.rate)
        self.flush()

    def flush(self):
        self.zi = np.zeros((4, 2, 2))

    def step(self, z):
        """xspeak's loop on a block (complex in, complex out), whatever `run` says"""
        out = []
        for comp, x in enumerate((np.ascontiguousarray(z.real), np.ascontiguousarray(z.imag))):
            x = self.fgain * x
            for n in range(4):
                x, self.zi[n, comp] = lfilter(self.b, self.a, x, zi=self.zi[n, comp])
            out.append(x)
        return out[0] + 1j * out[1]

    def process(self, z):
        return self.step(z) if self.run else z


class Cbl:
    """the carrier block (cblock.c:29-94), tau 0.02 at dsp rate"""

    def __init__(self, rate, tau=0.02, run=0):
        self.mtau = math.exp(-1.0 / (rate * tau))
        self.run = run
        self.flush()

    def flush(self):
        self.prev_in = [0.0, 0.0]
        self.prev_out = [0.0, 0.0]

    def process(self, z):
        if not self.run:
            return z
        out = []
        m = self.mtau
        for comp, x in enumerate((z.real.tolist(), z.imag.tolist())):
            pi, po = self.prev_in[comp], self.prev_out[comp]
            y = [0.0] * len(x)
            for i, v in enumerate(x):
                o = v - pi + m * po
                y[i] = o
                pi = v
                po = 0.0 if abs(o) < 1.0e-100 else o
            self.prev_in[comp], self.prev_out[comp] = pi, po
            out.append(np.array(y))
        return out[0] + 1j * out[1]


class Mpeak:
    """the multi-peak filter (iir.c:367-555): the sum of the enabled peaks among the first npeaks, each its own SPEAK"""

    def __init__(self, rate, run=0):
        self.run, self.npeaks, self.enable = run, 2, [1, 1]
        self.pfil = [Speak(rate, 2125.0, 75.0, 1.0, run=1), Speak(rate, 2295.0, 75.0, 1.0, run=1)]

    def flush(self):
        for p in self.pfil:
            p.flush()

    def process(self, z):
        if not self.run:
            return z
        mix = np.zeros_like(z)
        for i in range(self.npeaks):
            if self.enable[i]:
                mix = mix + self.pfil[i].step(z)
        return mix


class AudioPeakChain:
    """xcbl -> xspeak -> xmpeak of one channel (RXA.c:591-593) with the WDSP setter names (channel argument left out)"""

    def __init__(self, rate):
        self.cbl, self.speak, self.mpeak = Cbl(rate), Speak(rate), Mpeak(rate)

    def SetRXACBLRun(self, run):
        self.cbl.run = run

    def SetRXASPCWRun(self, run):
        self.speak.run = run

    def SetRXASPCWFreq(self, f):
        self.speak.f = f
        self.speak.calc()

    def SetRXASPCWBandwidth(self, bw):
        self.speak.bw = bw
        self.speak.calc()

    def SetRXASPCWGain(self, g):
        self.speak.gain = g
        self.speak.calc()

    def SetRXAmpeakRun(self, run):
        self.mpeak.run = run

    def SetRXAmpeakNpeaks(self, n):
        assert 0 <= n <= 2
        self.mpeak.npeaks = n

    def SetRXAmpeakFilEnable(self, fil, enable):
        self.mpeak.enable[fil] = enable

    def SetRXAmpeakFilFreq(self, fil, f):
        self.mpeak.pfil[fil].f = f
        self.mpeak.pfil[fil].calc()

    def SetRXAmpeakFilBw(self, fil, bw):
        self.mpeak.pfil[fil].bw = bw
        self.mpeak.pfil[fil].calc()

    def SetRXAmpeakFilGain(self, fil, g):
        self.mpeak.pfil[fil].gain = g
        self.mpeak.pfil[fil].calc()

    def flush(self):                  # flush_rxa, RXA.c:553-555
        self.cbl.flush()
        self.speak.flush()
        self.mpeak.flush()

    def process(self, z):
        z = np.asarray(z, dtype=np.complex128)
        return self.mpeak.process(self.speak.process(self.cbl.process(z)))


def panel(z, gain1=4.0, gain2I=1.0, gain2Q=1.0, inselect=3, copy=0):
    """xpanel's 2x2 real matrix (patchpanel.c:55-101), the engine's EpiParam without the fixed AGC gain"""
    gI, gQ = gain1 * gain2I, gain1 * gain2Q
    sI, sQ = float(inselect >> 1), float(inselect & 1)
    re, im = z.real, z.imag
    if copy == 0:
        return gI * sI * re + 1j * (gQ * sQ * im)
    if copy == 1:
        return gI * sI * re + 1j * (gQ * sI * re)
    if copy == 2:
        return gI * sQ * im + 1j * (gQ * sQ * im)
    return gI * sQ * im + 1j * (gQ * sI * re)
