"""Restatement of WDSP's syllabic squelch (xssql) for the tests.

Written from the reference's semantics (wdsp/ssql.c, the carrier block of wdsp/cblock.c:29-94, dbqlp of wdsp/iir.c:829-916, create_rxa's
arguments RXA.c:447-461), not from the HIP code.  Every step that takes a decision is stepped sample by sample as written; the biquad
low-pass goes through scipy.signal.lfilter with its state carried from call to call.  `process` works on one channel's complex block
and returns the squelched block; it also leaves the per-sample gain and trigger of that block in `gain` and `tr`, and what its
decisions were taken on in `wdist` (|lp - wdaverage|, held against wthresh), `trv` (the trigger voltage, held against tr_thresh) and `zc`
(see `margins`).  Every piece of state is carried from call to call, so calls of one DSP block give what one long call gives.
"""
import math

import numpy as np
from scipy.signal import lfilter

PI = 3.1415926535897932           # wdsp/comm.h
TWOPI = 6.2831853071795864
MUTED, INCREASE, UNMUTED, DECREASE = range(4)


def slews(ntup, ntdown, muted_gain=0.0):
    """compute_ssql_slews (ssql.c:110-127): theta accumulates by += delta"""
    cup, cdown = [], []
    delta, theta = PI / ntup, 0.0
    for _ in range(ntup + 1):
        cup.append(muted_gain + (1.0 - muted_gain) * 0.5 * (1.0 - math.cos(theta)))
        theta += delta
    delta, theta = PI / ntdown, 0.0
    for _ in range(ntdown + 1):
        cdown.append(muted_gain + (1.0 - muted_gain) * 0.5 * (1.0 + math.cos(theta)))
        theta += delta
    return cup, cdown


def dbqlp(rate, fc=11.3, Q=1.0):
    """calc_dbqlp (iir.c:829-843) as lfilter's (b, a): y0 = a0 x0 + a1 x1 + a2 x2 + b1 y1 + b2 y2"""
    w0 = TWOPI * fc / rate
    cs = math.cos(w0)
    c = math.sin(w0) / (2.0 * Q)
    den = 1.0 + c
    a0, a1, a2 = 0.5 * (1.0 - cs) / den, (1.0 - cs) / den, 0.5 * (1.0 - cs) / den
    b1, b2 = 2.0 * cs / den, (c - 1.0) / den
    return np.array([a0, a1, a2]), np.array([1.0, -b1, -b2])


class Ssql:
    """one xssql instance as create_rxa makes it (run 0, 70 ms ramps, muted gain 0, taus 0.1, wthresh 0.08, ring 2400, fmax 2000)"""

    def __init__(self, rate, run=0):
        self.rate = int(rate)
        self.run = run
        self.tup = self.tdown = 0.070
        self.muted_gain = 0.0
        self.tau_mute = self.tau_unmute = 0.1
        self.wthresh = 0.08
        self.tr_thresh, self.tr_ss_mute, self.tr_ss_unmute = 0.8197, 1.0, 0.3125
        self.wdtau = 0.5
        self.rsize, self.fmax = 2400, 2000.0
        # calc_ssql (ssql.c:129-154)
        self.mtau = math.exp(-1.0 / (self.rate * 0.02))
        self.div = self.fmax * 2.0 * self.rsize / self.rate
        self.b, self.a = dbqlp(float(self.rate))
        self.wdmult = math.exp(-1.0 / (self.rate * self.wdtau))
        self.wdaverage = 0.0
        self.tr_voltage = self.tr_thresh
        self.mute_mult = 1.0 - math.exp(-1.0 / (self.rate * self.tau_mute))
        self.unmute_mult = 1.0 - math.exp(-1.0 / (self.rate * self.tau_unmute))
        self.ntup = int(self.tup * self.rate)
        self.ntdown = int(self.tdown * self.rate)
        self.cup, self.cdown = slews(self.ntup, self.ntdown, self.muted_gain)
        self.state, self.count = MUTED, 0
        self.flush_parts()
        self.gain = np.zeros(0)
        self.tr = np.zeros(0, dtype=np.int8)
        self.wdist, self.trv, self.zc = np.zeros(0), np.zeros(0), np.inf

    def flush_parts(self):
        """what flush_ssql zeroes (ssql.c:208-220): the blocker, the ftov ring, rcount and inlast, the biquad"""
        self.prev_in = self.prev_out = 0.0
        self.ring = [0] * self.rsize
        self.rptr = 0
        self.rcount = 0
        self.inlast = 0.0
        self.zi = np.zeros(2)

    def flush(self):
        self.flush_parts()

    # the setters (ssql.c:330-370)
    def SetRXASSQLRun(self, run):
        self.run = run

    def SetRXASSQLThreshold(self, threshold):
        self.wthresh = threshold / 2.0

    def SetRXASSQLTauMute(self, tau):
        self.tau_mute = tau
        self.mute_mult = 1.0 - math.exp(-1.0 / (self.rate * tau)) if tau > 0.0 else 1.0

    def SetRXASSQLTauUnMute(self, tau):
        self.tau_unmute = tau
        self.unmute_mult = 1.0 - math.exp(-1.0 / (self.rate * tau)) if tau > 0.0 else 1.0

    # the stages
    def cbl_i(self, x):
        """xcbl on the I component (cblock.c:74-94): the output as written, the kept output flushed below 1e-100"""
        out = np.empty(len(x))
        pin, pout, mtau = self.prev_in, self.prev_out, self.mtau
        for i, v in enumerate(x.tolist()):
            o = v - pin + mtau * pout
            out[i] = o
            pin = v
            pout = 0.0 if abs(o) < 1.0e-100 else o
        self.prev_in, self.prev_out = pin, pout
        return out

    def ftov(self, x):
        """xftov (ssql.c:70-108)"""
        out = np.empty(len(x))
        ring, rptr, rcount, last = self.ring, self.rptr, self.rcount, self.inlast
        # (diagnostics, `margins`: how far the crossings' two tests were from going the other way)
        xs = np.asarray(x, dtype=np.float64)
        prev = np.concatenate([[last], xs[:-1]])
        step, near0 = np.abs(prev - xs), np.minimum(np.abs(prev), np.abs(xs))
        sign = prev * xs < 0.0
        # (a sample that is exactly 0 -- the line's start, a stage ahead that puts out 0.0 -- is no near miss: its product is exactly 0)
        self.zc = min(float(np.min(np.abs(step[sign] - 0.01), initial=np.inf)) / 0.01, float(np.min(near0[(step > 0.01) & (near0 > 0.0)], initial=np.inf)) / 0.01)
        for i, v in enumerate(x.tolist()):
            if ring[rptr] == 1:
                rcount -= 1
                ring[rptr] = 0
            if last * v < 0.0 and abs(last - v) > 0.01:
                ring[rptr] = 1
                rcount += 1
            rptr += 1
            if rptr == self.rsize:
                rptr = 0
            r = rcount / self.div
            out[i] = 1.0 if 1.0 < r else r
            last = v
        self.rptr, self.rcount, self.inlast = rptr, rcount, last
        return out

    def lowpass(self, x):
        y, self.zi = lfilter(self.b, self.a, x, zi=self.zi)
        return y

    def window(self, lp):
        """the window detector (ssql.c:241-250): 0 = unmute, 1 = mute"""
        wd = np.empty(len(lp), dtype=np.int8)
        dist = np.empty(len(lp))
        w, m, om, th = self.wdaverage, self.wdmult, 1.0 - self.wdmult, self.wthresh
        for i, v in enumerate(lp.tolist()):
            w = m * w + om * v
            wd[i] = 0 if (v - w) > th or (w - v) > th else 1
            dist[i] = abs(v - w)
        self.wdaverage = w
        self.wdist = dist
        return wd

    def trigger(self, wd):
        """ssql.c:252-260: 1 = unmuted"""
        tr = np.empty(len(wd), dtype=np.int8)
        trv = np.empty(len(wd))
        v = self.tr_voltage
        for i, d in enumerate(wd.tolist()):
            if d == 0:
                v += (self.tr_ss_unmute - v) * self.unmute_mult
            else:
                v += (self.tr_ss_mute - v) * self.mute_mult
            tr[i] = 0 if v > self.tr_thresh else 1
            trv[i] = v
        self.tr_voltage = v
        self.trv = trv
        return tr

    def machine(self, tr):
        """the state machine (ssql.c:262-296): the gain of every sample"""
        g = np.empty(len(tr))
        state, count = self.state, self.count
        for i, t in enumerate(tr.tolist()):
            if state == MUTED:
                if t == 1:
                    state, count = INCREASE, self.ntup
                g[i] = self.muted_gain
            elif state == INCREASE:
                g[i] = self.cup[self.ntup - count]
                if count == 0:
                    state = UNMUTED
                count -= 1
            elif state == UNMUTED:
                if t == 0:
                    state, count = DECREASE, self.ntdown
                g[i] = 1.0
            else:
                g[i] = self.cdown[self.ntdown - count]
                if count == 0:
                    state = MUTED
                count -= 1
        self.state, self.count = state, count
        return g

    def process(self, z):
        z = np.asarray(z, dtype=np.complex128)
        if not self.run:
            self.gain = np.ones(len(z))
            self.tr = np.zeros(0, dtype=np.int8)
            self.wdist, self.trv, self.zc = np.zeros(0), np.zeros(0), np.inf
            return z.copy()
        i = self.cbl_i(np.ascontiguousarray(z.real))
        lp = self.lowpass(self.ftov(i))
        self.tr = self.trigger(self.window(lp))
        self.gain = self.machine(self.tr)
        g = self.gain
        out = np.empty_like(z)
        # out = muted_gain * in / in * cup / in (UNMUTED: as is) / in * cdown: products of reals, as the reference's
        out.real = z.real * g
        out.imag = z.imag * g
        return out


def crossing_margin(v, th):
    """the smallest relative distance from th of the samples on both sides of any crossing of it (inf where v never crosses)"""
    v = np.asarray(v)
    below = v < th
    x = np.flatnonzero(below[1:] != below[:-1])
    if not x.size:
        return np.inf
    return min(float(np.min(np.abs(v[x] - th))), float(np.min(np.abs(v[x + 1] - th)))) / th


def edges(gain):
    """(opens, closes): the ramps up and down that start within `gain` (a ramp start is a sample after a muted / unit one)"""
    g = np.asarray(gain)
    muted, unity = g == 0.0, g == 1.0
    opens = int(np.sum(muted[:-1] & ~muted[1:]))
    closes = int(np.sum(unity[:-1] & ~unity[1:]))
    return opens, closes


def syllabic(n, rate, seed=0, amp=0.3, on=1.0, off=1.5, lo=400.0, hi=1800.0, rest=None):
    """a tone hopping between about lo and hi Hz every 60-150 ms, with a little noise, gated on for `on` s and off (zero) for `off` s
    in turn (complex, at baseband).  rest: a steady tone of that frequency through the off periods instead of nothing -- with silence the
    window detector's average (tau 0.5 s, ssql.c:129-154) takes most of a second to come down to the silence and let the squelch close;
    a steady tone near the hops' mean frequency is within the window at once, and the squelch closes after tau_mute"""
    rng = np.random.default_rng(seed)
    f = np.empty(n)
    i = 0
    while i < n:
        seg = int(rng.uniform(0.060, 0.150) * rate)
        f[i:i + seg] = rng.uniform(lo, lo + 200.0) if rng.random() < 0.5 else rng.uniform(hi - 200.0, hi)
        i += seg
    ph = 2.0 * np.pi * np.cumsum(f) / rate
    t = np.arange(n) / rate
    gate = (t % (on + off)) < on
    z = (amp * np.exp(1j * ph) + 0.001 * (rng.standard_normal(n) + 1j * rng.standard_normal(n))) * gate
    if rest is not None:
        z = z + amp * np.exp(2j * np.pi * ((rest * t) % 1.0)) * ~gate
    return z
