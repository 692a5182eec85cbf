"""WDSP's noise blanker (ANB: xanb and its setters, wdsp/nob.c:33-187, 348-422) restated sample by sample in plain Python, for the
tests of qh_anb_* and the EXT names.  Written from the behaviour, quirks included:

  * the delay line is read T = trans_count + adv_count samples behind its write point: output i is input i - T times a scale;
  * avg already holds the current sample when the sample is compared with avg * threshold; a hit loads count with T, the state machine
    looks at count, then count drops by one if positive;
  * htime is set neither on entry to the hang state nor by a reset: it keeps what the last hang left (0 the first time), so the first
    quiet hang lasts hang_count samples longer than the later ones;
  * run = 0 copies the input undelayed and leaves every piece of state, the delay line included, as it is;
  * tau, hangtime, advtime, backtau and samplerate start the blanker over (zeroed delay line); threshold and run do not.

math.cos / math.exp are the C library's, so wave[] and backmult are the numbers the host side of the library computes.

`margin` is the smallest |mag - avg * threshold| / (avg * threshold) seen so far: how far the closest compare sat from flipping."""
import math

import numpy as np

MAX_TAU = 0.002
MAX_ADVTIME = 0.002
MAX_SAMPLERATE = 1536000


class Anb:
    def __init__(self, samplerate, tau, hangtime, advtime, backtau, threshold, run=1):
        self.run = run
        self.samplerate, self.tau, self.hangtime, self.advtime, self.backtau, self.threshold = float(samplerate), tau, hangtime, advtime, backtau, threshold
        self.dline_size = int((MAX_TAU + MAX_ADVTIME) * MAX_SAMPLERATE) + 1
        self.dtime = self.atime = self.htime = self.itime = 0
        self.margin = math.inf
        self.triggers = 0
        self._init()

    def _init(self):
        self.trans_count = max(2, int(self.tau * self.samplerate))
        self.hang_count = int(self.hangtime * self.samplerate)
        self.adv_count = int(self.advtime * self.samplerate)
        self.count = 0
        self.in_idx = self.trans_count + self.adv_count
        self.out_idx = 0
        coef = math.pi / self.trans_count
        self.state = 0
        self.avg = 1.0
        self.power = 1.0
        self.backmult = math.exp(-1.0 / (self.samplerate * self.backtau))
        self.ombackmult = 1.0 - self.backmult
        self.wave = [0.5 * math.cos(i * coef) for i in range(self.trans_count + 1)]
        self.dline = [0j] * self.dline_size

    @property
    def delay(self):
        return self.trans_count + self.adv_count

    # the setters of nob.c:348-422
    def SetRun(self, run):
        self.run = run

    def SetSamplerate(self, rate):
        self.samplerate = float(int(rate))
        self._init()

    def SetTau(self, tau):
        self.tau = tau
        self._init()

    def SetHangtime(self, t):
        self.hangtime = t
        self._init()

    def SetAdvtime(self, t):
        self.advtime = t
        self._init()

    def SetBacktau(self, tau):
        self.backtau = tau
        self._init()

    def SetThreshold(self, thresh):
        self.threshold = thresh

    def flush(self):
        self._init()

    def process(self, x):
        x = np.asarray(x, dtype=np.complex128)
        if not self.run:
            return x.copy()
        n = len(x)
        out = np.zeros(n, dtype=np.complex128)
        re, im = x.real.tolist(), x.imag.tolist()
        T = self.trans_count + self.adv_count
        bm, om, th = self.backmult, self.ombackmult, self.threshold
        wave, dline, size = self.wave, self.dline, self.dline_size
        avg, count, state, power = self.avg, self.count, self.state, self.power
        dtime, atime, htime, itime = self.dtime, self.atime, self.htime, self.itime
        in_idx, out_idx = self.in_idx, self.out_idx
        margin, triggers = self.margin, self.triggers
        sqrt = math.sqrt
        for i in range(n):
            a, b = re[i], im[i]
            mag = sqrt(a * a + b * b)
            avg = bm * avg + om * mag
            dline[in_idx] = x[i]
            lim = avg * th
            if lim > 0.0:
                m = abs(mag - lim) / lim
                if m < margin:
                    margin = m
            if mag > lim:
                count = T
                triggers += 1
            if state == 0:
                out[i] = dline[out_idx]
                if count > 0:
                    state, dtime, power = 1, 0, 1.0
            elif state == 1:
                scale = power * (0.5 + wave[dtime])
                d = dline[out_idx]
                out[i] = complex(d.real * scale, d.imag * scale)
                dtime += 1
                if dtime > self.trans_count:
                    state, atime = 2, 0
            elif state == 2:
                atime += 1
                if atime > self.adv_count:
                    state = 3
            elif state == 3:
                if count > 0:
                    htime = -count
                htime += 1
                if htime > self.hang_count:
                    state, itime = 4, 0
            else:
                scale = 0.5 - wave[itime]
                d = dline[out_idx]
                out[i] = complex(d.real * scale, d.imag * scale)
                if count > 0:
                    state, dtime, power = 1, 0, scale
                else:
                    itime += 1
                    if itime > self.trans_count:
                        state = 0
            if count > 0:
                count -= 1
            in_idx += 1
            if in_idx == size:
                in_idx = 0
            out_idx += 1
            if out_idx == size:
                out_idx = 0
        self.avg, self.count, self.state, self.power = avg, count, state, power
        self.dtime, self.atime, self.htime, self.itime = dtime, atime, htime, itime
        self.in_idx, self.out_idx = in_idx, out_idx
        self.margin, self.triggers = margin, triggers
        return out


def run_cuts(anb, x, cuts):
    """x through `anb` in the calls [cuts[k], cuts[k+1])."""
    parts = [anb.process(x[a:b]) for a, b in zip(cuts[:-1], cuts[1:])]
    return np.concatenate(parts) if parts else np.zeros(0, dtype=np.complex128)
