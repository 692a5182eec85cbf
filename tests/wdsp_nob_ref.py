"""WDSP's second noise blanker (NOB: xnob and its setters, wdsp/nobII.c:36-155, 157-495, 605-734) restated sample by sample in plain
Python, for the tests of qh_nob_* and the EXT names.  Written from the behaviour, quirks included:

  * one ring of dline_size = 50690 slots (whatever the rate) holds the samples and their impulse flags; the newest sample is written
    D = adv_slew + adv + 1 + max_imp_seq + hang + hang_slew + 10 slots ahead of the one that leaves, and the machine looks at the flag
    adv_slew + adv + 1 slots ahead of it;
  * avg already holds the current sample when the sample is compared with avg * threshold;
  * the ten most recent samples without a flag, at or before out + adv_slew, are kept on every sample (bfbuff);
  * a flag under the scan point in state 0 sets up one blank: the flags ahead are walked, every impulse stretched by hang + hang_slew,
    sequences closer than adv_slew + adv merged, up to max_imp_seq samples; beyond that the overflow path (states 5 to 9) zeroes the
    output until a whole window of flags is clear;
  * the look-ahead and the gather of the next ten clean samples read the ring where they point, also ahead of the write position:
    there the slot still holds what was written dline_size samples earlier (or the flush's zeros).  `read_ahead` counts such reads;
  * that gather stops after one whole turn of the ring, the taps it has not found being zeros (the reference's loop does not end when
    the ring holds fewer than ten slots without a flag); `short_gathers` counts them;
  * modes: 0 zeros, 1 the backward 10-tap sum, 2 the mean of both sums, 3 the forward sum, 4 a line from one to the other, stepped by
    repeated addition;
  * run = 0 copies the input undelayed and leaves every piece of state as it is; samplerate, tau, hangtime, advtime and backtau start
    the blanker over (init_nob: zeroed ring); run, mode, threshold and the buffer size reset nothing, and I, Q, deltaI, deltaQ persist,
    so a mode set during a blank shows at the next set-up.

math.cos / math.exp are the C library's, so awave[], hwave[] and backmult are the numbers the host side of the library computes.

`margin` is the smallest |mag - avg * threshold| / (avg * threshold) seen so far: how far the closest compare sat from flipping.
`blanks` counts set-ups, `merges` the sequences joined to an earlier one by the look-ahead, `overflows` the set-ups that took the
overflow path, `fills` keeps (step, I1, Q1, I2, Q2, I, Q, deltaI, deltaQ, adv_count + blank_count) of every blank that was filled."""
import math

import numpy as np

MAX_ADV_SLEW_TIME = 0.002
MAX_ADV_TIME = 0.002
MAX_HANG_SLEW_TIME = 0.002
MAX_HANG_TIME = 0.002
MAX_SEQ_TIME = 0.025
MAX_SAMPLERATE = 1536000.0
FILTERLEN = 10
FCOEFS = (0.308720593, 0.216104415, 0.151273090, 0.105891163, 0.074123814, 0.051886670, 0.036320669, 0.025424468, 0.017797128, 0.012457989)


class Nob:
    def __init__(self, samplerate, mode, slewtime, hangtime, advtime, backtau, threshold, run=1, max_imp_seq_time=0.025):
        self.run, self.mode = run, mode
        self.samplerate = float(samplerate)
        self.advslewtime = self.hangslewtime = slewtime
        self.hangtime, self.advtime, self.backtau, self.threshold = hangtime, advtime, backtau, threshold
        self.max_imp_seq_time = max_imp_seq_time
        self.dline_size = int(MAX_SAMPLERATE * (MAX_ADV_SLEW_TIME + MAX_ADV_TIME + MAX_HANG_SLEW_TIME + MAX_HANG_TIME + MAX_SEQ_TIME) + 2)
        self.time = self.blank_count = 0
        self.I = self.Q = self.deltaI = self.deltaQ = 0.0
        self.I1 = self.Q1 = self.I2 = self.Q2 = 0.0
        self.Ilast = self.Qlast = self.Inext = self.Qnext = 0.0
        self.margin = math.inf
        self.triggers = self.blanks = self.merges = self.overflows = self.read_ahead = self.short_gathers = 0
        self.steps = 0                                  # samples processed while running, over all restarts
        self.fills = []
        self._init()

    def _init(self):
        sr = self.samplerate
        self.adv_slew_count = int(self.advslewtime * sr)
        self.adv_count = int(self.advtime * sr)
        self.hang_count = int(self.hangtime * sr)
        self.hang_slew_count = int(self.hangslewtime * sr)
        self.max_imp_seq = int(self.max_imp_seq_time * sr)
        self.backmult = math.exp(-1.0 / (sr * self.backtau))
        self.ombackmult = 1.0 - self.backmult
        self.awave = [0.5 * math.cos((i + 1) * (math.pi / (self.adv_slew_count + 1))) for i in range(self.adv_slew_count)]
        self.hwave = [0.5 * math.cos(i * (math.pi / self.hang_slew_count)) for i in range(self.hang_slew_count)]
        self.flush()

    def flush(self):
        self.out_idx = 0
        self.scan_idx = self.out_idx + self.adv_slew_count + self.adv_count + 1
        self.in_idx = self.scan_idx + self.max_imp_seq + self.hang_count + self.hang_slew_count + FILTERLEN
        if self.in_idx >= self.dline_size:
            raise ValueError("the write position would start beyond the ring (the reference overruns it)")
        self.state = 0
        self.overflow = 0
        self.avg = 1.0
        self.bfb_in_idx = FILTERLEN - 1
        self.ffb_in_idx = FILTERLEN - 1
        self.dline = [0j] * self.dline_size
        self.imp = [0] * self.dline_size
        self.bfbuff = [0j] * FILTERLEN
        self.ffbuff = [0j] * FILTERLEN

    @property
    def delay(self):
        return self.adv_slew_count + self.adv_count + 1 + self.max_imp_seq + self.hang_count + self.hang_slew_count + FILTERLEN

    @property
    def counts(self):
        return self.adv_slew_count, self.adv_count, self.hang_count, self.hang_slew_count, self.max_imp_seq

    # the setters of nobII.c:650-734
    def SetRun(self, run):
        self.run = run

    def SetMode(self, mode):
        self.mode = mode

    def SetSamplerate(self, rate):
        self.samplerate = float(int(rate))
        self._init()

    def SetTau(self, tau):
        self.advslewtime = self.hangslewtime = tau
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

    def _ahead(self, idx):
        """1 if ring slot idx has not been written since the sample now leaving was: a read ahead of the write position"""
        size = self.dline_size
        return 1 if (idx - self.out_idx) % size > (self.in_idx - self.out_idx) % size else 0

    def _setup(self):
        """state 0 with a flag under the scan point, nobII.c:201-333"""
        size, imp, dline = self.dline_size, self.imp, self.dline
        self.blanks += 1
        self.time = 0
        self.state = 1 if self.adv_slew_count > 0 else 2 if self.adv_count > 0 else 3
        tidx = self.scan_idx
        self.blank_count = 0
        while True:
            hcount = 0
            while (imp[tidx] > 0 or hcount > 0) and self.blank_count < self.max_imp_seq:
                self.read_ahead += self._ahead(tidx)
                self.blank_count += 1
                if hcount > 0:
                    hcount -= 1
                if imp[tidx] > 0:
                    hcount = self.hang_count + self.hang_slew_count
                tidx += 1
                if tidx >= size:
                    tidx -= size
            j, length, lidx = 1, 0, tidx
            while j <= self.adv_slew_count + self.adv_count and length == 0:
                self.read_ahead += self._ahead(lidx)
                if imp[lidx] == 1:
                    length = j
                    tidx = lidx
                lidx += 1
                if lidx >= size:
                    lidx -= size
                j += 1
            self.blank_count += length
            if self.blank_count > self.max_imp_seq:
                self.blank_count = self.max_imp_seq
                self.overflow = 1
                break
            if length == 0:
                break
            self.merges += 1
        if self.overflow == 0:
            self.blank_count -= self.hang_slew_count
            self.read_ahead += self._ahead(tidx)
            self.Inext, self.Qnext = dline[tidx].real, dline[tidx].imag
            mode = self.mode
            if mode in (1, 2, 4):
                k = self.bfb_in_idx
                i1 = q1 = 0.0
                for c in FCOEFS:
                    i1 += c * self.bfbuff[k].real
                    q1 += c * self.bfbuff[k].imag
                    k -= 1
                    if k < 0:
                        k += FILTERLEN
                self.I1, self.Q1 = i1, q1
            if mode in (2, 3, 4):
                ff_idx = self.scan_idx + self.blank_count
                if ff_idx >= size:
                    ff_idx -= size
                ffcount = looked = 0
                while ffcount < FILTERLEN:
                    if looked == size:                                  # one whole turn: the missing taps are zeros
                        self.short_gathers += 1
                    if looked >= size or imp[ff_idx] == 0:
                        self.read_ahead += self._ahead(ff_idx) if looked < size else 0
                        self.ffb_in_idx += 1
                        if self.ffb_in_idx == FILTERLEN:
                            self.ffb_in_idx -= FILTERLEN
                        self.ffbuff[self.ffb_in_idx] = dline[ff_idx] if looked < size else 0j
                        ffcount += 1
                    looked += 1
                    ff_idx += 1
                    if ff_idx >= size:
                        ff_idx -= size
                k = self.ffb_in_idx + 1
                if k >= FILTERLEN:
                    k -= FILTERLEN
                i2 = q2 = 0.0
                for c in FCOEFS:
                    i2 += c * self.ffbuff[k].real
                    q2 += c * self.ffbuff[k].imag
                    k += 1
                    if k >= FILTERLEN:
                        k -= FILTERLEN
                self.I2, self.Q2 = i2, q2
            if mode == 0:
                self.deltaI = self.deltaQ = 0.0
                self.I = self.Q = 0.0
            elif mode == 1:
                self.deltaI = self.deltaQ = 0.0
                self.I, self.Q = self.I1, self.Q1
            elif mode == 2:
                self.deltaI = self.deltaQ = 0.0
                self.I, self.Q = 0.5 * (self.I1 + self.I2), 0.5 * (self.Q1 + self.Q2)
            elif mode == 3:
                self.deltaI = self.deltaQ = 0.0
                self.I, self.Q = self.I2, self.Q2
            elif mode == 4:
                self.deltaI = (self.I2 - self.I1) / (self.adv_count + self.blank_count)
                self.deltaQ = (self.Q2 - self.Q1) / (self.adv_count + self.blank_count)
                self.I, self.Q = self.I1, self.Q1
            self.fills.append((self.steps, self.I1, self.Q1, self.I2, self.Q2, self.I, self.Q, self.deltaI, self.deltaQ, self.adv_count + self.blank_count))
        else:
            self.overflows += 1
            if self.adv_slew_count > 0:
                self.state = 5
            else:
                self.state = 6
                self.time = 0
                self.blank_count += self.adv_count + FILTERLEN

    def process(self, x):
        x = np.asarray(x, dtype=np.complex128)
        if not self.run:
            return x.copy()
        n = len(x)
        out = np.zeros(n, dtype=np.complex128)
        re, im = x.real.tolist(), x.imag.tolist()
        size, imp, dline = self.dline_size, self.imp, self.dline
        bm, om = self.backmult, self.ombackmult
        sqrt = math.sqrt
        for i in range(n):
            a, b = re[i], im[i]
            dline[self.in_idx] = complex(a, b)
            mag = sqrt(a * a + b * b)
            self.avg = bm * self.avg + om * mag
            lim = self.avg * self.threshold
            if lim > 0.0:
                m = abs(mag - lim) / lim
                if m < self.margin:
                    self.margin = m
            if mag > lim:
                imp[self.in_idx] = 1
                self.triggers += 1
            else:
                imp[self.in_idx] = 0
            bf_idx = self.out_idx + self.adv_slew_count
            if bf_idx >= size:
                bf_idx -= size
            if imp[bf_idx] == 0:
                self.bfb_in_idx += 1
                if self.bfb_in_idx == FILTERLEN:
                    self.bfb_in_idx -= FILTERLEN
                self.bfbuff[self.bfb_in_idx] = dline[bf_idx]
            st = self.state
            if st == 0:
                d = dline[self.out_idx]
                out[i] = d
                self.Ilast, self.Qlast = d.real, d.imag
                if imp[self.scan_idx] > 0:
                    self._setup()
            elif st == 1:
                scale = 0.5 + self.awave[self.time]
                out[i] = complex(self.Ilast * scale + (1.0 - scale) * self.I, self.Qlast * scale + (1.0 - scale) * self.Q)
                self.time += 1
                if self.time == self.adv_slew_count:
                    self.time = 0
                    self.state = 2 if self.adv_count > 0 else 3
            elif st == 2:
                out[i] = complex(self.I, self.Q)
                self.I += self.deltaI
                self.Q += self.deltaQ
                self.time += 1
                if self.time == self.adv_count:
                    self.state = 3
                    self.time = 0
            elif st == 3:
                out[i] = complex(self.I, self.Q)
                self.I += self.deltaI
                self.Q += self.deltaQ
                self.time += 1
                if self.time == self.blank_count:
                    if self.hang_slew_count > 0:
                        self.state = 4
                        self.time = 0
                    else:
                        self.state = 0
            elif st == 4:
                scale = 0.5 - self.hwave[self.time]
                out[i] = complex(self.Inext * scale + (1.0 - scale) * self.I, self.Qnext * scale + (1.0 - scale) * self.Q)
                self.time += 1
                if self.time == self.hang_slew_count:
                    self.state = 0
            elif st == 5:
                scale = 0.5 + self.awave[self.time]
                out[i] = complex(self.Ilast * scale, self.Qlast * scale)
                self.time += 1
                if self.time == self.adv_slew_count:
                    self.state = 6
                    self.time = 0
                    self.blank_count += self.adv_count + FILTERLEN
            elif st == 6:
                self.time += 1
                if self.time == self.blank_count:
                    self.state = 7
            elif st == 7:
                staydown = 0
                self.time = 0
                tidx = self.scan_idx + self.hang_slew_count + self.hang_count
                if tidx >= size:
                    tidx -= size
                window = self.adv_count + self.adv_slew_count + self.hang_slew_count + self.hang_count
                while self.time <= window:
                    self.time += 1
                    if imp[tidx] == 1:
                        staydown = 1
                    tidx -= 1
                    if tidx < 0:
                        tidx += size
                self.time += 1                                          # the failed compare increments too
                if staydown == 0:
                    if self.hang_count > 0:
                        self.state = 8
                        self.time = 0
                    elif self.hang_slew_count > 0:
                        self.state = 9
                        self.time = 0
                        tidx = self.scan_idx + self.hang_slew_count + self.hang_count - self.adv_count - self.adv_slew_count
                        if tidx >= size:
                            tidx -= size
                        if tidx < 0:
                            tidx += size
                        self.Inext, self.Qnext = dline[tidx].real, dline[tidx].imag
                    else:
                        self.state = 0
                        self.overflow = 0
            elif st == 8:
                self.time += 1
                if self.time == self.hang_count:
                    if self.hang_slew_count > 0:
                        self.state = 9
                        self.time = 0
                        tidx = self.scan_idx + self.hang_slew_count - self.adv_count - self.adv_slew_count
                        if tidx >= size:
                            tidx -= size
                        if tidx < 0:
                            tidx += size
                        self.Inext, self.Qnext = dline[tidx].real, dline[tidx].imag
                    else:
                        self.state = 0
                        self.overflow = 0
            else:
                scale = 0.5 - self.hwave[self.time]
                out[i] = complex(self.Inext * scale, self.Qnext * scale)
                self.time += 1
                if self.time >= self.hang_slew_count:
                    self.state = 0
                    self.overflow = 0
            self.in_idx += 1
            if self.in_idx == size:
                self.in_idx = 0
            self.scan_idx += 1
            if self.scan_idx == size:
                self.scan_idx = 0
            self.out_idx += 1
            if self.out_idx == size:
                self.out_idx = 0
            self.steps += 1
        return out


def run_cuts(nob, x, cuts):
    """x through `nob` in the calls [cuts[k], cuts[k+1])."""
    parts = [nob.process(x[a:b]) for a, b in zip(cuts[:-1], cuts[1:])]
    return np.concatenate(parts) if parts else np.zeros(0, dtype=np.complex128)
