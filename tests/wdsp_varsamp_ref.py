"""WDSP's variable-ratio resampler (calc_varsamp, flush_varsamp, hshift and xvarsamp, wdsp/varsamp.c:29-68,104-179) restated sample by
sample in plain Python, for the tests of qh_varsamp_* and the V names.  Literal: the ring and idx_in are kept as the C has them, the
control variables are Python floats (IEEE doubles) stepped statement by statement, the low 16 bits of inv_cvar are cleared through a
uint64 view, hshift forms h[j] + frac * (h[k] - h[j]) with every operation rounded, and the dot product adds its rsize products in the
order j = 0, 1, ... (np.cumsum adds serially).  h is oracle.pyoracle.fir_bandpass, the reference's own arithmetic.

Quirks kept:
  * the entry statements (var, old_inv_cvar, cvar, inv_cvar, dicvar) run whether or not the resampler runs; run = 0 copies;
  * varmode 1 restarts inv_cvar from the previous call's end value and slides it by (new - old) / size a sample, and the cleared bits
    make a slide smaller than 2^-36 of inv_cvar stand still on the way up and move a whole step on the way down;
  * flush_varsamp leaves inv_cvar alone; the rate and bandwidth setters go through calc_varsamp, which starts it from the last var;
  * size = 0 with varmode 1 divides by zero into dicvar, which nothing reads: inv_cvar keeps the old value.

Besides the samples, process returns for every output sample B = sum_j |hs[j]| |x[i - j]|, the scale of the rounding error of a dot
product of these terms in any order.  rec_i / rec_h: the input index inside the call and the h_offset of every output of the last call;
max_k: the largest index of h that hshift has read."""
import numpy as np

_H = {}


def _design(in_rate, out_rate, R, fc, fc_low, gain):
    from oracle import pyoracle
    if out_rate >= in_rate:
        min_rate, norm_rate = float(in_rate), float(in_rate)
    else:
        min_rate, norm_rate = float(out_rate), float(in_rate)
    if fc == 0.0:
        fc = 0.95 * 0.45 * min_rate
    fc_norm_high = fc / norm_rate
    fc_norm_low = -fc_norm_high if fc_low < 0.0 else fc_low / norm_rate
    rsize = int(140.0 * norm_rate / min_rate)
    ncoef = rsize + 1
    ncoef += (R - 1) * (ncoef - 1)
    key = (ncoef, fc_norm_low, fc_norm_high, R, gain)
    if key not in _H:
        _H[key] = pyoracle.fir_bandpass(ncoef, fc_norm_low, fc_norm_high, float(R), 1, 0, float(R) * gain)
    return rsize, ncoef, _H[key]


def clear16(v):
    a = np.array([v], dtype=np.float64)
    a.view(np.uint64)[0] &= np.uint64(0xffffffffffff0000)
    return float(a[0])


class Varsamp:
    def __init__(self, in_rate, out_rate, R, fc=0.0, fc_low=-1.0, gain=1.0, var=1.0, varmode=1, run=1):
        self.run, self.in_rate, self.out_rate, self.fcin, self.fc_low, self.R, self.gain = run, in_rate, out_rate, fc, fc_low, R, gain
        self.var, self.varmode = var, varmode
        self.max_k = -1
        self.rec_i, self.rec_h = [], []
        self.calc()

    def calc(self):                                                     # calc_varsamp, varsamp.c:29-68
        self.nom_ratio = float(self.out_rate) / float(self.in_rate)
        self.cvar = self.var * self.nom_ratio
        self.inv_cvar = 1.0 / self.cvar
        self.old_inv_cvar = self.inv_cvar
        self.dicvar = 0.0
        self.rsize, self.ncoef, self.h = _design(self.in_rate, self.out_rate, self.R, self.fcin, self.fc_low, self.gain)
        self.ring = np.zeros(self.rsize, dtype=np.complex128)
        self.idx_in = self.rsize - 1
        self.h_offset = 0.0
        self.isamps = 0.0
        self._taps = np.arange(self.rsize - 1, -1, -1) * self.R         # j - hidx for i = 0 .. rsize - 1 (the loop runs i downwards)
        self._order = np.arange(self.rsize)

    def flush(self):                                                    # flush_varsamp, varsamp.c:104-110
        self.ring[:] = 0.0
        self.idx_in = self.rsize - 1
        self.h_offset = 0.0
        self.isamps = 0.0

    def state(self):
        return (self.inv_cvar, self.h_offset, self.isamps, self.idx_in)

    def hshift(self):                                                   # varsamp.c:112-122
        pos = float(self.R) * self.h_offset
        hidx = int(pos)
        frac = pos - float(hidx)
        j = hidx + self._taps
        self.max_k = max(self.max_k, int(j[0]) + 1)
        hj = self.h[j]
        return hj + frac * (self.h[j + 1] - hj)

    def process(self, x, var):                                          # xvarsamp, varsamp.c:124-179
        """-> (out, B)"""
        x = np.asarray(x, dtype=np.complex128)
        size = len(x)
        self.rec_i, self.rec_h = [], []
        self.var = var
        self.old_inv_cvar = self.inv_cvar
        self.cvar = self.var * self.nom_ratio
        self.inv_cvar = 1.0 / self.cvar
        if self.varmode:
            with np.errstate(all="ignore"):
                self.dicvar = float(np.float64(self.inv_cvar - self.old_inv_cvar) / np.float64(size))
            self.inv_cvar = self.old_inv_cvar
        else:
            self.dicvar = 0.0
        if not self.run:
            return x.copy(), np.abs(x)
        out, bound = [], []
        rs = self.rsize
        for i in range(size):
            self.ring[self.idx_in] = x[i]
            self.inv_cvar += self.dicvar
            self.inv_cvar = clear16(self.inv_cvar)
            self.delta = 1.0 - self.inv_cvar
            while self.isamps < 1.0:
                hs = self.hshift()
                self.rec_i.append(i)
                self.rec_h.append(self.h_offset)
                self.h_offset += self.delta
                while self.h_offset >= 1.0:
                    self.h_offset -= 1.0
                while self.h_offset < 0.0:
                    self.h_offset += 1.0
                idx = self.idx_in + self._order
                idx[idx >= rs] -= rs
                r = self.ring[idx]
                out.append(complex(np.cumsum(hs * r.real)[-1], np.cumsum(hs * r.imag)[-1]))
                bound.append(float(np.sum(np.abs(hs) * np.abs(r))))
                self.isamps += self.inv_cvar
            self.isamps -= 1.0
            self.idx_in -= 1
            if self.idx_in < 0:
                self.idx_in = rs - 1
        return np.array(out, dtype=np.complex128), np.array(bound, dtype=np.float64)

    # setInRate / setOutRate / setBandwidth_varsamp, varsamp.c:193-226
    def set_rates(self, in_rate, out_rate):
        self.in_rate, self.out_rate = in_rate, out_rate
        self.calc()

    def set_bandwidth(self, fc_low, fc_high):
        if fc_low != self.fc_low or fc_high != self.fcin:
            self.fc_low, self.fcin = fc_low, fc_high
            self.calc()


def run_cuts(vs, x, cuts, var):
    """x through `vs` in the calls [cuts[k], cuts[k+1]) with var[k] -> (out, B, counts)."""
    ys, bs, counts = [], [], []
    for k, (a, b) in enumerate(zip(cuts[:-1], cuts[1:])):
        y, bd = vs.process(x[a:b], var[k])
        ys.append(y); bs.append(bd); counts.append(len(y))
    return np.concatenate(ys), np.concatenate(bs), counts
