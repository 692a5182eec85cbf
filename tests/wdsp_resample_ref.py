"""WDSP's fixed-ratio resampler (calc_resample, flush_resample, xresample and the setters, wdsp/resample.c:35-204; create_resampleF,
flush_resampleF and xresampleF, resample.c:236-330) restated sample by sample in plain Python, for the tests of qh_resample_* and the V /
FV names.  Literal: the ring and idx_in are kept as the C has them, phnum steps through `while phnum < L`, the dot product adds its cpp
products in the order j = 0, 1, ... (np.cumsum adds serially), and the real-float form widens with float() on the way in and narrows with
np.float32 on the way out.  The prototype is oracle.pyoracle.fir_bandpass, the reference's own arithmetic; `taps=` (phase-major
h[L][cpp], flat or two-dimensional) puts another table in its place, so a test can hand over the library's.

Besides the samples, process returns for every output sample B = sum_j |h[n + j]| |ring[...]|, per component (real and imaginary
parts of B for the complex form): the scale of the rounding error of a dot product of these terms in any order.  The real-float
form returns the double sums as well, so a test can tell how close a sum lies to a float rounding midpoint."""
import numpy as np


def _gcd_lm(in_rate, out_rate):
    x, y = in_rate, out_rate
    while y != 0:
        x, y = y, x % y
    return out_rate // x, in_rate // x


def calc_resample(in_rate, out_rate, fc=0.0, ncoef=0, gain=1.0, fc_low=-1.0):
    """resample.c:35-72 -> (L, M, ncoef, cpp, h phase-major flat)"""
    from oracle import pyoracle
    L, M = _gcd_lm(in_rate, out_rate)
    min_rate = in_rate if in_rate < out_rate else out_rate
    if fc == 0.0:
        fc = 0.45 * float(min_rate)
    full_rate = float(in_rate * L)
    fc_norm_high = fc / full_rate
    fc_norm_low = -fc_norm_high if fc_low < 0.0 else fc_low / full_rate
    if ncoef == 0:
        ncoef = int(140.0 * full_rate / min_rate)
    ncoef = (ncoef // L + 1) * L
    cpp = ncoef // L
    impulse = pyoracle.fir_bandpass(ncoef, fc_norm_low, fc_norm_high, 1.0, 1, 0, gain * float(L))
    h = np.ascontiguousarray(impulse.reshape(cpp, L).T).reshape(-1)     # h[j * cpp + k / L] = impulse[j + k]
    return L, M, ncoef, cpp, h


def calc_resample_f(in_rate, out_rate):
    """create_resampleF's design, resample.c:250-273 -> (L, M, ncoef, cpp, h phase-major flat)"""
    from oracle import pyoracle
    L, M = _gcd_lm(in_rate, out_rate)
    min_rate = in_rate if in_rate < out_rate else out_rate
    fc = 0.45 * float(min_rate)
    full_rate = float(in_rate * L)
    fc_norm = fc / full_rate
    ncoef = int(60.0 / fc_norm)
    ncoef = (ncoef // L + 1) * L
    cpp = ncoef // L
    impulse = pyoracle.fir_bandpass(ncoef, -fc_norm, +fc_norm, 1.0, 1, 0, float(L))
    h = np.ascontiguousarray(impulse.reshape(cpp, L).T).reshape(-1)
    return L, M, ncoef, cpp, h


class _Base:
    def _install(self, design, taps):
        self.L, self.M, self.ncoef, self.cpp, h = design
        if taps is not None:
            h = np.ascontiguousarray(taps, dtype=np.float64).reshape(-1)
            assert h.size == self.ncoef, (h.size, self.ncoef)
        self.h = h
        self.ringsize = self.cpp
        self.ring = np.zeros(self.ringsize, dtype=self.ring_dtype)
        self.idx_in = self.ringsize - 1
        self.phnum = 0
        self._order = np.arange(self.cpp)

    def flush(self):                                                    # flush_resample(F), resample.c:112-118, 289-294
        self.ring[:] = 0
        self.idx_in = self.ringsize - 1
        self.phnum = 0

    def _walk(self, x, dot):
        for i in range(len(x)):
            self.ring[self.idx_in] = x[i]
            while self.phnum < self.L:
                n = self.cpp * self.phnum
                idx = self.idx_in + self._order
                idx[idx >= self.ringsize] -= self.ringsize
                dot(self.h[n:n + self.cpp], self.ring[idx])
                self.phnum += self.M
            self.phnum -= self.L
            self.idx_in -= 1
            if self.idx_in < 0:
                self.idx_in = self.ringsize - 1


class Resample(_Base):
    """RESAMPLE, complex doubles"""
    ring_dtype = np.complex128

    def __init__(self, in_rate, out_rate, fc=0.0, ncoef=0, gain=1.0, run=1, taps=None):
        self.run, self.in_rate, self.out_rate, self.fcin, self.fc_low, self.ncoefin, self.gain = run, in_rate, out_rate, fc, -1.0, ncoef, gain
        self.calc(taps)

    def calc(self, taps=None):                                          # calc_resample
        self._install(calc_resample(self.in_rate, self.out_rate, self.fcin, self.ncoefin, self.gain, self.fc_low), taps)

    def process(self, x):                                               # xresample, resample.c:121-157
        """-> (out complex128, B complex128: the bound's scale of the real and of the imaginary part); run = 0 -> (x, |.| of x), and
        xresample's return value is 0 then"""
        x = np.asarray(x, dtype=np.complex128)
        if not self.run:
            return x.copy(), np.abs(x.real) + 1j * np.abs(x.imag)
        out, bound = [], []

        def dot(h, r):
            out.append(complex(np.cumsum(h * r.real)[-1], np.cumsum(h * r.imag)[-1]))
            a = np.abs(h)
            bound.append(complex(float(np.sum(a * np.abs(r.real))), float(np.sum(a * np.abs(r.imag)))))

        self._walk(x, dot)
        return np.array(out, dtype=np.complex128), np.array(bound, dtype=np.complex128)

    # setInRate / setOutRate / setFCLow / setBandwidth_resample, resample.c:171-204
    def set_rates(self, in_rate, out_rate, taps=None):
        self.in_rate, self.out_rate = in_rate, out_rate
        self.calc(taps)

    def set_fc_low(self, fc_low, taps=None):
        if fc_low != self.fc_low:
            self.fc_low = fc_low
            self.calc(taps)

    def set_bandwidth(self, fc_low, fc_high, taps=None):
        if fc_low != self.fc_low or fc_high != self.fcin:
            self.fc_low, self.fcin = fc_low, fc_high
            self.calc(taps)


class ResampleF(_Base):
    """RESAMPLEF, real floats through a ring of doubles"""
    ring_dtype = np.float64

    def __init__(self, in_rate, out_rate, run=1, taps=None):
        self.run, self.in_rate, self.out_rate = run, in_rate, out_rate
        self.calc(taps)

    def calc(self, taps=None):
        self._install(calc_resample_f(self.in_rate, self.out_rate), taps)

    def set_rates(self, in_rate, out_rate, taps=None):
        self.in_rate, self.out_rate = in_rate, out_rate
        self.calc(taps)

    def process(self, x):                                               # xresampleF, resample.c:296-330
        """-> (out float32, B float64, I float64: the sums before (float)I)"""
        x = np.asarray(x, dtype=np.float32)
        if not self.run:
            return x.copy(), np.abs(x).astype(np.float64), x.astype(np.float64)
        out, bound, sums = [], [], []

        def dot(h, r):
            I = float(np.cumsum(h * r)[-1])
            sums.append(I)
            out.append(np.float32(I))
            bound.append(float(np.sum(np.abs(h) * np.abs(r))))

        self._walk([float(v) for v in x], dot)
        return np.array(out, dtype=np.float32), np.array(bound, dtype=np.float64), np.array(sums, dtype=np.float64)


def run_cuts(rs, x, cuts):
    """x through `rs` in the calls [cuts[k], cuts[k+1]) -> per call the tuple process returns"""
    return [rs.process(x[a:b]) for a, b in zip(cuts[:-1], cuts[1:])]
