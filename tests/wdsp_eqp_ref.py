"""Restatement of WDSP's receive equalizer (create_eqp / xeqp and the eight RXA setters, wdsp/eq.c:166-377) for the tests.

Written from the reference's semantics, not from the HIP code.  The design is eq_impulse as restated in tests/wdsp_fmsq_ref.py; a
minimum-phase design goes through the oracle's mp_imp (wo_mp_imp, fir.c:319-368) with its complex taps kept, as calc_fircore keeps them
(firmin.c:327-328).  The filter is a direct convolution over a persistent delay line of nc - 1 samples:

  * xfircore (firmin.c:409-430) multiplies the stored spectra of the last nc / size input blocks by the masks of the impulse response's
    partitions, which is the convolution of the last nc - 1 + size input samples with the taps;
  * setImpulse_fircore(..., 1) (firmin.c:448-452) makes new masks and leaves the stored spectra alone: the new taps act on the kept line;
  * setNc_fircore (firmin.c:454-466) re-plans and so starts from a zero line: `SetRXAEQNC` with a new nc zeroes `delay`;
  * xeqp with run 0 copies and does not call the fircore (eq.c:202-208): the line stays as it was.

`fircore()` gives the same taps to oracle.pyoracle.Fircore (a fresh fircore, a zero line), which tests/test_eqp_restatement.py holds the
convolution to.  Taps are in create_fircore's form with the 1 / (2 size) of the design undone (the reference's unnormalised inverse
transform of 2 size points restores it), so a 0 dB profile has unit gain."""
import ctypes as C

import numpy as np

from wdsp_fmsq_ref import eq_impulse

DEFAULT_F = [0.0, 32.0, 63.0, 125.0, 250.0, 500.0, 1000.0, 2000.0, 4000.0, 8000.0, 16000.0]       # RXA.c:259
GRPH_F = [0.0, 150.0, 400.0, 1500.0, 6000.0]                                                       # eq.c:333-336


def mp_imp(h):
    """mp_imp(N, h, out, 16, 0) of the oracle library on complex taps h"""
    from oracle import pyoracle
    L = pyoracle.lib()
    L.wo_mp_imp.argtypes = [C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_int]
    L.wo_mp_imp.restype = None
    src = np.ascontiguousarray(h, dtype=np.complex128)
    out = np.zeros_like(src)
    L.wo_mp_imp(src.size, src.ctypes.data, out.ctypes.data, 16, 0)
    return out


def convolve(x, h):
    """sum_k h[k] x[n - k] for the n where every x[n - k] exists, through one transform (error ~1e-16 of the largest output)"""
    n = len(x) + len(h) - 1
    nfft = 1 << (n - 1).bit_length()
    y = np.fft.ifft(np.fft.fft(x, nfft) * np.fft.fft(h, nfft))[:n]
    return y[len(h) - 1:len(x)]


class Eqp:
    """one xeqp instance as create_rxa makes it (RXA.c:257-275)"""

    def __init__(self, rate=48000, size=256, run=0, nc=None, mp=0, taps=None):
        # taps: the filter as the caller has it (nc complex taps, scale 1 / (2 size)) instead of this file's design -- for mp 1 at ctfmode 0,
        # where mp_imp takes the logarithm of skirts that eq_impulse puts at 1e-100 and the transforms' rounding at 1e-17 (DESIGN.md,
        # deviations of xfmsq): such a design is decided by the rounding of whichever FFT made it.  Dropped by the next design setter.
        self.rate, self.size, self.run = float(rate), size, run
        self.nc = max(2048, size) if nc is None else nc
        self.mp = mp
        self.nfreqs, self.F, self.G = 10, list(DEFAULT_F), [0.0] * 11
        self.ctfmode, self.wintype = 0, 0
        self.taps = taps
        self._design()
        self.delay = np.zeros(self.nc - 1, dtype=np.complex128)

    def design(self):
        """the taps create_fircore / setImpulse_fircore get (scale 1 / (2 size)), through mp_imp when mp is set"""
        h = eq_impulse(self.nc, self.nfreqs, self.F, self.G, self.rate, 1.0 / (2.0 * self.size), self.ctfmode, self.wintype).astype(np.complex128)
        return mp_imp(h) if self.mp else h

    def _design(self):
        h = self.design() if self.taps is None else np.asarray(self.taps, dtype=np.complex128)
        assert len(h) == self.nc
        self.h = h * (2.0 * self.size)
        self.taps = None

    def use_taps(self, taps):
        """the current design replaced by the caller's taps (scale 1 / (2 size)), the line kept"""
        assert taps is not None and len(taps) == self.nc
        self.taps = taps
        self._design()

    def fircore(self):
        """a fresh oracle fircore with the taps in use (a zero delay line)"""
        from oracle import pyoracle
        return pyoracle.Fircore(self.size, self.nc, self.h / (2.0 * self.size))

    def flush(self):
        """flush_eqp (eq.c:197-200)"""
        self.delay[:] = 0.0

    # the setters, eq.c:242-377
    def SetRXAEQRun(self, run):
        self.run = run

    def SetRXAEQNC(self, nc):
        if self.nc != nc:
            self.nc = nc
            self._design()
            self.delay = np.zeros(nc - 1, dtype=np.complex128)

    def SetRXAEQMP(self, mp):
        if self.mp != mp:
            self.mp = mp
            self._design()

    def SetRXAEQProfile(self, nfreqs, F, G):
        self.nfreqs, self.F, self.G = nfreqs, list(F[:nfreqs + 1]), list(G[:nfreqs + 1])
        self._design()

    def SetRXAEQCtfmode(self, mode):
        self.ctfmode = mode
        self._design()

    def SetRXAEQWintype(self, wintype):
        self.wintype = wintype
        self._design()

    def SetRXAGrphEQ(self, rxeq):
        self.nfreqs, self.F = 4, list(GRPH_F)
        self.G = [float(rxeq[0]), float(rxeq[1]), float(rxeq[1]), float(rxeq[2]), float(rxeq[3])]
        self.ctfmode = 0
        self._design()

    def SetRXAGrphEQ10(self, rxeq):
        self.nfreqs, self.F = 10, list(DEFAULT_F)
        self.G = [float(v) for v in rxeq[:11]]
        self.ctfmode = 0
        self._design()

    def RXASetNC(self, nc):
        self.SetRXAEQNC(nc)             # RXA.c:941

    def RXASetMP(self, mp):
        self.SetRXAEQMP(mp)             # RXA.c:954

    def process(self, x):
        """xeqp over a whole number of blocks"""
        x = np.asarray(x, dtype=np.complex128)
        assert len(x) % self.size == 0
        if not self.run:
            return x.copy()
        cat = np.concatenate([self.delay, x])
        self.delay = cat[len(cat) - (self.nc - 1):].copy()
        return convolve(cat, self.h)
