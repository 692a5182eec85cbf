"""xsiphon mode 0, suck and flush_siphon restated from wdsp/siphon.c, for the tests of the RXA engine's siphon tap (RXA.c:590).

create_rxa makes the siphon with sipsize 4096, mode 0, insize = dsp_size (RXA.c:392-401).  `Siphon.push` is xsiphon over a whole number of
blocks of insize samples, `suck` is suck() with outsize = size, `flush` is flush_siphon."""
import numpy as np

SIPSIZE = 4096                                              # RXA.c:398; "MUST BE A POWER OF TWO" (siphon.c:63)


class Siphon:
    def __init__(self, insize, sipsize=SIPSIZE):
        assert sipsize & (sipsize - 1) == 0
        self.insize, self.sipsize = int(insize), int(sipsize)
        self.sipbuff = np.zeros(self.sipsize, dtype=np.complex128)         # malloc0, siphon.c:66
        self.idx = 0                                                        # siphon.c:67

    def flush(self):                                        # siphon.c:88-94
        self.sipbuff[:] = 0.0
        self.idx = 0

    def xsiphon(self, block):                               # siphon.c:96-130, mode 0
        a = np.asarray(block, dtype=np.complex128)
        assert a.size == self.insize
        if self.insize >= self.sipsize:                     # :105-106
            self.sipbuff[:] = a[self.insize - self.sipsize:]
            return
        if self.insize > self.sipsize - self.idx:           # :109-113
            first = self.sipsize - self.idx
            second = self.insize - first
        else:                                               # :114-118
            first, second = self.insize, 0
        self.sipbuff[self.idx:self.idx + first] = a[:first]                 # :119
        self.sipbuff[:second] = a[first:first + second]                     # :120
        self.idx += self.insize                             # :121
        if self.idx >= self.sipsize:
            self.idx -= self.sipsize

    def push(self, x):
        x = np.asarray(x, dtype=np.complex128)
        assert x.size % self.insize == 0
        for k in range(0, x.size, self.insize):
            self.xsiphon(x[k:k + self.insize])

    def suck(self, outsize):                                # siphon.c:148-163
        assert 0 <= outsize <= self.sipsize                 # (beyond sipsize the reference leaves sipout as it was)
        out = np.zeros(outsize, dtype=np.complex128)
        mask = self.sipsize - 1
        j = (self.idx - outsize) & mask
        size = self.sipsize - j
        if size >= outsize:
            out[:] = self.sipbuff[j:j + outsize]
        else:
            out[:size] = self.sipbuff[j:]
            out[size:] = self.sipbuff[:outsize - size]
        return out
