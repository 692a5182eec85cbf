"""A literal restatement of WDSP's iobuffs (wdsp/iobuffs.c) around any block function: create_iobuffs (:384-423), create_slews / flush_slews
(:47-96), upslew0 (:98-160), downslew0 (:226-300), fexchange0 (:464-516) and dexchange (:583-604), with pre_main_build's sizes
(wdsp/channel.c:37-58).  The DSP thread (main.c:40-58) runs synchronously: every BuffReady count released by fexchange0 is one dexchange
and one call of `block` before fexchange0 goes on to its output, which is the order a single-threaded caller sees.

    block(x) -> y      dsp_insize complex samples in, dsp_outsize out: one xrxa (wo_xrxa_block of an oracle channel, or a composition)

A channel whose sizes or rates change is a new Iobuffs (SetInputBuffsize ... SetAllRates destroy and create them, channel.c:169-258) around
the block function that goes on.  bfo = 1 (block for output), as every caller here opens its channels.
"""
import numpy as np

DSP_MULT = 2            # comm.h:118
BEGIN, DELAYUP, UPSLEW, ON, DELAYDOWN, DOWNSLEW, ZERO, OFF = range(8)


class Iobuffs:
    def __init__(self, block, in_size, dsp_size, in_rate, dsp_rate, out_rate, tdelayup=0.010, tslewup=0.025, tdelaydown=0.0, tslewdown=0.010,
                 state=1):
        self.block = block
        self.in_size, self.in_rate, self.out_rate = in_size, in_rate, out_rate
        self.tdelayup, self.tslewup, self.tdelaydown, self.tslewdown = tdelayup, tslewup, tdelaydown, tslewdown
        # pre_main_build, channel.c:39-52
        self.dsp_insize = dsp_size * (in_rate // dsp_rate) if in_rate >= dsp_rate else dsp_size // (dsp_rate // in_rate)
        self.dsp_outsize = dsp_size * (out_rate // dsp_rate) if out_rate >= dsp_rate else dsp_size // (dsp_rate // out_rate)
        self.out_size = in_size // (in_rate // out_rate) if in_rate >= out_rate else in_size * (out_rate // in_rate)
        # create_iobuffs, iobuffs.c:384-423
        self.r1_outsize = self.dsp_insize
        self.r1_size = max(self.r1_outsize, in_size)
        self.r2_insize = self.dsp_outsize
        self.r2_size = max(self.out_size, self.r2_insize)
        self.r1_active, self.r2_active = DSP_MULT * self.r1_size, DSP_MULT * self.r2_size
        self.r1 = np.zeros(self.r1_active, dtype=np.complex128)
        self.r2 = np.zeros(self.r2_active, dtype=np.complex128)
        self.r1_inidx = self.r1_outidx = self.r1_unqueued = 0
        self.r2_inidx = (DSP_MULT - 1) * self.r2_size
        self.r2_outidx = 0
        self.r2_havesamps = (DSP_MULT - 1) * self.r2_size
        n = self.r2_havesamps // self.out_size
        self.r2_unqueued = self.r2_havesamps - n * self.out_size
        self.sem_buffready, self.sem_outready = 0, n
        self.outbuff = np.zeros(self.dsp_outsize, dtype=np.complex128)      # what create_main leaves: the first dexchange moves zeros
        self.create_slews()
        self.exchange = 0
        if state:                   # OpenChannel, channel.c:93-99
            self.upflag = 1
            self.exchange = 1

    def create_slews(self):         # iobuffs.c:47-80
        self.ustate = self.dstate = BEGIN
        self.ucount = self.dcount = 0
        self.ndelup, self.ndeldown = int(self.tdelayup * self.in_rate), int(self.tdelaydown * self.out_rate)
        self.ntup, self.ntdown = int(self.tslewup * self.in_rate), int(self.tslewdown * self.out_rate)
        self.cup, self.cdown = np.zeros(self.ntup + 1), np.zeros(self.ntdown + 1)
        delta, theta = (np.pi / self.ntup if self.ntup else 0.0), 0.0
        for i in range(self.ntup + 1):
            self.cup[i] = 0.5 * (1.0 - np.cos(theta))
            theta += delta
        delta, theta = (np.pi / self.ntdown if self.ntdown else 0.0), 0.0
        for i in range(self.ntdown + 1):
            self.cdown[i] = 0.5 * (1.0 + np.cos(theta))
            theta += delta
        self.upflag = self.downflag = 0

    def flush_slews(self):          # iobuffs.c:88-96
        self.ustate = self.dstate = BEGIN
        self.ucount = self.dcount = 0
        self.upflag = self.downflag = 0

    # SetChannelTDelayUp ... SetChannelTSlewDown, channel.c:301-347
    def SetChannelTDelayUp(self, time):
        self.tdelayup = time
        self.ndelup = int(time * self.in_rate)
        self.flush_slews()

    def SetChannelTSlewUp(self, time):
        self.tslewup = time
        self.create_slews()

    def SetChannelTDelayDown(self, time):
        self.tdelaydown = time
        self.ndeldown = int(time * self.out_rate)
        self.flush_slews()

    def SetChannelTSlewDown(self, time):
        self.tslewdown = time
        self.create_slews()

    def upslew0(self, pin):         # iobuffs.c:98-160
        pout = self.r1[self.r1_inidx:self.r1_inidx + self.in_size]
        for i in range(self.in_size):
            v = pin[i]
            if self.ustate == BEGIN:
                pout[i] = 0.0
                if v != 0.0:
                    if self.ndelup > 0:
                        self.ustate, self.ucount = DELAYUP, self.ndelup
                    elif self.ntup > 0:
                        self.ustate, self.ucount = UPSLEW, self.ntup
                    else:
                        self.ustate = ON
            elif self.ustate == DELAYUP:
                pout[i] = 0.0
                self.ucount -= 1
                if self.ucount + 1 == 0:
                    if self.ntup > 0:
                        self.ustate, self.ucount = UPSLEW, self.ntup
                    else:
                        self.ustate = ON
            elif self.ustate == UPSLEW:
                pout[i] = v * self.cup[self.ntup - self.ucount]
                self.ucount -= 1
                if self.ucount + 1 == 0:
                    self.ustate = ON
            else:
                pout[i] = v
                if i == self.in_size - 1:
                    self.ustate = BEGIN
                    self.upflag = 0

    def downslew0(self, pout):      # iobuffs.c:226-300
        pin = self.r2[self.r2_outidx:self.r2_outidx + self.out_size]
        for i in range(self.out_size):
            v = pin[i]
            if self.dstate == BEGIN:
                pout[i] = v
                if self.ndeldown > 0:
                    self.dstate, self.dcount = DELAYDOWN, self.ndeldown
                elif self.ntdown > 0:
                    self.dstate, self.dcount = DOWNSLEW, self.ntdown
                else:
                    self.dstate, self.dcount = ZERO, self.out_size
            elif self.dstate == DELAYDOWN:
                pout[i] = v
                self.dcount -= 1
                if self.dcount + 1 == 0:
                    if self.ntdown > 0:
                        self.dstate, self.dcount = DOWNSLEW, self.ntdown
                    else:
                        self.dstate, self.dcount = ZERO, self.out_size
            elif self.dstate == DOWNSLEW:
                pout[i] = v * self.cdown[self.ntdown - self.dcount]
                self.dcount -= 1
                if self.dcount + 1 == 0:
                    self.dstate, self.dcount = ZERO, self.out_size
            elif self.dstate == ZERO:
                pout[i] = 0.0
                self.dcount -= 1
                if self.dcount + 1 == 0:
                    self.dstate = OFF
            else:
                pout[i] = 0.0
                if i == self.out_size - 1:
                    self.dstate = BEGIN
                    self.downflag = 0

    def dexchange(self):            # iobuffs.c:583-604; returns the DSP block's input
        self.r2_havesamps += self.r2_insize
        self.r2[self.r2_inidx:self.r2_inidx + self.r2_insize] = self.outbuff
        self.r2_inidx += self.r2_insize
        if self.r2_inidx == self.r2_active:
            self.r2_inidx = 0
        self.r2_unqueued += self.r2_insize
        if self.r2_unqueued >= self.out_size:
            n = self.r2_unqueued // self.out_size
            self.sem_outready += n
            self.r2_unqueued -= n * self.out_size
        x = self.r1[self.r1_outidx:self.r1_outidx + self.r1_outsize].copy()
        self.r1_outidx += self.r1_outsize
        if self.r1_outidx == self.r1_active:
            self.r1_outidx = 0
        return x

    def fexchange0(self, pin):      # iobuffs.c:464-516; returns (out, error), out None when the exchange is off (`out` is left alone)
        if not self.exchange:
            return None, 0
        error = 0
        pin = np.asarray(pin, dtype=np.complex128)
        assert pin.size == self.in_size
        if self.upflag:
            self.upslew0(pin)
        else:
            self.r1[self.r1_inidx:self.r1_inidx + self.in_size] = pin
        self.r1_unqueued += self.in_size
        if self.r1_unqueued >= self.r1_outsize:
            n = self.r1_unqueued // self.r1_outsize
            self.sem_buffready += n
            self.r1_unqueued -= n * self.r1_outsize
        self.r1_inidx += self.in_size
        if self.r1_inidx == self.r1_active:
            self.r1_inidx = 0
        while self.sem_buffready > 0:       # the DSP thread, main.c:40-58
            self.sem_buffready -= 1
            self.outbuff = np.asarray(self.block(self.dexchange()), dtype=np.complex128)
            assert self.outbuff.size == self.dsp_outsize
        self.r2_havesamps = max(self.r2_havesamps - self.out_size, 0)
        out = np.zeros(self.out_size, dtype=np.complex128)
        if self.sem_outready > 0:           # WaitForSingleObject (Sem_OutReady) returns
            self.sem_outready -= 1
            if self.downflag:
                self.downslew0(out)
                if not self.downflag:
                    self.exchange = 0
            else:
                out[:] = self.r2[self.r2_outidx:self.r2_outidx + self.out_size]
        else:                               # the reference would block for ever: reported the way its non-bfo path does
            error = -2
        self.r2_outidx += self.out_size
        if self.r2_outidx == self.r2_active:
            self.r2_outidx = 0
        return out, error

    def run(self, x):
        """x (a whole number of in_size blocks) through fexchange0: the out_size blocks in a row, and how many calls reported an error;
        ends where the exchange goes off"""
        x = np.asarray(x, dtype=np.complex128)
        assert x.size % self.in_size == 0
        outs, errs = [], 0
        for b in range(x.size // self.in_size):
            y, err = self.fexchange0(x[b * self.in_size:(b + 1) * self.in_size])
            if y is None:
                break
            outs.append(y)
            errs += err != 0
        return np.concatenate(outs), errs
