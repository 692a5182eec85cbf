"""Restatement of WDSP's FM squelch (xfmsq) and of what feeds it, for the tests.

Written from the reference's semantics, not from the HIP code: eq_impulse (wdsp/eq.c:39-158) through fir_fsamp (wdsp/fir.c:127-185) and
the loop of xfmd that makes the trigger (wdsp/fmd.c:151-172); calc_fmsq / flush_fmsq / xfmsq and the setters
(wdsp/fmsq.c) with create_rxa's arguments (RXA.c:214-234).  The noise filter is a direct convolution over a persistent delay line; the
averages, the ready delay and the state machine are stepped sample by sample as written.  `Fmsq.process(trigger, insig)` returns the
squelched block and leaves the per-sample gain, avnoise and the real values of the tail counts of that block in `gain`, `av`, `tails`.
"""
import math

import numpy as np

PI = 3.1415926535897932           # wdsp/comm.h
TWOPI = 6.2831853071795864
MUTED, INCREASE, UNMUTED, TAIL, DECREASE = range(5)


def fsamp_window(N, wintype):
    """get_fsamp_window (fir.c:44-81): 4-term (0) or 7-term (1) Blackman-Harris, else none"""
    arg0 = 2.0 * PI / (N - 1.0)
    c = np.cos(arg0 * np.arange(N))
    if wintype == 0:
        return 0.21747 + c * (-0.45325 + c * (0.28256 + c * (-0.04672)))
    if wintype == 1:
        return (6.3964424114390378e-02 + c * (-2.3993864599352804e-01 + c * (3.5015956323820469e-01 + c * (-2.4774111897080783e-01
                + c * (8.5438256055858031e-02 + c * (-1.2320203369293225e-02 + c * (4.3778825791773474e-04)))))))
    return np.ones(N)


def fir_fsamp(N, A, scale, wintype):
    """fir_fsamp, even N, rtype 1 (fir.c:151-181): real taps"""
    assert N % 2 == 0
    M = (N - 1) / 2.0
    n = np.arange(N // 2)[:, None]
    k = np.arange(1, N // 2)[None, :]
    s = np.sum(2.0 * np.asarray(A)[1:N // 2][None, :] * np.cos(TWOPI * (n - M) * k / N), axis=1)
    half = (1.0 / N) * (A[0] + s)
    h = np.concatenate([half, half[::-1]])
    return h * (scale * fsamp_window(N, wintype))


def eq_impulse(N, nfreqs, F, G, samplerate, scale, ctfmode, wintype):
    """eq.c:39-158 for even N"""
    assert N % 2 == 0
    fp = [0.0] * (nfreqs + 2)
    gp = [0.0] * (nfreqs + 2)
    fp[nfreqs + 1] = 1.0
    gpreamp = G[0]
    pairs = []
    for i in range(1, nfreqs + 1):
        f = 2.0 * F[i] / samplerate
        f = 0.0 if f < 0.0 else 1.0 if f > 1.0 else f
        pairs.append((f, G[i]))
    pairs.sort(key=lambda p: p[0])
    for i in range(1, nfreqs + 1):
        fp[i], gp[i] = pairs[i - 1]
    gp[0] = gp[1]
    gp[nfreqs + 1] = gp[nfreqs]
    mid = N // 2
    A = [0.0] * (mid + 1)
    j = 0
    for i in range(mid):
        f = (i + 0.5) / mid
        while f > fp[j + 1]:
            j += 1
        frac = (f - fp[j]) / (fp[j + 1] - fp[j])
        A[i] = math.pow(10.0, 0.05 * (frac * gp[j + 1] + (1.0 - frac) * gp[j] + gpreamp)) * scale
    if ctfmode == 0:
        low = int(fp[1] * mid - 0.5)
        high = int(fp[nfreqs] * mid - 0.5)
        lowmag, highmag = A[low], A[high]
        flow4 = math.pow(low / mid, 4.0)
        fhigh4 = math.pow(high / mid, 4.0)
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
    return fir_fsamp(N, np.array(A), 1.0, wintype)


def pllpole(zeta=1.0, omegaN=20000.0):
    """fmd.c:39"""
    return omegaN * math.sqrt(2.0 * zeta * zeta + 1.0 + math.sqrt((2.0 * zeta * zeta + 1.0) * (2.0 * zeta * zeta + 1.0) + 1)) / TWOPI


def fmsq_impulse(nc, rate, size):
    """calc_fmsq's noise filter (fmsq.c:36-46) with mp 0, as create_fircore keeps it: the 1 / (2 size) of the design undone"""
    pp = pllpole()
    F = [0.0, 5000.0, pp, 20000.0]
    G = [0.0, 0.0, 3.0, +20.0 * math.log10(20000.0 / pp)]
    return eq_impulse(nc, 3, F, G, float(rate), 1.0 / (2.0 * size), 0, 0) * (2.0 * size)


class FmLoop:
    """the loop, dc removal and gain of xfmd (fmd.c:151-172) with create_rxa's constants (RXA.c:197-205): complex in, audio out"""

    def __init__(self, rate, deviation=5000.0):
        zeta, omegaN, tau = 1.0, 20000.0, 0.02
        self.omega_min = TWOPI * -8000.0 / rate
        self.omega_max = TWOPI * 8000.0 / rate
        self.g1 = 1.0 - math.exp(-2.0 * omegaN * zeta / rate)
        self.g2 = -self.g1 + 2.0 * (1 - math.exp(-omegaN * zeta / rate) * math.cos(omegaN / rate * math.sqrt(1.0 - zeta * zeta)))
        self.mtau = math.exp(-1.0 / (rate * tau))
        self.onem_mtau = 1.0 - self.mtau
        self.again = rate / (deviation * TWOPI)
        self.flush()

    def flush(self):
        self.phs = self.fil_out = self.omega = self.fmdc = 0.0

    def process(self, z):
        out = np.empty(len(z))
        phs, fil_out, omega, fmdc = self.phs, self.fil_out, self.omega, self.fmdc
        g1, g2, lo, hi, mtau, om, again = self.g1, self.g2, self.omega_min, self.omega_max, self.mtau, self.onem_mtau, self.again
        cos, sin, atan2 = math.cos, math.sin, math.atan2
        for i, (re, im) in enumerate(zip(z.real.tolist(), z.imag.tolist())):
            v0, v1 = cos(phs), sin(phs)
            c0 = re * v0 + im * v1
            c1 = -re * v1 + im * v0
            if c0 == 0.0 and c1 == 0.0:
                c0 = 1.0
            det = atan2(c1, c0)
            del_out = fil_out
            omega += g2 * det
            if omega < lo:
                omega = lo
            if omega > hi:
                omega = hi
            fil_out = g1 * det + omega
            phs += del_out
            while phs >= TWOPI:
                phs -= TWOPI
            while phs < 0.0:
                phs += TWOPI
            fmdc = mtau * fmdc + om * fil_out
            out[i] = again * (fil_out - fmdc)
        self.phs, self.fil_out, self.omega, self.fmdc = phs, fil_out, omega, fmdc
        return out


def ready_count(rate, tdelay=0.100):
    """the samples xfmsq takes to set `ready` (fmsq.c:153-154): ramp += rstep until ramp >= tdelay, counted as made"""
    rstep, ramp, n = 1.0 / rate, 0.0, 0
    while True:
        ramp += rstep
        n += 1
        if ramp >= tdelay:
            return n


class Fmsq:
    """one xfmsq instance as create_rxa makes it (RXA.c:214-234)"""

    def __init__(self, rate, size=256, run=0, nc=2048, mp=0, tup=0.050, tdown=0.010, ntup=None, ntdown=None, taps=None):
        # taps: the noise filter as the caller has it (create_fircore's form, the 1 / (2 size) undone) instead of this file's design;
        # needed with mp 1.  mp_imp (fir.c:319-368) takes the logarithm of a stop band that eq_impulse's skirts put at 1e-100 and the
        # transforms' rounding at 1e-17, so a minimum-phase design of this filter is decided by the rounding of whichever FFT made it: a
        # restatement with numpy's transforms left taps 3 % (2048) to 30 % (256) from the library's host transform, and the reference's
        # FFTW would leave a third set.  No restatement of mp_imp is kept here for that reason.
        self.taps = taps
        self.rate = float(rate)
        self.size = size
        self.run = run
        self.fc, self.tdelay, self.avtau, self.longtau = 5000.0, 0.100, 0.001, 0.100
        self.tail_thresh, self.unmute_thresh, self.min_tail, self.max_tail = 0.750, 0.562, 0.000, 1.200
        self.nc, self.mp = nc, mp
        # calc_fmsq (fmsq.c:29-78)
        self._design()
        self.delay = np.zeros(self.nc - 1)
        self.avm = math.exp(-1.0 / (self.rate * self.avtau))
        self.onem_avm = 1.0 - self.avm
        self.avnoise = 100.0
        self.longavm = math.exp(-1.0 / (self.rate * self.longtau))
        self.onem_longavm = 1.0 - self.longavm
        self.longnoise = 1.0
        self.ntup = int(tup * self.rate) if ntup is None else ntup          # (tiny tables for the hand-made cases)
        self.ntdown = int(tdown * self.rate) if ntdown is None else ntdown
        self.cup, self.cdown = [], []
        delta, theta = PI / self.ntup, 0.0
        for _ in range(self.ntup + 1):
            self.cup.append(0.5 * (1.0 - math.cos(theta)))
            theta += delta
        delta, theta = PI / self.ntdown, 0.0
        for _ in range(self.ntdown + 1):
            self.cdown.append(0.5 * (1 + math.cos(theta)))
            theta += delta
        self.state, self.count = MUTED, 0
        self.ready, self.ramp, self.rstep = 0, 0.0, 1.0 / self.rate
        self.gain, self.av, self.tails = np.zeros(0), np.zeros(0), []

    def _design(self):
        assert self.taps is not None or not self.mp, "a minimum-phase case brings its taps"
        self.h = fmsq_impulse(self.nc, self.rate, self.size) if self.taps is None else np.asarray(self.taps)
        assert len(self.h) == self.nc

    def flush(self):
        """flush_fmsq (fmsq.c:122-130); the count is not touched"""
        self.delay[:] = 0.0
        self.avnoise, self.longnoise = 100.0, 1.0
        self.state, self.ready, self.ramp = MUTED, 0, 0.0

    # the setters (fmsq.c:235-279)
    def SetRXAFMSQRun(self, run):
        self.run = run

    def SetRXAFMSQThreshold(self, threshold):
        self.tail_thresh = threshold
        self.unmute_thresh = 0.9 * threshold

    def SetRXAFMSQNC(self, nc):
        if self.nc != nc:
            self.nc = nc
            self._design()
            self.delay = np.zeros(nc - 1)            # setNc_fircore zeroes the delay line (firmin.c:454-466)

    def SetRXAFMSQMP(self, mp):
        if self.mp != mp:
            self.mp = mp
            self._design()

    def noise_filter(self, trigger):
        """xfircore over the trigger (I = Q): the two components of the filter's output"""
        x = np.concatenate([self.delay, trigger])
        self.delay = x[len(x) - (self.nc - 1):].copy()
        y = np.convolve(x, self.h, mode="valid")      # real trigger, complex taps when mp
        # (I, Q) of a complex filter on the complex signal (t, t): (1 + j) t * h
        z = (1.0 + 1.0j) * y
        return z.real, z.imag

    def process(self, trigger, insig):
        insig = np.asarray(insig, dtype=np.complex128)
        n = len(insig)
        if not self.run:
            self.gain, self.av, self.tails = np.ones(n), np.zeros(0), []
            return insig.copy()
        n0, n1 = self.noise_filter(np.asarray(trigger, dtype=np.float64))
        noise = np.sqrt(n0 * n0 + n1 * n1).tolist()
        g, av, tails = np.empty(n), np.empty(n), []
        avnoise, longnoise, state, count, ready, ramp = self.avnoise, self.longnoise, self.state, self.count, self.ready, self.ramp
        avm, om, lavm, lom = self.avm, self.onem_avm, self.longavm, self.onem_longavm
        for i in range(n):
            nz = noise[i]
            avnoise = avm * avnoise + om * nz
            longnoise = lavm * longnoise + lom * nz
            if not ready:
                ramp += self.rstep
            if ramp >= self.tdelay:
                ready = 1
            av[i] = avnoise
            if state == MUTED:
                if avnoise < self.unmute_thresh and ready:
                    state, count = INCREASE, self.ntup
                g[i] = 0.0
            elif state == INCREASE:
                g[i] = self.cup[self.ntup - count]
                if count == 0:
                    state = UNMUTED
                count -= 1
            elif state == UNMUTED:
                if avnoise > self.tail_thresh:
                    state = TAIL
                    lnlimit = 1.0 if longnoise > 1.0 else longnoise
                    real = (self.min_tail + (self.max_tail - self.min_tail) * lnlimit) * self.rate
                    tails.append(real)
                    count = int(real)
                g[i] = 1.0
            elif state == TAIL:
                g[i] = 1.0
                if avnoise < self.unmute_thresh:
                    state = UNMUTED
                elif count == 0:                        # count-- == 0: the decrement is overwritten
                    state, count = DECREASE, self.ntdown
                else:
                    count -= 1
            else:
                g[i] = self.cdown[self.ntdown - count]
                if count == 0:
                    state = MUTED
                count -= 1
        self.avnoise, self.longnoise, self.state, self.count, self.ready, self.ramp = avnoise, longnoise, state, count, ready, ramp
        self.gain, self.av, self.tails = g, av, tails
        out = np.empty_like(insig)
        out.real = insig.real * g
        out.imag = insig.imag * g
        out[g == 0.0] = 0.0                          # MUTED stores 0.0 (fmsq.c:164-165); cup[0] = 0 times a finite sample is 0 too
        return out


def margins(av, thresholds, tails):
    """(the smallest relative distance from a threshold of the samples on both sides of any crossing of it, the smallest distance of a
    tail count's real value from an integer): the figures the GPU comparison's state equality rests on"""
    av = np.asarray(av)
    worst = np.inf
    for th in thresholds:
        below = av < th
        x = np.flatnonzero(below[1:] != below[:-1])
        if x.size:
            worst = min(worst, float(np.min(np.abs(av[x] - th)) / th), float(np.min(np.abs(av[x + 1] - th)) / th))
    tail = min((abs(t - round(t)) for t in tails), default=np.inf)
    return worst, tail


def keyed_fm(n, rate, seed=3, amp=0.3, off=0.5, on=0.9, tone=1000.0, dev=3000.0, sigma=0.01, bw=8000.0, start_on=False):
    """the issue's recipe at baseband: a carrier of amplitude amp keyed off / on, a tone at +-dev deviation, complex noise of the given
    sigma band-limited to +-bw"""
    rng = np.random.default_rng(seed)
    t = np.arange(n) / rate
    ph = 2.0 * np.pi * np.cumsum(dev * np.sin(2.0 * np.pi * tone * t)) / rate
    phase_t = (t + (off if start_on else 0.0)) % (off + on)
    gate = phase_t >= off
    w = rng.standard_normal(n) + 1j * rng.standard_normal(n)
    W = np.fft.fft(w)
    W[np.abs(np.fft.fftfreq(n, 1.0 / rate)) > bw] = 0.0
    w = np.fft.ifft(W)
    w *= sigma / np.sqrt(np.mean(np.abs(w) ** 2) / 2.0)
    return amp * np.exp(1j * ph) * gate + w
