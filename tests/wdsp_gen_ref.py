"""A literal, sample-by-sample restatement of WDSP's signal generator as RXA's gen0 runs it (wdsp/gen.c:29-354, created by RXA.c:60-66
with run 0 and mode 2): xgen's modes 0 (tone), 1 (two-tone), 3 (sweep), 6 (pulse) and "any other" (silence), the calc_* functions, the
eight SetRXAPreGen* setters and flush_gen, with the reference's own additions, comparisons and wraps in the reference's order.  Modes 4
and 5 (sawtooth, triangle) are not restated: the engine refuses them.

Mode 2 is NOT the reference's (Marsaglia's polar method on rand(), seeded by the clock, one generator for the whole process): `noise`
restates this project's generator, the same polar method on a counter-based uniform source.

Test infrastructure only; plain Python floats are IEEE doubles, so the sums round as the reference's do."""
import math

import numpy as np

TWOPI = 6.2831853071795864          # comm.h
PI = 3.1415926535897932
OFF, UP, ON, DOWN = 0, 1, 2, 3      # enum pstate, gen.c:165-171
MASK = (1 << 64) - 1
GOLDEN = 0x9E3779B97F4A7C15
NOISE_MAX_ATTEMPTS = 64


class Gen:
    def __init__(self, rate, size, run=0, mode=2):
        """create_gen (gen.c:113-152) as create_rxa calls it (RXA.c:60-66)"""
        self.run, self.size, self.rate, self.mode = run, size, float(rate), mode
        self.tone_mag, self.tone_freq = 1.0, 1000.0
        self.tt_mag1, self.tt_mag2, self.tt_f1, self.tt_f2 = 0.5, 0.5, 900.0, 1700.0
        self.noise_mag = 1.0
        self.sweep_mag, self.sweep_f1, self.sweep_f2, self.sweep_rate = 1.0, -20000.0, 20000.0, 4000.0
        self.pulse_mag, self.pulse_pf, self.pulse_duty, self.pulse_trans, self.pulse_tf = 1.0, 0.25, 0.25, 0.002, 1000.0
        self.calc_tone(); self.calc_tt(); self.calc_sweep(); self.calc_pulse()

    # ---- gen.c:29-96
    def calc_tone(self):
        self.tone_phs = 0.0
        self.tone_delta = TWOPI * self.tone_freq / self.rate
        self.tone_cosdelta, self.tone_sindelta = math.cos(self.tone_delta), math.sin(self.tone_delta)

    def calc_tt(self):
        self.tt_phs1 = self.tt_phs2 = 0.0
        self.tt_delta1, self.tt_delta2 = TWOPI * self.tt_f1 / self.rate, TWOPI * self.tt_f2 / self.rate
        self.tt_cos1, self.tt_cos2 = math.cos(self.tt_delta1), math.cos(self.tt_delta2)
        self.tt_sin1, self.tt_sin2 = math.sin(self.tt_delta1), math.sin(self.tt_delta2)

    def calc_sweep(self):
        self.sweep_phs = 0.0
        self.sweep_dphs = TWOPI * self.sweep_f1 / self.rate
        self.sweep_d2phs = TWOPI * self.sweep_rate / (self.rate * self.rate)
        self.sweep_dphsmax = TWOPI * self.sweep_f2 / self.rate

    def calc_pulse(self):
        self.pulse_pperiod = 1.0 / self.pulse_pf
        self.pulse_tphs = 0.0
        self.pulse_tdelta = TWOPI * self.pulse_tf / self.rate
        self.pulse_tcos, self.pulse_tsin = math.cos(self.pulse_tdelta), math.sin(self.pulse_tdelta)
        self.pntrans = int(self.pulse_trans * self.rate)
        self.pnon = int(self.pulse_duty * self.pulse_pperiod * self.rate)
        self.pnoff = int(self.pulse_pperiod * self.rate) - self.pnon - 2 * self.pntrans
        if self.pnoff < 0:
            self.pnoff = 0
        self.pcount = self.pnoff
        self.pstate = OFF
        delta, theta = PI / float(self.pntrans), 0.0
        self.ctrans = []
        for _ in range(self.pntrans + 1):
            self.ctrans.append(0.5 * (1.0 - math.cos(theta)))
            theta += delta

    def flush(self):
        """flush_gen (gen.c:160-163): the state goes to OFF and pcount stays as it was"""
        self.pstate = OFF

    # ---- the setters, gen.c:384-450
    def SetRun(self, run): self.run = run
    def SetMode(self, mode): self.mode = mode
    def SetToneMag(self, mag): self.tone_mag = mag
    def SetToneFreq(self, freq): self.tone_freq = freq; self.calc_tone()
    def SetNoiseMag(self, mag): self.noise_mag = mag
    def SetSweepMag(self, mag): self.sweep_mag = mag
    def SetSweepFreq(self, f1, f2): self.sweep_f1, self.sweep_f2 = f1, f2; self.calc_sweep()
    def SetSweepRate(self, rate): self.sweep_rate = rate; self.calc_sweep()

    # ---- xgen, gen.c:173-354, one block of `size` samples; None when the generator does not run (in == out: the buffer is left alone)
    def block(self):
        if not self.run:
            return None
        n = self.size
        out = np.zeros(n, dtype=np.complex128)
        if self.mode == 0:
            c, s = math.cos(self.tone_phs), math.sin(self.tone_phs)
            for i in range(n):
                out[i] = complex(self.tone_mag * c, -self.tone_mag * s)
                t1, t2 = c, s
                c = t1 * self.tone_cosdelta - t2 * self.tone_sindelta
                s = t1 * self.tone_sindelta + t2 * self.tone_cosdelta
                self.tone_phs += self.tone_delta
                if self.tone_phs >= TWOPI: self.tone_phs -= TWOPI
                if self.tone_phs < 0.0: self.tone_phs += TWOPI
        elif self.mode == 1:
            c1, s1 = math.cos(self.tt_phs1), math.sin(self.tt_phs1)
            c2, s2 = math.cos(self.tt_phs2), math.sin(self.tt_phs2)
            for i in range(n):
                out[i] = complex(self.tt_mag1 * c1 + self.tt_mag2 * c2, -self.tt_mag1 * s1 - self.tt_mag2 * s2)
                tc, ts = c1, s1
                c1 = tc * self.tt_cos1 - ts * self.tt_sin1
                s1 = tc * self.tt_sin1 + ts * self.tt_cos1
                self.tt_phs1 += self.tt_delta1
                if self.tt_phs1 >= TWOPI: self.tt_phs1 -= TWOPI
                if self.tt_phs1 < 0.0: self.tt_phs1 += TWOPI
                tc, ts = c2, s2
                c2 = tc * self.tt_cos2 - ts * self.tt_sin2
                s2 = tc * self.tt_sin2 + ts * self.tt_cos2
                self.tt_phs2 += self.tt_delta2
                if self.tt_phs2 >= TWOPI: self.tt_phs2 -= TWOPI
                if self.tt_phs2 < 0.0: self.tt_phs2 += TWOPI
        elif self.mode == 2:
            raise NotImplementedError("mode 2 draws on rand(): see `noise` for this project's generator")
        elif self.mode == 3:
            dphs0 = TWOPI * self.sweep_f1 / self.rate
            for i in range(n):
                out[i] = complex(self.sweep_mag * math.cos(self.sweep_phs), -self.sweep_mag * math.sin(self.sweep_phs))
                self.sweep_phs += self.sweep_dphs
                self.sweep_dphs += self.sweep_d2phs
                if self.sweep_phs >= TWOPI: self.sweep_phs -= TWOPI
                if self.sweep_phs < 0.0: self.sweep_phs += TWOPI
                if self.sweep_dphs > self.sweep_dphsmax:
                    self.sweep_dphs = dphs0
        elif self.mode in (4, 5):
            raise NotImplementedError("sawtooth and triangle are refused by the engine (DESIGN.md b20)")
        elif self.mode == 6:
            c, s = math.cos(self.pulse_tphs), math.sin(self.pulse_tphs)
            for i in range(n):
                v = 0.0
                if self.pnoff != 0:
                    if self.pstate == OFF:
                        v = 0.0
                        self.pcount -= 1
                        if self.pcount == 0: self.pstate, self.pcount = UP, self.pntrans
                    elif self.pstate == UP:
                        v = self.pulse_mag * c * self.ctrans[self.pntrans - self.pcount]
                        self.pcount -= 1
                        if self.pcount == 0: self.pstate, self.pcount = ON, self.pnon
                    elif self.pstate == ON:
                        v = self.pulse_mag * c
                        self.pcount -= 1
                        if self.pcount == 0: self.pstate, self.pcount = DOWN, self.pntrans
                    else:
                        v = self.pulse_mag * c * self.ctrans[self.pcount]
                        self.pcount -= 1
                        if self.pcount == 0: self.pstate, self.pcount = OFF, self.pnoff
                out[i] = complex(v, 0.0)
                t1, t2 = c, s
                c = t1 * self.pulse_tcos - t2 * self.pulse_tsin
                s = t1 * self.pulse_tsin + t2 * self.pulse_tcos
                self.pulse_tphs += self.pulse_tdelta
                if self.pulse_tphs >= TWOPI: self.pulse_tphs -= TWOPI
                if self.pulse_tphs < 0.0: self.pulse_tphs += TWOPI
        return out

    def blocks(self, nblk):
        return np.concatenate([self.block() for _ in range(nblk)])


def sweep_period(rate, f1, f2, sweeprate, limit=None):
    """Samples from a reset of the sweep to the next, by the reference's own chain: dphs starts at TWOPI * f1 / rate, `dphs += d2phs` once
    a sample, and the sample whose sum exceeds dphsmax resets it (gen.c:253-258).  1 where the start already exceeds dphsmax (every sample
    resets), 0 where the chain never gets there (d2phs <= 0)."""
    rate = float(rate)
    dphs = TWOPI * f1 / rate
    d2phs = TWOPI * sweeprate / (rate * rate)
    dphsmax = TWOPI * f2 / rate
    if dphs > dphsmax:
        return 1
    if d2phs <= 0.0:
        return 0
    n = 0
    while True:
        dphs += d2phs
        n += 1
        if dphs > dphsmax:
            return n
        if limit is not None and n >= limit:
            return 0


# ---- this project's noise generator (quisk_amd/csrc/qh_gen.hpp)
def default_seed(ch):
    return (GOLDEN * (ch + 1)) & MASK


def _mix64(z):
    """splitmix64's finalizer on uint64 arrays"""
    z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
    z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
    return z ^ (z >> np.uint64(31))


def noise(seed, ch, start, n, mag):
    """Samples start .. start + n - 1 of channel ch's noise stream: the polar method of gen.c:232-243 with r = 2 u - 1, u = the top 53 bits
    of a 64-bit word times 2^-53.  The words of sample k's attempt a are mix64(K + GOLDEN (2 a + 1)) and mix64(K + GOLDEN (2 a + 2)),
    K = mix64(mix64(seed + GOLDEN (ch + 1)) + GOLDEN k): every sample draws for itself.  c >= 1 is rejected as in the reference, and so
    is c == 0; r1 r1 + r2 r2 is two products and a sum, each rounded."""
    with np.errstate(over="ignore"):
        g = np.uint64(GOLDEN)
        key = _mix64(np.array([(seed + GOLDEN * (ch + 1)) & MASK], dtype=np.uint64))[0]
        K = _mix64(key + g * (np.uint64(start) + np.arange(n, dtype=np.uint64)))
        out = np.zeros(n, dtype=np.complex128)
        todo = np.arange(n)
        for a in range(NOISE_MAX_ATTEMPTS):
            if not todo.size:
                break
            k = K[todo]
            w1 = _mix64(k + g * np.uint64(2 * a + 1))
            w2 = _mix64(k + g * np.uint64(2 * a + 2))
            r1 = 2.0 * ((w1 >> np.uint64(11)).astype(np.float64) * 2.0 ** -53) - 1.0
            r2 = 2.0 * ((w2 >> np.uint64(11)).astype(np.float64) * 2.0 ** -53) - 1.0
            c = r1 * r1 + r2 * r2
            ok = (c < 1.0) & (c != 0.0)
            co = c[ok]
            rad = np.sqrt(-2.0 * np.log(co) / co)
            out[todo[ok]] = (mag * rad * r1[ok]) + 1j * (mag * rad * r2[ok])
            todo = todo[~ok]
    return out
