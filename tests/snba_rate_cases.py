"""Inputs and cases shared by the tests of xsnba at DSP rates of 96 to 384 kHz and blocks up to 4096 (test_gpu_snba_rates.py,
test_gpu_snba_forms.py, test_gpu_snba_rates_engine.py) and by the CPU test that vets those inputs (test_snba_rate_inputs.py).

`crackle` and `setup` are those of test_gpu_snba_parity.py at the engine's input rate: carriers with impulsive interference, so that
frames really get repaired.  About 0.8 s of signal per case, cut into ragged calls of (0..3, 3..4, 4..71, ...) blocks.

The blanker's detector compares against thresholds and its repair inverts a Toeplitz matrix, so the reference itself can turn a
last-bit change of its input into another set of repaired samples.  Every input here is one on which it does not
(test_snba_rate_inputs.py): where a (channel number, seed offset) of `crackle` failed that, another one stands in `chans`."""
import numpy as np

from quisk_amd import synth

USB, FM, AM, LSB, SAM = 1, 5, 6, 0, 10
SECONDS = 0.8


def crackle(c, n, mode=USB, fs=192000.0, rate=25.0):
    rng = np.random.default_rng(900 + c)
    t = np.arange(n) / fs
    f0 = -synth.shift_freq(c)
    sgn = 1.0 if mode == LSB else -1.0
    k = rng.integers(0, n, int(rate * n / fs))
    if mode in (AM, SAM):
        env = 1.0 + 0.5 * np.cos(2 * np.pi * 700.0 * t) + 0.3 * np.cos(2 * np.pi * 1900.0 * t)
        for w in range(24):
            env[np.minimum(k + w, n - 1)] += 1.0 + 2.0 * rng.random(k.size)
        x = 0.2 * env * np.exp(2j * np.pi * f0 * t)
    elif mode == FM:
        steps = np.zeros(n)
        sg = np.sign(rng.random(k.size) - 0.5)
        for w in range(48):
            steps[np.minimum(k + w, n - 1)] += sg * 0.8 / 48
        x = 0.2 * np.exp(2j * np.pi * f0 * t + 2j * (np.sin(2 * np.pi * 800.0 * t) + 0.5 * np.sin(2 * np.pi * 1500.0 * t)) + 1j * np.cumsum(steps))
    else:
        x = sum(a * np.exp(2j * np.pi * (f0 + sgn * f) * t) for a, f in ((0.08, 700.0), (0.05, 1210.0), (0.03, 2300.0)))
        x[k] += (2.0 + 6.0 * rng.random(k.size)) * np.exp(2j * np.pi * rng.random(k.size))
    return x + 0.01 * (rng.standard_normal(n) + 1j * rng.standard_normal(n))


def setup(t, a, ch, mode, size=256, snba_band=True):
    """t: an engine (a = (channel,)) or an oracle channel (a = ()).  ch: the `crackle` channel number, which places the carrier.
    snba_band False: RXASetPassband (RXA.c:926-932) without its SetRXASNBAOutputBandwidth, which leaves the blanker's output resampler
    at its creation bandwidth -- where calc_snba puts it when the DSP rate changes."""
    def passband(lo, hi):
        if snba_band: t.RXASetPassband(*a, lo, hi)
        else: t.SetRXABandpassFreqs(*a, lo, hi); t.RXANBPSetFreqs(*a, lo, hi)
    if size > 2048:
        t.RXASetNC(*a, size)                # 'size' must be <= 'nc' (wdsp/nbp.c:308)
    t.SetRXAShiftRun(*a, 1); t.SetRXAShiftFreq(*a, synth.shift_freq(ch)); t.RXANBPSetRun(*a, 1)
    t.SetRXAMode(*a, mode)
    if mode == LSB: passband(-3000.0, -300.0)
    elif mode in (AM, SAM, FM): passband(-4000.0, 4000.0)
    else: passband(300.0, 3000.0)
    t.SetRXAAGCMode(*a, 0); t.SetRXAAGCFixed(*a, 6.0)


class Case:
    """rates: (in_rate, dsp_rate, out_rate, dsp_size); modes: one per channel; chans: the `crackle` channel number of each"""

    def __init__(self, rates, modes, chans=None, seconds=SECONDS, extra_cuts=(), shift=True, snba_band=True):
        self.snba_band = snba_band
        self.shift = shift      # False: the carriers are brought to 0 Hz on the host and xshift stays off (no oscillator phase in the chain)
        self.in_rate, self.dsp_rate, self.out_rate, self.size = self.rates = rates
        self.modes = modes
        self.chans = tuple(chans) if chans is not None else tuple(range(len(modes)))
        self.nch = len(modes)
        self.insize = self.size * self.in_rate // self.dsp_rate
        self.outsize = self.size * self.out_rate // self.dsp_rate
        self.nblk = int(round(seconds * self.dsp_rate / self.size))
        self.extra_cuts = tuple(extra_cuts)

    def cuts(self):
        """ragged calls: blocks (0..3, 3..4, 4..71, 71..nblk), as far as the signal goes"""
        edges = [e for e in (0, 3, 4, 71) + self.extra_cuts if e < self.nblk] + [self.nblk]
        return list(zip(edges, edges[1:]))

    def reference(self, oracle, x, events=None, snba=1):
        """the oracle channels' xrxa over the ragged calls; events: {call index: fn(target, lead arguments, channel index)}, applied
        ahead of that call"""
        out = []
        for i in range(self.nch):
            o = self.oracle_channel(oracle, i, snba)
            ys = []
            for k, (a, b) in enumerate(self.cuts()):
                if events and k in events:
                    events[k](o, (), i)
                ys.append(o.xrxa(x[i, a * self.insize:b * self.insize]))
            out.append(np.concatenate(ys))
            o.close()
        return np.stack(out)

    def through(self, e, x, events=None):
        """the same through an engine"""
        ys = []
        for k, (a, b) in enumerate(self.cuts()):
            if events and k in events:
                for i in range(self.nch):
                    events[k](e, (i,), i)
            ys.append(e.process_host(x[:, a * self.insize:b * self.insize]))
        return np.concatenate(ys, axis=1)

    def inputs(self):
        x = np.stack([crackle(c, self.nblk * self.insize, m, fs=float(self.in_rate)) for c, m in zip(self.chans, self.modes)])
        if not self.shift:
            t = np.arange(x.shape[1]) / float(self.in_rate)
            x = x * np.stack([np.exp(2j * np.pi * synth.shift_freq(c) * t) for c in self.chans])
        return x

    def settings(self, t, a, i):
        setup(t, a, self.chans[i], self.modes[i], self.size, self.snba_band)
        if not self.shift:
            t.SetRXAShiftRun(*a, 0)

    def oracle_channel(self, oracle, i, snba=1):
        o = oracle.WdspChannel(self.insize, self.size, self.in_rate, self.dsp_rate, self.out_rate)
        self.settings(o, (), i)
        o.SetRXASNBARun(snba)
        return o

    def engine(self, qh, snba=1):
        e = qh.RxaEngine(self.nch, dsp_size=self.size, in_rate=self.in_rate, dsp_rate=self.dsp_rate, out_rate=self.out_rate)
        for i in range(self.nch):
            self.settings(e, (i,), i)
            e.SetRXASNBARun(i, snba)
        return e


# the cases of test_gpu_snba_rates.py, as (in, dsp, out, size) and the channels' modes
CASES = {
    "96k_256": Case((192000, 96000, 48000, 256), (USB, LSB, AM)),
    "96k_64": Case((96000, 96000, 96000, 64), (USB, AM)),
    "192k_512": Case((192000, 192000, 48000, 512), (USB, LSB)),
    # ratio 32: the longest window.  (LSB on `crackle` channel 2: channel 0's input is one the reference amplifies, 5.7e-7 against itself)
    "384k_1024": Case((384000, 384000, 48000, 1024), (LSB, AM), chans=(2, 1)),
    "48k_2048": Case((48000, 48000, 48000, 2048), (USB,)),             # the new block sizes
    "96k_4096": Case((96000, 96000, 96000, 4096), (USB,)),
}


def _bandwidth(t, a, i):
    """SetRXASNBAOutputBandwidth on channel 0 (the oracle reaches it through RXASetPassband, RXA.c:926-932: the engine gets that
    function's three calls one by one)"""
    if i != 0: return
    if a:
        t.SetRXABandpassFreqs(*a, 300.0, 2400.0); t.SetRXASNBAOutputBandwidth(*a, 300.0, 2400.0); t.RXANBPSetFreqs(*a, 300.0, 2400.0)
    else:
        t.RXASetPassband(300.0, 2400.0)


def _run(v):
    def ev(t, a, i):
        if i == 0: t.SetRXASNBARun(*a, v)
    return ev


# the two setter cases at 192 k with dsp_size 512, two channels: the events by call index (Case.cuts: calls 3 and 4 start at blocks 71 and 150)
SETTER_CASE = Case((192000, 192000, 48000, 512), (USB, LSB), extra_cuts=(150,))
SETTER_EVENTS = {"bandwidth": {3: _bandwidth}, "off_on": {3: _run(0), 4: _run(1)}}
# test_gpu_snba_rates_engine.py: the signal behind the rate change 48 k -> 96 k, and the WDSP names at 96000 / 256
# (`crackle` channel 1: on channel 0's half second the reference moves by 5.1e-6 under a 1e-12 perturbation)
# (without xshift: the engine's oscillator has run through the silence behind the change, a fresh channel's starts at phase 0)
# (and with the blanker's output resampler at its creation bandwidth, as setDSPSamplerate_rxa's calc_snba leaves it: DESIGN.md row b24)
AFTER_RATE_CHANGE = Case((96000, 96000, 48000, 64), (USB,), chans=(1,), seconds=0.5, shift=False, snba_band=False)
NAMES_CASE = Case((96000, 96000, 48000, 256), (USB,))
