"""The restatement of xcbl / xspeak / xmpeak (tests/rxa_audio_peak_ref.py) against closed forms.  CPU only."""
import math

import numpy as np
from scipy.signal import freqz

from rxa_audio_peak_ref import AudioPeakChain, Cbl, Mpeak, Speak, speak_design

RATE = 48000.0


def _h(b, a, f, rate=RATE):
    _, h = freqz(b, a, worN=[2 * math.pi * f / rate])
    return h[0]


def test_speak_design1_gain_at_f_and_dc():
    for f, bw, gain in ((600.0, 100.0, 2.0), (800.0, 50.0, 1.5), (2125.0, 75.0, 1.0)):
        b, a, fgain, _ = speak_design(f, bw, gain, RATE)
        # four stages, each A^2 = 6.25 at f (the RBJ peaking form), times fgain = gain / 6.25^4
        assert abs(abs(fgain * _h(b, a, f) ** 4) - gain) < 1e-9 * gain
        assert abs(abs(fgain * _h(b, a, 0.0) ** 4) - gain / 2.5 ** 8) < 1e-12
        assert abs(fgain - gain / 2.5 ** 8) < 1e-18


def test_speak_f_below_200_is_200():
    lo, at = speak_design(150.0, 50.0, 2.0, RATE), speak_design(200.0, 50.0, 2.0, RATE)
    assert lo[3] == 200.0
    assert np.array_equal(lo[0], at[0]) and np.array_equal(lo[1], at[1]) and lo[2] == at[2]
    s = Speak(RATE, f=150.0)
    assert s.f == 200.0


def test_speak_runs_per_component_with_state_carried():
    rng = np.random.default_rng(1)
    z = rng.standard_normal(3000) + 1j * rng.standard_normal(3000)
    s1, s2 = Speak(RATE, run=1), Speak(RATE, run=1)
    whole = s1.process(z)
    parts = np.concatenate([s2.process(z[:7]), s2.process(z[7:1000]), s2.process(z[1000:])])
    assert np.max(np.abs(whole - parts)) < 1e-15
    # I and Q see the same real filter
    re = Speak(RATE, run=1).process(z.real.astype(np.complex128))
    assert np.max(np.abs(whole.real - re.real)) < 1e-15


def test_cbl_blocks_dc_and_mtau():
    c = Cbl(RATE, run=1)
    assert c.mtau == math.exp(-1.0 / (RATE * 0.02))
    y = c.process(np.full(48000, 1.0 + 2.0j))
    assert abs(y[0] - (1.0 + 2.0j)) == 0.0
    assert abs(y[1] - c.mtau * (1.0 + 2.0j)) < 1e-15        # y1 = x1 - x0 + mtau y0
    assert np.abs(y[-1]) < 1e-20
    # the stored output under 1e-100 is zero: a long run of zeros after it leaves exact zeros behind
    y2 = c.process(np.zeros(300000, dtype=np.complex128))
    assert y2[-1] == 0.0 and c.prev_out == [0.0, 0.0]


def test_mpeak_is_the_sum_of_its_peaks():
    rng = np.random.default_rng(2)
    z = rng.standard_normal(4000) + 1j * rng.standard_normal(4000)
    m = Mpeak(RATE, run=1)
    p0, p1 = Speak(RATE, 2125.0, 75.0, 1.0, run=1), Speak(RATE, 2295.0, 75.0, 1.0, run=1)
    y = m.process(z)
    assert np.max(np.abs(y - (p0.process(z) + p1.process(z)))) < 1e-15
    m.enable = [0, 0]
    assert np.array_equal(m.process(z), np.zeros_like(z))
    m.enable, m.npeaks = [1, 1], 0
    assert np.array_equal(m.process(z), np.zeros_like(z))


def test_chain_order_and_flushing_setters():
    rng = np.random.default_rng(3)
    z = rng.standard_normal(2000) + 1j * rng.standard_normal(2000)
    ch = AudioPeakChain(RATE)
    assert np.array_equal(ch.process(z), z)                    # create_rxa: all three off
    ch.SetRXACBLRun(1); ch.SetRXASPCWRun(1); ch.SetRXAmpeakRun(1)
    c, s, m = Cbl(RATE, run=1), Speak(RATE, run=1), Mpeak(RATE, run=1)
    assert np.max(np.abs(ch.process(z) - m.process(s.process(c.process(z))))) < 1e-15
    ch.SetRXAmpeakFilBw(1, 120.0)
    assert np.all(ch.mpeak.pfil[1].zi == 0) and np.any(ch.mpeak.pfil[0].zi != 0)
    ch.SetRXASPCWGain(1.0)
    assert np.all(ch.speak.zi == 0)
