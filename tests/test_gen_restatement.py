"""What the restatement of WDSP's signal generator (tests/wdsp_gen_ref.py, wdsp/gen.c:29-354) does, pinned on the CPU: the tone's frequency
and magnitude, the sweep's reset periods as the reference's own addition chain gives them (a closed form is one sample off at the
defaults), the pulse's segment lengths and flush_gen's quirk, and the distribution of this project's noise generator at its default
seed."""
import numpy as np
import pytest

from wdsp_gen_ref import Gen, default_seed, noise, sweep_period

RATE = 48000


@pytest.mark.parametrize("freq,mag", [(700.0, 0.5), (-1250.0, 0.25)])
def test_tone_frequency_and_magnitude(freq, mag):
    """WDSP's +f is exp(-j 2 pi f t) of I + jQ (Q negated, gen.c:187-188)"""
    g = Gen(RATE, 256, run=1, mode=0)
    g.SetToneMag(mag); g.SetToneFreq(freq)
    n = 4800                                                    # 10 Hz bins: both frequencies sit on one
    z = g.blocks(19)[:n]
    spec = np.fft.fft(z) / n
    k = int(np.argmax(np.abs(spec)))
    assert np.fft.fftfreq(n, 1.0 / RATE)[k] == -freq
    assert abs(abs(spec[k]) - mag) < 1e-12
    assert np.abs(np.abs(z) - mag).max() < 1e-12
    assert z[0] == complex(mag, -0.0)
    g.SetToneFreq(freq)                                         # calc_tone: the phase goes to 0
    assert g.tone_phs == 0.0 and g.block()[0] == complex(mag, -0.0)


def test_two_tone_defaults():
    g = Gen(RATE, 4800, run=1, mode=1)
    spec = np.fft.fft(g.block()) / 4800
    f = np.fft.fftfreq(4800, 1.0 / RATE)
    top = np.argsort(np.abs(spec))[-2:]
    assert sorted(f[top]) == [-1700.0, -900.0]
    assert np.allclose(np.abs(spec[top]), 0.5, atol=1e-12)


@pytest.mark.parametrize("f1,f2,rate,want", [(-2000.0, 2000.0, 400000.0, 481), (-1000.0, 3000.0, 250000.0, 769), (-2000.0, 2001.7, 400000.0, 481),
                                             (-20000.0, 20000.0, 4000.0, 480000)])
def test_sweep_reset_periods(f1, f2, rate, want):
    """the samples at which dphs is back at its start in the literal xgen, three periods in a row (two at the defaults), and the chain
    walked alone"""
    assert sweep_period(RATE, f1, f2, rate) == want
    g = Gen(RATE, want - 1, run=1, mode=3)
    g.SetSweepFreq(f1, f2); g.SetSweepRate(rate)
    start = g.sweep_dphs
    for _ in range(3 if want < 1000 else 2):
        g.size = want - 1
        g.block()
        assert g.sweep_dphs > start and g.sweep_dphs <= g.sweep_dphsmax        # (the chain only rises: no reset so far)
        g.size = 1
        g.block()
        assert g.sweep_dphs == start                                            # sample `want` of the period resets it


def test_sweep_that_never_resets_and_one_that_always_does():
    assert sweep_period(RATE, 0.0, 1000.0, -5000.0) == 0
    assert sweep_period(RATE, 1000.0, 0.0, 5000.0) == 1
    g = Gen(RATE, 64, run=1, mode=3)
    g.SetSweepFreq(1000.0, 0.0); g.SetSweepRate(5000.0)          # f2 < f1: every sample resets, a tone at f1
    z = g.blocks(4)
    t = Gen(RATE, 64, run=1, mode=0)
    t.SetToneFreq(1000.0)
    assert np.abs(z - t.blocks(4)).max() < 1e-12


def test_pulse_segments_at_48k():
    g = Gen(RATE, 4096, run=1, mode=6)
    assert (g.pntrans, g.pnon, g.pnoff) == (96, 48000, 143808)
    period = g.pnoff + 2 * g.pntrans + g.pnon
    assert period == 4 * RATE
    z = g.blocks((2 * period + 4095) // 4096)
    assert np.all(z.imag == 0.0)
    for k in range(2):
        p = z[k * period:(k + 1) * period].real
        assert np.all(p[:g.pnoff] == 0.0)                       # OFF, pnoff samples the first time too (pcount starts at pnoff)
        on = p[g.pnoff + g.pntrans:g.pnoff + g.pntrans + g.pnon]
        t = np.arange(k * period + g.pnoff + g.pntrans, k * period + g.pnoff + g.pntrans + g.pnon)
        assert np.abs(on - np.cos(2.0 * np.pi * ((1000.0 * t / RATE) % 1.0))).max() < 1e-9
        up = p[g.pnoff:g.pnoff + g.pntrans]
        assert up[0] == 0.0 and abs(up).max() < 1.0             # ctrans[0] = 0 opens the edge
    assert g.ctrans[0] == 0.0 and abs(g.ctrans[96] - 1.0) < 1e-12


def test_flush_gen_goes_to_off_with_the_count_left_over():
    """flush_gen (gen.c:160-163) in the middle of ON: OFF then lasts what ON had left, not pnoff"""
    g = Gen(RATE, 1000, run=1, mode=6)
    into_on = 5000
    g.size = g.pnoff + g.pntrans + into_on
    g.block()
    assert g.pstate == 2 and g.pcount == g.pnon - into_on
    left = g.pcount
    g.flush()
    assert g.pstate == 0 and g.pcount == left
    g.size = left + g.pntrans + 10
    z = g.block().real
    assert np.all(z[:left] == 0.0) and z[left] == 0.0 and z[left + 1] != 0.0          # UP starts behind `left` samples of silence
    assert g.pstate == 2


def test_noise_stream_does_not_depend_on_the_cuts_and_differs_by_channel_and_seed():
    a = noise(default_seed(0), 0, 0, 2048, 1.0)
    b = np.concatenate([noise(default_seed(0), 0, s, 256, 1.0) for s in range(0, 2048, 256)])
    assert np.array_equal(a, b)
    assert not np.array_equal(a, noise(default_seed(1), 1, 0, 2048, 1.0))
    assert not np.array_equal(a, noise(default_seed(0), 1, 0, 2048, 1.0))
    assert not np.array_equal(a, noise(12345, 0, 0, 2048, 1.0))


@pytest.mark.parametrize("ch", [0, 1, 2, 3])
def test_noise_distribution_at_the_default_seed(ch):
    """N = 65536 samples per component at mag 0.25; five standard errors of each statistic under the reference's distribution (unit
    normal components times mag): mean mag / sqrt(N), variance mag^2 sqrt(2 / N), correlations 1 / sqrt(N)"""
    N, mag = 65536, 0.25
    z = noise(default_seed(ch), ch, 0, N, mag)
    for x in (z.real, z.imag):
        assert abs(x.mean()) <= 5.0 * mag / np.sqrt(N)
        assert abs(x.var() / mag ** 2 - 1.0) <= 5.0 * np.sqrt(2.0 / N)
        u = (x - x.mean()) / x.std()
        for lag in range(1, 9):
            assert abs(np.mean(u[:-lag] * u[lag:])) <= 5.0 / np.sqrt(N), lag
    assert abs(np.corrcoef(z.real, z.imag)[0, 1]) <= 5.0 / np.sqrt(N)
