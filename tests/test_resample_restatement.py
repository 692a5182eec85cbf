"""tests/wdsp_resample_ref.py, the sample-by-sample restatement of wdsp/resample.c that the GPU tests of qh_resample_* compare against,
held to what is known without it: the oracle's compiled xresample (bit for bit, on ragged calls), the sizes derived by hand from
resample.c:53-66 and 258-267, and the real-float form against the complex one run on the same taps.  CPU only."""
import numpy as np
import pytest

from wdsp_resample_ref import Resample, ResampleF, calc_resample, calc_resample_f, run_cuts

PAIRS = [(48000, 44100), (44100, 48000), (96000, 48000), (48000, 96000), (48000, 48000), (384000, 48000)]
# L, M, cpp by hand: gcd(48000, 44100) = 300 -> L 147, M 160; ncoef = (int)(140 * 48000 * 147 / 44100) = 22400 -> (22400 / 147 + 1) 147,
# cpp 153; 44.1 k -> 48 k: 140 * 44100 * 160 / 44100 = 22400 -> 22400 / 160 + 1 = 141; and so on
SIZES = {(48000, 44100): (147, 160, 153), (44100, 48000): (160, 147, 141), (96000, 48000): (1, 2, 281), (48000, 96000): (2, 1, 141),
         (48000, 48000): (1, 1, 141), (384000, 48000): (1, 8, 1121)}
N = 3000
CUTS = [0, 1, 2, 40, 139, 400, 400, 2300, N]


def _x(seed):
    rng = np.random.default_rng(seed)
    return rng.standard_normal(N) + 1j * rng.standard_normal(N)


@pytest.mark.parametrize("pair", PAIRS)
def test_complex_restatement_is_the_oracles_xresample(oracle, pair):
    x = _x(pair[0] // 100 + pair[1] // 1000)
    ref, orc = Resample(*pair), oracle.Resample(*pair)
    assert (ref.L, ref.M, ref.cpp) == SIZES[pair]
    taps, L, M, ncoef, cpp = oracle.resample_taps(*pair)
    assert (L, M, cpp) == SIZES[pair] and np.array_equal(taps, ref.h)
    total = 0
    for k, (a, b) in enumerate(zip(CUTS[:-1], CUTS[1:])):
        y, B = ref.process(x[a:b])
        want = orc(x[a:b])
        assert len(y) == len(want) == len(B), (pair, k)
        assert np.array_equal(y, want), (pair, k)                       # bit for bit
        assert np.all(np.abs(y.real) <= B.real * (1 + 1e-12)) and np.all(np.abs(y.imag) <= B.imag * (1 + 1e-12))
        total += len(y)
    # the closed form the bank's host side uses: ceil(N L / M) from phase 0
    assert total == -(-N * ref.L // ref.M)


def test_hand_derived_sizes_of_the_float_design(oracle):
    # 48 k -> 44.1 k: fc_norm = 0.45 * 44100 / (48000 * 147), 60 / fc_norm = 21333.3 -> (21333 / 147 + 1) 147 = 146 rows of 147
    assert calc_resample_f(48000, 44100)[:4] == (147, 160, 146 * 147, 146)
    # 48 k -> 96 k: fc_norm = 0.45 * 48000 / 96000 = 0.225, 60 / 0.225 = 266.67 -> (266 / 2 + 1) 2 = 268
    assert calc_resample_f(48000, 96000)[:4] == (2, 1, 268, 134)


def test_fc_low_moves_the_lower_band_edge_only_when_it_is_not_negative(oracle):
    base = calc_resample(48000, 44100)[4]
    assert np.array_equal(calc_resample(48000, 44100, fc_low=-3.0)[4], base)
    L, M, ncoef, cpp, h = calc_resample(48000, 44100, fc=9000.0, fc_low=300.0)
    full = 48000.0 * L
    want = oracle.fir_bandpass(ncoef, 300.0 / full, 9000.0 / full, 1.0, 1, 0, float(L))
    assert np.array_equal(h.reshape(L, cpp).T.reshape(-1), want)
    # the low-pass sums to L at 0 Hz; the band from 300 Hz up has 0 Hz on its lower slope (the window's main lobe is some 2 kHz wide here)
    assert abs(base.sum() - L) < 1e-6 * L and abs(h.sum()) < 0.5 * L


@pytest.mark.parametrize("pair", [(48000, 44100), (48000, 96000), (96000, 48000)])
def test_float_restatement_is_the_complex_ones_real_part_on_the_same_taps(oracle, pair):
    rng = np.random.default_rng(pair[1] // 100)
    x = rng.standard_normal(N).astype(np.float32)
    f = ResampleF(*pair)
    L, M, ncoef, cpp, h = calc_resample_f(*pair)
    c = Resample(pair[0], pair[1], ncoef=ncoef - 1, taps=h)              # (ncoef - 1) / L + 1 rows: the same table size
    assert (c.L, c.M, c.cpp) == (f.L, f.M, f.cpp) == (L, M, cpp)
    for (yf, Bf, If), (yc, Bc) in zip(run_cuts(f, x, CUTS), run_cuts(c, x.astype(np.complex128), CUTS)):
        assert yf.dtype == np.float32 and len(yf) == len(yc)
        assert np.array_equal(If, yc.real) and np.array_equal(yf, yc.real.astype(np.float32)) and np.array_equal(Bf, Bc.real)
        assert not np.any(yc.imag)


def test_setters_restart_only_on_a_change(oracle):
    x = _x(5)
    r = Resample(48000, 44100)
    r.process(x[:500])
    state = (r.idx_in, r.phnum, r.ring.copy())
    r.set_fc_low(-1.0)
    r.set_bandwidth(-1.0, 0.0)
    assert (r.idx_in, r.phnum) == state[:2] and np.array_equal(r.ring, state[2])
    r.set_fc_low(200.0)
    assert r.phnum == 0 and not np.any(r.ring) and r.idx_in == r.ringsize - 1
    r.process(x[500:700])
    r.set_rates(48000, 44100)                                           # setInRate_resample always goes through calc_resample
    assert r.phnum == 0 and not np.any(r.ring)
    r.run = 0
    y, _ = r.process(x[:7])
    assert np.array_equal(y, x[:7]) and r.phnum == 0
