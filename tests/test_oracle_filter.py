"""The filter.c restatement (oracle/quisk_oracle.c) against golden vectors generated from the reference's
own filter.c, and bit-exact against that build's outputs on seeded random input (tests/golden/ref_build_golden.npz)."""
import os

import numpy as np
import pytest

GOLD = os.path.join(os.path.dirname(__file__), "golden", "filter_golden.npz")
SPLITS = [0, 1, 7, 333, 2, 64, 1000, 5, 0, 588]


def stream(seed, n, complex_=True):
    rng = np.random.default_rng(seed)
    x = rng.standard_normal(n)
    if complex_:
        x = x + 1j * rng.standard_normal(n)
    return x


def run_split(fn, x):
    out, pos = [], 0
    for k in SPLITS:
        out.append(fn(x[pos:pos + k]))
        pos += k
    return np.concatenate(out)


@pytest.fixture(scope="module")
def gold():
    return np.load(GOLD)


def test_golden_all_primitives(oracle, gold):
    po = oracle
    n = sum(SPLITS)
    xc, xr = stream(11, n), stream(12, n, False)
    t98, t147, t245, t36 = gold["taps98"], gold["taps147"], gold["taps245"], gold["taps36"]
    cases = {}
    for name, taps, d in (("cDecimate_98_d2", t98, 2), ("cDecimate_147_d3", t147, 3), ("cDecimate_245_d5", t245, 5),
                          ("cDecimate_98_d1", t98, 1)):
        f = po.OracleFir(taps)
        cases[name] = run_split(lambda v, f=f, d=d: f.cDecimate(v, d), xc)
    f = po.OracleFir(t245); f.tune(0.0625, 1)
    cases["cCDecimate_245_d5_usb"] = run_split(lambda v: f.cCDecimate(v, 5), xc)
    f2 = po.OracleFir(t98); f2.tune(-0.11, 0)
    cases["cCDecimate_98_d2_lsb"] = run_split(lambda v: f2.cCDecimate(v, 2), xc)
    f3 = po.OracleFir(t147, is_complex=False)
    cases["dDecimate_147_d3"] = run_split(lambda v: f3.dDecimate(v, 3), xr)
    f4 = po.OracleFir(t36, is_complex=False)
    cases["dFilter_36"] = run_split(lambda v: f4.dFilter(v), xr)
    f5 = po.OracleFir(t36)
    cases["cInterpolate_36_x2"] = run_split(lambda v: f5.cInterpolate(v, 2), xc)
    f6 = po.OracleFir(t36, is_complex=False)
    cases["dInterpolate_36_x3"] = run_split(lambda v: f6.dInterpolate(v, 3), xr)
    f7 = po.OracleFir(t98)
    cases["cInterpDecim_98_6_5"] = run_split(lambda v: f7.cInterpDecim(v, 2, 3), xc)
    h = po.OracleHB45(); cases["cDecim2HB45"] = run_split(h.cDecim2, xc)
    h2 = po.OracleHB45(); cases["cInterp2HB45"] = run_split(h2.cInterp2, xc)
    h3 = po.OracleHB45(); cases["dInterp2HB45"] = run_split(h3.dInterp2, xr)
    for name, got in cases.items():
        want = gold[name]
        assert got.shape == want.shape, name
        # the tuned (complex-tap) cases go through libm's sin/cos at table-build time: allow 1 ulp there
        if name.startswith("cCDecimate"):
            assert np.allclose(got, want, rtol=0, atol=1e-15 * np.abs(want).max()), name
        else:
            assert np.array_equal(got, want), name          # bit exact


def test_golden_cascade_config5(oracle, gold):
    po = oracle
    x = stream(13, 256 * 5 * 40)
    y = x
    for _ in range(8):
        y = po.OracleHB45().cDecim2(y)
    out = po.OracleFir(gold["taps245"]).cDecimate(y, 5)
    assert np.array_equal(out, gold["cascade_8hb45_d5"])


REF_GOLD = os.path.join(os.path.dirname(__file__), "golden", "ref_build_golden.npz")
BIT_EXACT_CUTS = ((0, 13), (13, 14), (14, 2500), (2500, 4000))


def bit_exact_cases():
    """(ntaps, decim), taps, input of test_bit_exact_against_reference_build -- tests/golden/make_ref_build_golden.py replays the same
    cases on the reference build."""
    rng = np.random.default_rng(77)
    for ntaps, d in ((5, 1), (50, 2), (147, 3), (1023, 32), (64, 7)):
        taps = rng.standard_normal(ntaps)
        yield (ntaps, d), taps, stream(rng.integers(1 << 30), 4000)


def test_bit_exact_against_reference_build(oracle):
    """Every call's output, bit for bit, as the reference's own filter.c (oracle/_ref) put it out: tests/golden/ref_build_golden.npz."""
    po = oracle
    ref = np.load(REF_GOLD)
    for (ntaps, d), taps, x in bit_exact_cases():
        a = po.OracleFir(taps)
        for lo, hi in BIT_EXACT_CUTS:
            assert np.array_equal(a.cDecimate(x[lo:hi], d), ref["fir_%d_%d_%d" % (ntaps, d, lo)]), (ntaps, d, lo)
    a = po.OracleHB45()
    x = stream(5, 3001)
    assert np.array_equal(a.cDecim2(x[:1001]), ref["hb45_0"])
    assert np.array_equal(a.cDecim2(x[1001:]), ref["hb45_1001"])


def test_decimator_is_plain_convolution(oracle):
    """Independent check of what the primitive means: y[m] = sum_k h[k] x[D*m + D-1 - k] (filter.c:203-229)."""
    po = oracle
    rng = np.random.default_rng(3)
    taps = rng.standard_normal(31)
    x = stream(4, 600)
    y = po.OracleFir(taps).cDecimate(x, 4)
    full = np.convolve(x, taps)[:600]
    assert np.allclose(y, full[3::4], rtol=0, atol=1e-12)
