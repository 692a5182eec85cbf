"""The plain references of tests/filter_forms_ref.py against the filter.c restatement (oracle.OracleFir / OracleHB45) and the golden
vectors made from the reference build, and the conditions under which the per-sample bounds of the three GPU test files mean what they
say.  No GPU."""
import os

import numpy as np
import pytest

import filter_forms_ref as R
from conftest import rel_rms
from filter_forms_ref import F32, SPLITS
from test_gpu_fir_forms import CASES as FIR_CASES
from test_gpu_hbcascade_forms import STAGES as HBC_STAGES
from test_gpu_polyphase_forms import CASES as RAT_CASES

GOLD = os.path.join(os.path.dirname(__file__), "golden", "filter_golden.npz")
AGREE = 1e-13


def stream(seed, n):
    rng = np.random.default_rng(seed)
    return rng.standard_normal(n) + 1j * rng.standard_normal(n)


@pytest.fixture(scope="module")
def gold():
    g = np.load(GOLD)
    assert list(g["splits"]) == SPLITS
    return g


def ragged(fn, x, d_or_ratio, taps):
    """fn call by call over SPLITS, the state (history, phase) carried by hand."""
    out, pos, phase = [], 0, 0
    for k in SPLITS:
        seg, hist = x[pos:pos + k], np.concatenate([np.zeros(taps.size, dtype=x.dtype), x[:pos]])
        if fn is R.fir_decimate:
            y, _ = R.fir_decimate(seg, taps, d_or_ratio, phase, hist)
            phase = (phase + k) % d_or_ratio
        else:
            U, D = d_or_ratio
            y, _ = R.rational(seg, taps, U, D, phase, hist)
            if k:
                phase = R.rational_count(k, U, D, phase)[1]
        out.append(y)
        pos += k
    return np.concatenate(out)


@pytest.mark.parametrize("name,tapkey,d", [("cDecimate_98_d2", "taps98", 2), ("cDecimate_147_d3", "taps147", 3),
                                            ("cDecimate_245_d5", "taps245", 5), ("cDecimate_98_d1", "taps98", 1)])
def test_fir_decimate_against_golden_and_oracle(oracle, gold, name, tapkey, d):
    x = stream(11, sum(SPLITS))
    y = ragged(R.fir_decimate, x, d, gold[tapkey])
    assert y.size == gold[name].size and rel_rms(y, gold[name]) < AGREE
    whole, A = R.fir_decimate(x, gold[tapkey], d)
    assert rel_rms(whole, y) < AGREE
    f = oracle.OracleFir(gold[tapkey])
    pos, ref = 0, []
    for k in SPLITS:
        ref.append(f.cDecimate(x[pos:pos + k], d))
        pos += k
    assert rel_rms(y, np.concatenate(ref)) < AGREE
    assert np.all(A.real >= np.abs(whole.real)) and np.all(A.imag >= np.abs(whole.imag))


def test_fir_decimate_complex_taps_against_golden(oracle, gold):
    x = stream(11, sum(SPLITS))
    f = oracle.OracleFir(gold["taps245"])
    f.tune(0.0625, 1)
    ct = np.ctypeslib.as_array(f.f.ctaps, shape=(2 * 245,)).view(np.complex128).copy()
    pos, ref = 0, []
    for k in SPLITS:
        ref.append(f.cCDecimate(x[pos:pos + k], 5))
        pos += k
    y = ragged(R.fir_decimate, x, 5, ct)
    assert rel_rms(y, np.concatenate(ref)) < AGREE


@pytest.mark.parametrize("name,tapkey,U,D", [("cInterpolate_36_x2", "taps36", 2, 1), ("cInterpDecim_98_6_5", "taps98", 2, 3)])
def test_rational_against_golden_and_oracle(oracle, gold, name, tapkey, U, D):
    x = stream(11, sum(SPLITS))
    y = ragged(R.rational, x, (U, D), gold[tapkey])
    assert y.size == gold[name].size and rel_rms(y, gold[name]) < AGREE
    whole, S = R.rational(x, gold[tapkey], U, D)
    assert rel_rms(whole, y) < AGREE
    f = oracle.OracleFir(gold[tapkey])
    pos, ref = 0, []
    for k in SPLITS:
        ref.append(f.cInterpDecim(x[pos:pos + k], U, D))
        pos += k
    assert rel_rms(y, np.concatenate(ref)) < AGREE
    assert np.all(S.real >= np.abs(whole.real)) and np.all(S.imag >= np.abs(whole.imag))


def test_hb45_against_golden_and_oracle(oracle, gold):
    x = stream(11, sum(SPLITS))
    y = ragged(R.fir_decimate, x, 2, R.hb45_taps())
    assert y.size == gold["cDecim2HB45"].size and rel_rms(y, gold["cDecim2HB45"]) < AGREE
    x = stream(13, 256 * 5 * 40)
    y8, B = R.hb45_chain(x, 8, R.U64)
    ref = x
    for _ in range(8):
        ref = oracle.OracleHB45().cDecim2(ref)
    assert y8.shape == ref.shape and rel_rms(y8, ref) < AGREE
    tail, _ = R.fir_decimate(y8, gold["taps245"], 5)
    assert rel_rms(tail, gold["cascade_8hb45_d5"]) < AGREE
    # two float64 evaluations of the chain in different orders: each is inside B of the exact result
    assert np.all(B.real > 0) and np.all(np.abs(y8.real - ref.real) <= 2 * B.real) and np.all(np.abs(y8.imag - ref.imag) <= 2 * B.imag)


@pytest.mark.parametrize("nstage", HBC_STAGES)
def test_hb45_bound_against_the_outer_tap(nstage):
    """What the cascade's fp32 bound can and cannot see: B over the output's RMS beside HB45's outer tap (1.86e-5).  A lost outer tap
    changes an output by about 1.86e-5 of a sample, inside the fp32 bound and seven orders above the fp64 one."""
    rec = R.hbc_case(nstage, F32, False)
    b32 = float(np.max(np.maximum(rec["B"].real, rec["B"].imag))) / rec["rms"]
    med = float(np.median(np.concatenate([rec["B"].real, rec["B"].imag], axis=None))) / rec["rms"]
    outer = abs(R.hb45_taps()[0])
    print("nstage %d: fp32 B / rms(want): median %.3e, largest %.3e; outer tap %.3e; TOL64 %.1e" % (nstage, med, b32, outer, R.TOL64))
    assert abs(outer - 1.86e-5) < 1e-7
    assert med > outer                          # fp32 cannot see a lost outer tap: its typical bound is wider than the tap ...
    assert R.TOL64 < 1e-6 * outer               # ... fp64 sees it a million times over


@pytest.mark.parametrize("case", RAT_CASES, ids=R.rat_case_id)
def test_float32_polyphase_sum_stays_inside_its_bound(case):
    """The kernel's arithmetic emulated in float32 on the CPU stays inside (K + 4) u S; the taps of every case keep |h[0]| and
    |h[ntaps - 1]| at 0.5 or more."""
    U, D, ntaps = case
    rec = R.rat_case(case, F32)
    assert abs(rec["taps"][0]) >= 0.5 and abs(rec["taps"][-1]) >= 0.5
    emu = R.polyphase_emulated(rec["x"], rec["taps"], U, D, np.float32)
    w = R.assert_inside("float32 emulation of %s" % R.rat_case_id(case), emu, rec["want"], rec["bound"], rec["blocks"], rec["calls"])
    print("%s: K = %d, worst error over bound %.3g" % (R.rat_case_id(case), rec["K"], w["ratio"]))
    assert w["ratio"] > 0.01 or rec["K"] == 1   # a bound the arithmetic comes nowhere near would guard nothing


@pytest.mark.parametrize("case", FIR_CASES, ids=R.fir_case_id)
def test_firbank_float32_bound_stays_under_the_project_tolerance(case):
    """16 E <= TOL32 rms(want) for every FirBank case: the per-sample bound is never looser than the project's stream tolerance moved to
    a sample.  An impulse stream's output is mostly zeros, so its RMS measures how sparse it is and not how large; there the condition is
    taken against the output's largest sample."""
    rec = R.fir_case(case, "noise", F32)
    assert abs(rec["taps"][0]) >= 0.5 and abs(rec["taps"][-1]) >= 0.5
    print("%s noise: E / rms(want) = %.3e" % (R.fir_case_id(case), rec["E"] / rec["rms"]))
    assert 16.0 * rec["E"] <= R.TOL32 * rec["rms"]
    rec = R.fir_case(case, "impulses", F32)
    peak = float(np.max(np.abs(rec["want"])))
    print("%s impulses: E / max|want| = %.3e, E / rms(want) = %.3e" % (R.fir_case_id(case), rec["E"] / peak, rec["E"] / rec["rms"]))
    assert 16.0 * rec["E"] <= R.TOL32 * peak


def test_one_wrapped_tap_at_one_seam_breaks_the_bounds():
    """What the bounds are for: the last tap's product lost at ONE output of one channel (a tile that starts a sample early, a history row
    a sample short).  With these taps it is tens of thousands of bounds large in either type.  With a last tap of 1e-4, the size the
    Hann-weighted taps of the older tests end on, the relative RMS over the stream stays under TOL32 and the per-sample bound still
    sees it."""
    case = (1023, 32, False)
    for dtype in (R.F64, F32):
        rec = R.fir_case(case, "noise", dtype)
        m = int(rec["tiles"][5])
        lost = rec["taps"][-1] * rec["x"][1, 32 * m + 31 - 1022].astype(np.complex128)
        got = rec["want"].copy()
        got[1, m] -= lost
        w = R.worst_sample(got, rec["want"], rec["bound"], rec["tiles"], rec["calls"])
        assert (w["channel"], w["index"], w["to_seam"]) == (1, m, 0) and w["ratio"] > 1e4
        got[1, m] = rec["want"][1, m] - 1e-4 * lost
        assert rel_rms(got[1], rec["want"][1]) < R.TOL32
        assert R.worst_sample(got, rec["want"], rec["bound"], rec["tiles"], rec["calls"])["ratio"] > 2


def test_os_model_is_an_overlap_save_filter():
    """In float64 the model agrees with the direct sums to rounding, at a tile per output and with a decimation phase."""
    x = stream(3, 700)
    for ntaps, d in ((4096, 1), (300, 7), (1, 3)):
        taps = R.forced_taps(ntaps, 9)
        want, _ = R.fir_decimate(x, taps, d, phase0=d // 2)
        got = R.os_model(x, taps, d, R.F64, phase0=d // 2)
        assert got.dtype == np.complex128 and got.shape == want.shape
        assert rel_rms(got, want) < 1e-13


def test_worst_sample_names_the_sample_and_its_distances():
    want = np.zeros((2, 50), dtype=np.complex128)
    got = want.copy()
    got[1, 33] = 1e-3j
    w = R.worst_sample(got, want, 1e-6, seams=[0, 30, 40], calls=[0, 20])
    assert (w["channel"], w["index"], w["part"], w["to_seam"], w["to_call"]) == (1, 33, "im", 3, 13) and abs(w["ratio"] - 1e3) < 1e-6
    with pytest.raises(AssertionError, match="channel 1 sample 33"):
        R.assert_inside("x", got, want, 1e-6, [0, 30, 40], [0, 20])
    got[0, 2] = np.nan
    assert R.worst_sample(got, want, 1e-6)["ratio"] == np.inf
    assert R.worst_sample(want, want, np.zeros((2, 50), dtype=np.complex128))["ratio"] == 0.0
