"""Every form of the overlap-save FIR bank (C ABI group 3: osfir_kernel at FOLD 1, 2, 4 and 8, with the plain store and the
keep-every-pick-th store, real and complex taps) in both sample types, every output sample held to a bound of its own against direct
float64 sums (tests/filter_forms_ref.py).  The taps carry no window: the first and the last are +-1, so a tile that starts its valid
outputs one sample early, a history row one sample short or a hist_next copy that misses a sample is an error of the size of a sample
at one output of a tile -- which a relative RMS over the stream cannot see and a per-sample bound cannot miss.

Measured (profiles/filter_forms_margins.json): in fp32 the kernel's largest error is 1.3 to 5.5 E, at most 0.34 of the bound 16 E, its
worst samples anywhere in a tile; in fp64 at most 0.021 of TOL64 rms(want).  No form needed an exception.  -m gpu."""
import numpy as np
import pytest

import filter_forms_ref as R
from filter_forms_ref import F32, F64

pytestmark = pytest.mark.gpu

# (ntaps, decim, complex taps).  Decimations 1, 3, 7 / 2, 6 / 4, 12, 20 / 8, 24, 32, 40: every fold with and without a pick.
# (4096, 1) leaves Lf = 1 (one output per tile), (4081, 8) Lf = 2, (4090, 7) one output per tile behind a pick of 7; one tap raises P
# to the fold.
CASES = [
    (1, 1, False), (2, 1, False), (98, 1, False), (4096, 1, False), (147, 3, False), (4090, 7, False),      # fold 1
    (43, 2, False), (98, 2, False), (100, 6, False),                                                        # fold 2
    (6, 4, False), (255, 4, False), (301, 12, False), (255, 20, False),                                     # fold 4
    (1, 8, False), (64, 8, False), (4081, 8, False), (511, 24, False), (1023, 32, False), (767, 40, False),  # fold 8
    (98, 1, True), (64, 8, True),                                                                           # complex taps
]
REFUSED = [(4097, 1), (4090, 8), (4081, 24)]            # Lf <= 0
HANDOVER = [(245, 5), (1023, 32)]
TYPES = [pytest.param(F64, id="f64"), pytest.param(F32, id="f32")]

# Exceptions under the rule "an fp32 form that exceeds 16 E but is clean at every seam is held to TOL32 rms(want) per sample, with the
# step that costs the precision named": (case, input) -> reason.  None so far.
F32_EXCEPTIONS = {}


def bound_of(case, kind, dtype, rec):
    if dtype == F32 and (case, kind) in F32_EXCEPTIONS:
        return R.TOL32 * rec["rms"]
    return rec["bound"]


@pytest.mark.parametrize("kind", ["noise", "impulses"])
@pytest.mark.parametrize("dtype", TYPES)
@pytest.mark.parametrize("case", CASES, ids=R.fir_case_id)
def test_every_sample_inside_its_bound(qh, case, dtype, kind):
    ntaps, d, _ = case
    rec = R.fir_case(case, kind, dtype)
    assert rec["geometry"][3] > 0
    bank = qh.FirBank(3, rec["taps"], d, dtype=dtype)
    y, starts = R.run_calls(bank, rec["x"], rec["sizes"])
    assert list(starts) == list(rec["calls"]) and y.shape == rec["want"].shape, "output counts differ from the reference's"
    assert y.dtype == R.ctype(dtype)
    w = R.assert_inside("%s %s %s" % (R.fir_case_id(case), "f32" if dtype else "f64", kind), y, rec["want"],
                        bound_of(case, kind, dtype, rec), rec["tiles"], rec["calls"])
    print("worst error over bound %.3g, %s samples from a tile start" % (w["ratio"], w["to_seam"]))


@pytest.mark.parametrize("dtype", TYPES)
def test_refusals_just_beyond_the_extremes(qh, dtype):
    """Taps that leave a tile no output (Lf <= 0) are refused at creation, and a good bank created straight after still works."""
    for ntaps, d in REFUSED:
        assert R.stage_geometry(ntaps, d)[3] <= 0
        with pytest.raises(qh.QuiskHipError):
            qh.FirBank(3, R.forced_taps(ntaps, 1), d, dtype=dtype)
        x = R.make_input("noise", 2, 50, 3, dtype)
        y = qh.FirBank(2, [1.0, 0.0, -1.0], 2, dtype=dtype).process_host(x)
        want, _ = R.fir_decimate(x, [1.0, 0.0, -1.0], 2)
        assert y.shape == want.shape
        R.assert_inside("bank after a refusal", y, want, 64 * R.unit(dtype) * np.max(np.abs(x)))


@pytest.mark.parametrize("dtype", TYPES)
@pytest.mark.parametrize("ntaps,d", HANDOVER)
def test_state_handed_over_from_the_host(qh, ntaps, d, dtype):
    """Bank A runs a prefix; bank B starts from the prefix's last ntaps - 1 samples and phase = len(prefix) % decim (FirBank.set_state);
    both then take the same calls.  B's outputs equal A's bit for bit and are inside the bound.

    A's history row holds P samples, B's the ntaps - 1 it was given behind P - (ntaps - 1) zeros (two for 1023 taps at fold 8).  A tile
    reads the row from slot decim - 1 - phase on, so the prefix's length is chosen to leave phase <= decim - 3: neither bank then reads
    the slots in which they differ, and the transforms see the same numbers."""
    fold, pick, P, Lf, per_tile = R.stage_geometry(ntaps, d)
    n_pre = 3001
    assert d - 1 - n_pre % d >= P - (ntaps - 1)
    later = [P - 1, 1, P + 1, per_tile * d + 3, 0, 2, 777]
    taps = R.forced_taps(ntaps, 5 * ntaps + d)
    x = R.make_input("noise", 3, n_pre + sum(later), 17 * ntaps, dtype)
    want, _ = R.fir_decimate(x, taps, d)
    m_pre = n_pre // d
    if dtype == F32:
        model = R.os_model(x[0], taps, d, F32)
        bound = 16.0 * float(np.max(np.maximum(np.abs(model.real - want[0].real), np.abs(model.imag - want[0].imag))))
    else:
        bound = R.TOL64 * R.rms(want)
    a = qh.FirBank(3, taps, d, dtype=dtype)
    ya_pre, _ = R.run_calls(a, x[:, :n_pre], [1000, n_pre - 1000])
    assert ya_pre.shape[1] == m_pre
    b = qh.FirBank(3, taps, d, dtype=dtype)
    b.set_state(x[:, n_pre - (ntaps - 1):n_pre], n_pre % d)
    ya, calls = R.run_calls(a, x[:, n_pre:], later)
    yb, _ = R.run_calls(b, x[:, n_pre:], later)
    assert ya.shape == yb.shape == want[:, m_pre:].shape
    assert ya.tobytes() == yb.tobytes(), "the bank started from a host state differs from the one that ran the prefix"
    R.assert_inside("hand-over %d taps / %d" % (ntaps, d), yb, want[:, m_pre:], bound, (), calls)
    with pytest.raises(ValueError):
        b.set_state(x[:, :ntaps], 0)                    # one sample too many
    with pytest.raises(qh.QuiskHipError):
        b.set_state(None, d)                            # phase out of range
