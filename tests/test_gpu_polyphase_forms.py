"""The time-domain polyphase resampler (C ABI group 3c, polyphase_kernel) at nine ratios in both sample types, every output sample
inside (K + 4) u S[m] of direct float64 sums (tests/filter_forms_ref.py): the bound of a length-K dot product in the bank's type with
taps rounded to it and one multiply by U.  The taps carry no window (first and last +-1), so a history row that is one sample short or
a phase that slips by one is an error of the size of a sample.  -m gpu."""
import numpy as np
import pytest

import filter_forms_ref as R
from filter_forms_ref import F32, F64

pytestmark = pytest.mark.gpu

# (interp U, decim D, ntaps).  2/1 with 45 taps: the taps do not divide evenly and the padding tap is zero.  7/64 with 5 taps: K = 1,
# no history row is read.
CASES = [(2, 1, 36), (2, 1, 45), (6, 5, 245), (4, 5, 245), (1, 4, 98), (3, 7, 301), (8, 1, 1000), (1, 1, 64), (7, 64, 5)]
HANDOVER = [(6, 5, 245), (3, 7, 301)]
TYPES = [pytest.param(F64, id="f64"), pytest.param(F32, id="f32")]


@pytest.mark.parametrize("dtype", TYPES)
@pytest.mark.parametrize("case", CASES, ids=R.rat_case_id)
def test_every_sample_inside_its_bound(qh, case, dtype):
    U, D, ntaps = case
    rec = R.rat_case(case, dtype)
    bank = qh.RationalFir(3, rec["taps"], U, D, dtype=dtype)
    assert bank.K == rec["K"]

    def after(j, y):
        k, phase = rec["counts"][j]
        assert (y.shape[1], bank.phase) == (k, phase), "call %d of %d samples: (outputs, phase)" % (j, rec["sizes"][j])

    y, starts = R.run_calls(bank, rec["x"], rec["sizes"], after)
    if D > 3 * U:
        assert sum(1 for n, (k, _) in zip(rec["sizes"], rec["counts"]) if n == 1 and k == 0) >= 4      # the phase outlasts several calls
    w = R.assert_inside("%s %s" % (R.rat_case_id(case), "f32" if dtype else "f64"), y, rec["want"], rec["bound"], rec["blocks"],
                        rec["calls"])
    print("worst error over bound %.3g" % w["ratio"])


@pytest.mark.parametrize("dtype", TYPES)
@pytest.mark.parametrize("case", HANDOVER, ids=R.rat_case_id)
def test_state_handed_over_from_the_host(qh, case, dtype):
    """Bank A runs a prefix; bank B starts from the prefix's last K - 1 samples and A's phase (RationalFir.set_state); both then take the
    same calls.  B's outputs equal A's bit for bit and are inside the bound."""
    U, D, ntaps = case
    K = (ntaps + U - 1) // U
    taps = R.forced_taps(ntaps, 3 * ntaps + U)
    n_pre, later = 1003, [K - 2, 1, K, 0, 300, 2, 611]
    x = R.make_input("noise", 3, n_pre + sum(later), 11 * ntaps + D, dtype)
    want, S = R.rational(x, taps, U, D)
    a = qh.RationalFir(3, taps, U, D, dtype=dtype)
    ya_pre, _ = R.run_calls(a, x[:, :n_pre], [400, n_pre - 400])
    m_pre, phase = R.rational_count(n_pre, U, D, 0)
    assert (ya_pre.shape[1], a.phase) == (m_pre, phase)
    b = qh.RationalFir(3, taps, U, D, dtype=dtype)
    b.set_state(x[:, n_pre - (K - 1):n_pre], a.phase)
    assert b.phase == phase
    ya, calls = R.run_calls(a, x[:, n_pre:], later)
    yb, _ = R.run_calls(b, x[:, n_pre:], later)
    assert ya.shape == yb.shape == want[:, m_pre:].shape
    assert ya.tobytes() == yb.tobytes(), "the bank started from a host state differs from the one that ran the prefix"
    assert a.phase == b.phase
    R.assert_inside("hand-over %s" % R.rat_case_id(case), yb, want[:, m_pre:], (K + 4) * R.unit(dtype) * S[:, m_pre:], (), calls)
    # the same start through the reference's own history and phase arguments
    want2, _ = R.rational(x[:, n_pre:], taps, U, D, phase0=phase, hist=x[:, :n_pre])
    assert np.max(np.abs(want2 - want[:, m_pre:])) <= 1e-13 * R.rms(want)
    with pytest.raises(ValueError):
        b.set_state(x[:, :K], 0)                        # one sample too many
