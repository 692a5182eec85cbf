"""The fused half-band cascade (C ABI group 3b) at 4, 6 and 7 stages in both sample types, every output sample inside the error bound
carried through the chain, B_nstage (tests/filter_forms_ref.py hb45_chain).

What each type can see.  HB45's outer tap is 1.86e-5.  In fp32 B is, at its median, 3.4e-5 of the output's RMS at 4 stages, 1.7e-4 at
6 and 3.6e-4 at 7 (written and checked by tests/test_filter_forms_ref.py::test_hb45_bound_against_the_outer_tap), so a warm-up or a
segment seam that loses the outer tap's product stays inside the fp32 bound: fp32 here guards the arithmetic of the 4-, 6- and 7-stage
forms, not their seams.  fp64 is also held to TOL64 rms(want) per sample, seven orders below the outer tap, and is what guards warm-up,
segment seams and the history written between calls.  -m gpu."""
import pytest

import filter_forms_ref as R
from filter_forms_ref import F32, F64

pytestmark = pytest.mark.gpu

STAGES = [4, 6, 7]
CASES = [(ns, ragged) for ns in STAGES for ragged in (False, True)]
TYPES = [pytest.param(F64, id="f64"), pytest.param(F32, id="f32")]


def hbc_case_id(case):
    return "%dstages_%s" % (case[0], "ragged_calls" if case[1] else "one_call")


@pytest.mark.parametrize("dtype", TYPES)
@pytest.mark.parametrize("case", CASES, ids=hbc_case_id)
def test_every_sample_inside_its_bound(qh, case, dtype):
    """One call: one channel of 5 x 8192 + 3 x 2^nstage samples -- five segments and a ragged last step at 4 stages (qh_hbcascade.hip
    launch()).  Ragged calls: two channels fed multiples of 2^nstage around the launch's history length."""
    nstage, ragged = case
    rec = R.hbc_case(nstage, dtype, ragged)
    if not ragged and nstage == 4:
        assert R.hbc_segment(1, rec["sizes"][0], nstage) == 8192
    c = qh.HalfBandCascade(rec["nch"], nstage, dtype=dtype)
    y, starts = R.run_calls(c, rec["x"], rec["sizes"])
    assert y.shape == rec["want"].shape and list(starts) == list(rec["calls"])
    name = "%s %s" % (hbc_case_id(case), "f32" if dtype else "f64")
    w = R.assert_inside(name, y, rec["want"], rec["B"], rec["segs"], rec["calls"])
    print("worst error over B %.3g" % w["ratio"])
    if dtype == F64:
        w = R.assert_inside(name + " (TOL64 rms)", y, rec["want"], R.TOL64 * rec["rms"], rec["segs"], rec["calls"])
        print("worst error over TOL64 rms %.3g" % w["ratio"])
