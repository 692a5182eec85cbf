"""The range the ANF / ANR setters accept (no GPU): taps 1..2048 and delay 0..2047, the reference's delay line (ANF_DLINE_SIZE, wdsp/anf.h).
The check stands in front of everything else a setter does, so it shows without an engine: a value outside the line is refused with
QH_ERR_INVALID and the range in the message, one inside it gets as far as the missing engine.  And the header and the documents state
that range, none of them the 64 taps of the one-tap-per-lane form alone."""
import ctypes as C
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
QH_ERR_INVALID = -2
RANGE = b"taps 1..2048, delay 0..2047"


def _bound(qh):
    lib = qh.load()
    for f in ("ANF", "ANR"):
        for n in ("Taps", "Delay"):
            getattr(lib, "qh_rxa_SetRXA%s%s" % (f, n)).argtypes = [C.c_void_p, C.c_int, C.c_int]
        getattr(lib, "qh_rxa_SetRXA%sVals" % f).argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_double, C.c_double]
    return lib


@pytest.mark.parametrize("f", ["ANF", "ANR"])
@pytest.mark.parametrize("what,value", [("Taps", 0), ("Taps", -1), ("Taps", 2049), ("Delay", -1), ("Delay", 2048)])
def test_a_value_outside_the_delay_line_is_refused(qh, f, what, value):
    lib = _bound(qh)
    assert getattr(lib, "qh_rxa_SetRXA%s%s" % (f, what))(None, 0, value) == QH_ERR_INVALID
    assert RANGE in lib.qh_last_error()
    taps, delay = (value, 16) if what == "Taps" else (64, value)
    assert getattr(lib, "qh_rxa_SetRXA%sVals" % f)(None, 0, taps, delay, 1e-4, 0.1) == QH_ERR_INVALID
    assert RANGE in lib.qh_last_error()


@pytest.mark.parametrize("f", ["ANF", "ANR"])
@pytest.mark.parametrize("what,value", [("Taps", 1), ("Taps", 65), ("Taps", 2048), ("Delay", 0), ("Delay", 65), ("Delay", 2047)])
def test_a_value_inside_it_gets_to_the_engine(qh, f, what, value):
    lib = _bound(qh)
    assert getattr(lib, "qh_rxa_SetRXA%s%s" % (f, what))(None, 0, value) == QH_ERR_INVALID
    assert RANGE not in lib.qh_last_error() and b"null engine" in lib.qh_last_error()


def test_the_header_and_the_documents_state_the_range():
    header = open(os.path.join(ROOT, "include", "quiskhip.h")).read()
    assert header.count("taps 1..2048") >= 2 and header.count("delay 0..2047") >= 2         # the engine's setters and the WDSP names
    for name in ("DESIGN.md", os.path.join("docs", "ALGORITHMS.md"), "INTEGRATION.md"):
        text = open(os.path.join(ROOT, name)).read()
        assert "lms_long_kernel" in text, name
        assert "above 64 taps" not in text and "up to 64 taps" not in text, name
