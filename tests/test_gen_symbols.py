"""gen0's names are in the built library (no GPU): the eight names a WDSP caller binds (wdsp/gen.c:384-450), the engine's nine, each with
a ctypes prototype in quisk_amd/lib.py and one declaration in include/quiskhip.h that cites its lines of gen.c; and the engine class
carries the methods."""
import os

SETTERS = {"Run": 2, "Mode": 2, "ToneMag": 2, "ToneFreq": 2, "NoiseMag": 2, "SweepMag": 2, "SweepFreq": 3, "SweepRate": 2}
WDSP = {"SetRXAPreGen" + n: k for n, k in SETTERS.items()}
ENGINE = {**{"qh_rxa_SetRXAPreGen" + n: k + 1 for n, k in SETTERS.items()}, "qh_rxa_set_gen_seed": 3}
METHODS = tuple(WDSP) + ("set_gen_seed",)


def test_the_names_are_exported_and_bound(qh):
    lib = qh.load()
    names = {**WDSP, **ENGINE}
    assert len(WDSP) == 8 and len(ENGINE) == 9
    missing = [n for n in names if not hasattr(lib, n)]
    assert not missing, missing
    unbound = [n for n in names if getattr(lib, n).argtypes is None]
    assert not unbound, unbound
    wrong = [(n, len(getattr(lib, n).argtypes)) for n, k in names.items() if len(getattr(lib, n).argtypes) != k]
    assert not wrong, wrong
    assert all(getattr(lib, n).restype is None for n in WDSP)   # the reference's are void


def test_the_header_declares_them_with_their_reference_lines(qh):
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "quiskhip.h")).read()
    for n in list(WDSP) + list(ENGINE):
        line = [ln for ln in header.splitlines() if (" " + n + "(") in ln]
        assert len(line) == 1, (n, line)
        assert "wdsp/gen.c:" in line[0], line[0]


def test_the_engine_class_has_the_methods(qh):
    for n in METHODS:
        assert callable(getattr(qh.RxaEngine, n, None)), n
