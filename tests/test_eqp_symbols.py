"""The receive equalizer's names are in the built library (no GPU): the eight names a WDSP caller binds (wdsp/eq.c:242-377), the engine's
eight setters and its diagnostic, each with a ctypes prototype in quisk_amd/lib.py and a declaration in include/quiskhip.h that cites its
lines of eq.c; and the engine class carries the setters and debug_eqp."""
import os

WDSP = {"SetRXAEQRun": 2, "SetRXAEQNC": 2, "SetRXAEQMP": 2, "SetRXAEQProfile": 4, "SetRXAEQCtfmode": 2, "SetRXAEQWintype": 2,
        "SetRXAGrphEQ": 2, "SetRXAGrphEQ10": 2}
ENGINE = {**{"qh_rxa_" + n: k + 1 for n, k in WDSP.items()}, "qh_rxa_debug_eqp": 4}


def test_the_names_are_exported_and_bound(qh):
    lib = qh.load()
    names = {**WDSP, **ENGINE}
    missing = [n for n in names if not hasattr(lib, n)]
    assert not missing, missing
    unbound = [n for n in names if getattr(lib, n).argtypes is None]
    assert not unbound, unbound
    wrong = [(n, len(getattr(lib, n).argtypes)) for n, k in names.items() if len(getattr(lib, n).argtypes) != k]
    assert not wrong, wrong


def test_the_header_declares_them_with_their_reference_lines(qh):
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "quiskhip.h")).read()
    for n in list(WDSP) + list(ENGINE):
        line = [ln for ln in header.splitlines() if (" " + n + "(") in ln]
        assert len(line) == 1, (n, line)
        assert n == "qh_rxa_debug_eqp" or "wdsp/eq.c:" in line[0], line[0]


def test_the_engine_class_has_the_setters(qh):
    from quisk_amd import rxa
    for n in WDSP:
        assert n in rxa._SETTERS
    assert hasattr(qh.RxaEngine, "debug_eqp")
