"""The FM squelch's names are in the built library (no GPU): the four names a WDSP caller binds (wdsp/fmsq.c:235-279), the engine's four
setters and its diagnostic, each with a ctypes prototype in quisk_amd/lib.py and a declaration in include/quiskhip.h; and the engine class
carries the setters beside the SSQL ones."""
import os

WDSP = {"SetRXAFMSQRun": 2, "SetRXAFMSQThreshold": 2, "SetRXAFMSQNC": 2, "SetRXAFMSQMP": 2}
ENGINE = {"qh_rxa_SetRXAFMSQRun": 3, "qh_rxa_SetRXAFMSQThreshold": 3, "qh_rxa_SetRXAFMSQNC": 3, "qh_rxa_SetRXAFMSQMP": 3, "qh_rxa_debug_fmsq": 4}


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
        assert n == "qh_rxa_debug_fmsq" or "wdsp/fmsq.c:" in line[0], line[0]


def test_the_engine_class_has_the_setters(qh):
    from quisk_amd import rxa
    for n in WDSP:
        assert n in rxa._SETTERS
    assert hasattr(qh.RxaEngine, "debug_fmsq")
