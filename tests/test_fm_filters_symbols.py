"""The FM filter names are in the built library (no GPU): the five names a WDSP front end calls when the user picks an FM filter width
(wdsp/fmd.c:278-384) and the engine's five setters, each with a ctypes prototype in quisk_amd/lib.py and a declaration in
include/quiskhip.h with its reference lines beside it; and the engine class carries the setters."""
import os

WDSP = {"SetRXAFMAFFilter": 3, "SetRXAFMNCde": 2, "SetRXAFMMPde": 2, "SetRXAFMNCaud": 2, "SetRXAFMMPaud": 2}
ENGINE = {"qh_rxa_" + n: k + 1 for n, k in WDSP.items()}
LINES = {"SetRXAFMAFFilter": "wdsp/fmd.c:364-384", "SetRXAFMNCde": "wdsp/fmd.c:278-293", "SetRXAFMMPde": "wdsp/fmd.c:295-305",
         "SetRXAFMNCaud": "wdsp/fmd.c:307-322", "SetRXAFMMPaud": "wdsp/fmd.c:324-334"}


def test_the_ten_names_are_exported_and_bound(qh):
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
        assert LINES[n.replace("qh_rxa_", "")] in line[0], line[0]
    assert "FM channels share their filters" not in header and "share their filters' design" not in header


def test_the_engine_class_has_the_setters(qh):
    from quisk_amd import rxa
    for n in WDSP:
        assert n in rxa._SETTERS
    assert hasattr(qh.RxaEngine, "debug_fm_rows")
