"""The sender's and the siphon's names are in the built library (no GPU): the three names a WDSP caller binds (wdsp/sender.c:111-122,
wdsp/siphon.c:182-211), the engine's tap functions and the analyzer's float feed, each with a ctypes prototype in quisk_amd/lib.py and one
declaration in include/quiskhip.h that cites its lines of sender.c or siphon.c; and the engine class carries the methods."""
import os

WDSP = {"SetRXASpectrum": 5, "RXAGetaSipF": 3, "RXAGetaSipF1": 3}
ENGINE = {"qh_rxa_set_sender": 3, "qh_rxa_sender_rows": 4, "qh_rxa_sender_rows_host": 5, "qh_rxa_set_siphon": 3, "qh_rxa_get_sip": 4,
          "qh_rxa_attach_display": 3, "qh_rxa_feed_display": 3, "qh_ana_feed_f32": 8}
METHODS = ("set_sender", "sender_rows_host", "set_siphon", "get_sip", "attach_display")


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
        assert "wdsp/sender.c:" in line[0] or "wdsp/siphon.c:" in line[0], line[0]


def test_the_engine_class_has_the_methods(qh):
    for n in METHODS:
        assert callable(getattr(qh.RxaEngine, n, None)), n
    from quisk_amd.analyzer import AnalyzerBank
    assert callable(getattr(AnalyzerBank, "feed_f32", None))
