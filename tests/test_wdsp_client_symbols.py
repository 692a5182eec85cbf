"""The RXA names that WDSP's other clients (piHPSDR, linHPSDR, Thetis) call are in the built library (no GPU): the AGC's display-side
knobs (wdsp/wcpAGC.c:440-557), pan and binaural (patchpanel.c:158-192), nc / mp / window per stage (nbp.c:563-588, snb.c:829-855,
bandpass.c:411-457) and the two wisdom names (wisdom.c).  Each is exported, declared in include/quiskhip.h with its lines of the reference,
has a ctypes prototype in quisk_amd/lib.py, and -- but for the wisdom pair, which no engine has -- a qh_rxa_* form that the engine class
reaches."""
import ctypes as C
import os
import re

# name: (source file of the reference, arguments behind the channel)
NAMES = {
    "SetRXAAGCThresh": ("wcpAGC.c", 3), "GetRXAAGCThresh": ("wcpAGC.c", 3), "SetRXAAGCHangLevel": ("wcpAGC.c", 1),
    "GetRXAAGCHangLevel": ("wcpAGC.c", 1), "GetRXAAGCHangThreshold": ("wcpAGC.c", 1), "GetRXAAGCTop": ("wcpAGC.c", 1),
    "SetRXAAGCMaxInputLevel": ("wcpAGC.c", 1),
    "SetRXAPanelPan": ("patchpanel.c", 1), "SetRXAPanelBinaural": ("patchpanel.c", 1),
    "RXANBPSetNC": ("nbp.c", 1), "RXANBPSetMP": ("nbp.c", 1),
    "RXABPSNBASetNC": ("snb.c", 1), "RXABPSNBASetMP": ("snb.c", 1),
    "SetRXABandpassNC": ("bandpass.c", 1), "SetRXABandpassMP": ("bandpass.c", 1), "SetRXABandpassWindow": ("bandpass.c", 1),
}
WISDOM = ("WDSPwisdom", "wisdom_get_status")
HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "quiskhip.h")


def test_the_names_are_exported_and_bound(qh):
    lib = qh.load()
    want = {**{n: k + 1 for n, (_, k) in NAMES.items()}, **{"qh_rxa_" + n: k + 2 for n, (_, k) in NAMES.items()},
            "WDSPwisdom": 1, "wisdom_get_status": 0}
    missing = [n for n in want if not hasattr(lib, n)]
    assert not missing, missing
    unbound = [n for n in want if getattr(lib, n).argtypes is None]
    assert not unbound, unbound
    wrong = [(n, len(getattr(lib, n).argtypes)) for n, k in want.items() if len(getattr(lib, n).argtypes) != k]
    assert not wrong, wrong


def test_the_header_declares_them_with_their_reference_lines():
    lines = open(HEADER).read().splitlines()
    for n, (src, _) in NAMES.items():
        for name in (n, "qh_rxa_" + n):
            decl = [ln for ln in lines if re.search(r"(?<![A-Za-z0-9_])" + name + r"\(", ln)]
            assert len(decl) == 1, (name, decl)
            assert re.search(r"wdsp/" + re.escape(src) + r":\d+-\d+", decl[0]), decl[0]
    for name in WISDOM:
        decl = [ln for ln in lines if re.search(r"(?<![A-Za-z0-9_])" + name + r"\(", ln)]
        assert len(decl) == 1, (name, decl)
        assert re.search(r"wdsp/wisdom\.c:\d+-\d+", decl[0]), decl[0]


def test_the_engine_class_reaches_them(qh):
    from quisk_amd import rxa
    for n in NAMES:
        if n.startswith("Get"):
            assert callable(getattr(qh.RxaEngine, n)), n
        else:
            assert n in rxa._SETTERS, n


def test_wisdom_returns_at_once_and_touches_no_file(qh, tmp_path):
    """WDSPwisdom is the first call of those clients: it returns like the reference's when its wisdom file was there, writes nothing into the
    directory it is given, ignores a null one and one that does not exist, and wisdom_get_status is a static NUL-terminated string"""
    lib = qh.load()
    assert lib.WDSPwisdom(None) is None
    assert lib.WDSPwisdom(str(tmp_path).encode() + b"/") is None
    assert os.listdir(str(tmp_path)) == []
    assert lib.WDSPwisdom(b"/nonexistent/directory/") is None
    s1 = lib.wisdom_get_status()
    assert isinstance(s1, bytes) and len(s1) < 128
    f = lib.wisdom_get_status
    keep = f.restype
    f.restype = C.c_void_p
    try:
        assert f() == f() and f() is not None       # one static buffer
    finally:
        f.restype = keep
