"""channel.c's run-time setters are in the built library (no GPU): the ten names a WDSP host binds (wdsp/channel.c:169-258,301-347) plus
SetType, the engine's nine entry points, each with a ctypes prototype in quisk_amd/lib.py and one declaration in include/quiskhip.h that
cites its lines of the reference; and the engine class carries the methods."""
import ctypes as C
import os

WDSP = {"SetInputBuffsize": [C.c_int] * 2, "SetDSPBuffsize": [C.c_int] * 2, "SetInputSamplerate": [C.c_int] * 2,
        "SetDSPSamplerate": [C.c_int] * 2, "SetOutputSamplerate": [C.c_int] * 2, "SetAllRates": [C.c_int] * 4,
        "SetChannelTDelayUp": [C.c_int, C.c_double], "SetChannelTSlewUp": [C.c_int, C.c_double],
        "SetChannelTDelayDown": [C.c_int, C.c_double], "SetChannelTSlewDown": [C.c_int, C.c_double]}
ENGINE_SET = {"qh_rxa_set_rates": 4, "qh_rxa_set_in_rate": 2, "qh_rxa_set_dsp_rate": 2, "qh_rxa_set_out_rate": 2, "qh_rxa_set_dsp_size": 2}
ENGINE_GET = ("qh_rxa_in_rate", "qh_rxa_dsp_rate", "qh_rxa_out_rate", "qh_rxa_dsp_size")
METHODS = ("set_rates", "set_in_rate", "set_dsp_rate", "set_out_rate", "set_dsp_size")


def test_the_names_are_exported_and_bound(qh):
    lib = qh.load()
    assert len(WDSP) == 10
    names = list(WDSP) + ["SetType"] + list(ENGINE_SET) + list(ENGINE_GET)
    missing = [n for n in names if not hasattr(lib, n)]
    assert not missing, missing
    unbound = [n for n in names if getattr(lib, n).argtypes is None]
    assert not unbound, unbound
    for n, sig in WDSP.items():
        assert list(getattr(lib, n).argtypes) == sig, n
        assert getattr(lib, n).restype is None, n       # the reference's are void
    assert list(lib.SetType.argtypes) == [C.c_int] * 2 and lib.SetType.restype is None
    for n, k in ENGINE_SET.items():
        a = list(getattr(lib, n).argtypes)
        assert a == [C.c_void_p] + [C.c_int] * (k - 1), n
    for n in ENGINE_GET:
        assert list(getattr(lib, n).argtypes) == [C.c_void_p] and getattr(lib, n).restype is C.c_int, n


def test_the_header_declares_them_with_their_reference_lines(qh):
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "quiskhip.h")).read()
    for n in list(WDSP) + ["SetType"] + list(ENGINE_SET) + list(ENGINE_GET):
        line = [ln for ln in header.splitlines() if (" " + n + "(") in ln]
        assert len(line) == 1, (n, line)
        assert "wdsp/channel.c:" in line[0], line[0]


def test_the_engine_class_has_the_methods(qh):
    for n in METHODS:
        assert callable(getattr(qh.RxaEngine, n, None)), n
    for n in ("in_rate", "dsp_rate", "out_rate", "dsp_size"):
        assert isinstance(getattr(qh.RxaEngine, n, None), property), n


def test_the_getters_answer_without_an_engine(qh):
    lib = qh.load()
    assert [getattr(lib, n)(None) for n in ENGINE_GET] == [0, 0, 0, 0]
    assert lib.qh_rxa_set_dsp_rate(None, 96000) != 0
