"""The fixed-ratio resampler's names are in the built library (no GPU): the V and FV names a WDSP caller binds (wdsp/resample.c:206-228,
332-354), the device hand-offs and the bank, each with a ctypes prototype in quisk_amd/lib.py and a declaration in the header; and the
Python class."""
import os
import re

V = ["create_resampleV", "xresampleV", "destroy_resampleV", "create_resampleFV", "xresampleFV", "destroy_resampleFV"]
DEVICE = ["qh_wdsp_xresampleV_device", "qh_wdsp_xresampleFV_device", "qh_wdsp_resampleV_max_out"]
BANK = ["qh_resample_create", "qh_resample_destroy", "qh_resample_set_run", "qh_resample_set_rates", "qh_resample_set_fc_low", "qh_resample_set_bandwidth",
        "qh_resample_flush", "qh_resample_L", "qh_resample_M", "qh_resample_cpp", "qh_resample_taps", "qh_resample_out_count", "qh_resample_max_out",
        "qh_resample_synchronize", "qh_resample_process", "qh_resample_process_host"]
HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "quiskhip.h")


def test_the_names_are_exported_and_bound(qh):
    lib = qh.load()
    missing = [n for n in V + DEVICE + BANK if not hasattr(lib, n)]
    assert not missing, missing
    unbound = [n for n in V + DEVICE + BANK if getattr(lib, n).argtypes is None]
    assert not unbound, unbound
    assert len(lib.create_resampleV.argtypes) == 2 and len(lib.xresampleV.argtypes) == 5 and len(lib.xresampleFV.argtypes) == 5
    assert len(lib.qh_resample_create.argtypes) == 9 and len(lib.qh_resample_process.argtypes) == 7
    assert len(lib.qh_wdsp_xresampleV_device.argtypes) == 6 and len(lib.qh_wdsp_xresampleFV_device.argtypes) == 6


def test_the_names_are_declared_with_the_reference_line_beside_them():
    header = open(HEADER).read()
    for n in V + DEVICE + BANK:
        assert re.search(r"\b%s\s*\(" % n, header), n
    for n, where in (("create_resampleV", "resample.c:208-212"), ("xresampleV", "resample.c:214-222"), ("destroy_resampleV", "resample.c:224-228"),
                     ("create_resampleFV", "resample.c:334-338"), ("xresampleFV", "resample.c:340-348"), ("destroy_resampleFV", "resample.c:350-354"),
                     ("qh_resample_flush", "resample.c:112-118"), ("qh_resample_set_fc_low", "resample.c:185-193"),
                     ("qh_resample_set_bandwidth", "resample.c:195-204")):
        line = [l for l in header.splitlines() if re.search(r"\b%s\s*\(" % n, l)][0]
        assert where in line, (n, line)
    assert "10f. WDSP's fixed-ratio resampler" in header


def test_the_struct_taking_names_are_not_provided(qh):
    lib = qh.load()
    for n in ("create_resample", "destroy_resample", "flush_resample", "xresample", "setFCLow_resample", "create_resampleF", "xresampleF"):
        assert not hasattr(lib, n), n
    assert "Not provided: create_resample, destroy_resample, flush_resample" in open(HEADER).read()


def test_the_python_class(qh):
    assert "WdspResampler" in qh.__all__
    for m in ("process_host", "process", "process_ptr", "max_out", "out_count", "set_run", "set_rates", "set_fc_low", "set_bandwidth", "flush", "L", "M",
              "cpp", "taps", "synchronize", "close"):
        assert hasattr(qh.WdspResampler, m), m
