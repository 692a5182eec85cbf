"""The variable-ratio resampler's names are in the built library (no GPU): the V names a WDSP caller binds (wdsp/varsamp.c:228-250), the
device hand-off and the bank, each with a ctypes prototype in quisk_amd/lib.py and a declaration in the header; and the Python class."""
import os
import re

V = ["create_varsampV", "xvarsampV", "destroy_varsampV", "qh_wdsp_xvarsampV_device", "qh_wdsp_varsampV_max_out"]
BANK = ["qh_varsamp_create", "qh_varsamp_destroy", "qh_varsamp_flush", "qh_varsamp_set_run", "qh_varsamp_set_varmode", "qh_varsamp_set_rates",
        "qh_varsamp_set_bandwidth", "qh_varsamp_rsize", "qh_varsamp_synchronize", "qh_varsamp_max_out", "qh_varsamp_process", "qh_varsamp_process_host"]
HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "quiskhip.h")


def test_the_names_are_exported_and_bound(qh):
    lib = qh.load()
    missing = [n for n in V + BANK if not hasattr(lib, n)]
    assert not missing, missing
    unbound = [n for n in V + BANK if getattr(lib, n).argtypes is None]
    assert not unbound, unbound
    assert len(lib.create_varsampV.argtypes) == 3 and len(lib.xvarsampV.argtypes) == 6 and len(lib.qh_varsamp_create.argtypes) == 11
    assert len(lib.qh_varsamp_process.argtypes) == 8 and len(lib.qh_wdsp_xvarsampV_device.argtypes) == 7


def test_the_names_are_declared_with_the_reference_line_beside_them():
    header = open(HEADER).read()
    for n in V + BANK:
        assert re.search(r"\b%s\s*\(" % n, header), n
    for n, where in (("create_varsampV", "varsamp.c:230-234"), ("xvarsampV", "varsamp.c:236-244"), ("destroy_varsampV", "varsamp.c:246-250"),
                     ("qh_varsamp_flush", "varsamp.c:104-110")):
        line = [l for l in header.splitlines() if re.search(r"\b%s\s*\(" % n, l)][0]
        assert where in line, (n, line)
    assert "10d. WDSP's variable-ratio resampler" in header


def test_rmatch_is_not_provided(qh):
    lib = qh.load()
    for n in ("create_rmatchV", "xrmatchIN", "xrmatchOUT", "destroy_rmatchV", "create_varsamp", "xvarsamp"):
        assert not hasattr(lib, n), n
    assert "Not provided: rmatch.c" in open(HEADER).read()


def test_the_python_class(qh):
    assert "WdspVarResampler" in qh.__all__
    for m in ("process_host", "process_ptr", "max_out", "set_run", "set_varmode", "set_rates", "set_bandwidth", "flush", "rsize", "synchronize", "close"):
        assert hasattr(qh.WdspVarResampler, m), m
