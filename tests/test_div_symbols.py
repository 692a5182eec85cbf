"""The diversity combiner's names are in the built library (no GPU): the EXT names a WDSP caller binds (wdsp/div.c:104-187), the device
hand-off and the bank, each with a ctypes prototype in quisk_amd/lib.py and a declaration in the header; and the Python class."""
import os
import re

EXT = {"create_divEXT": "div.c:107-111", "destroy_divEXT": "div.c:113-117", "flush_divEXT": "div.c:119-123", "xdivEXT": "div.c:125-134",
       "SetEXTDIVRun": "div.c:137-144", "SetEXTDIVBuffsize": "div.c:147-154", "SetEXTDIVNr": "div.c:157-164", "SetEXTDIVOutput": "div.c:168-175",
       "SetEXTDIVRotate": "div.c:179-187"}
DEVICE = ["qh_wdsp_xdivEXT_device"]
BANK = ["qh_div_create", "qh_div_destroy", "qh_div_set_run", "qh_div_set_nr", "qh_div_set_output", "qh_div_set_rotate", "qh_div_get",
        "qh_div_synchronize", "qh_div_process", "qh_div_process_host"]
HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "quiskhip.h")


def test_the_names_are_exported_and_bound(qh):
    lib = qh.load()
    names = list(EXT) + DEVICE + BANK
    missing = [n for n in names if not hasattr(lib, n)]
    assert not missing, missing
    unbound = [n for n in names if getattr(lib, n).argtypes is None]
    assert not unbound, unbound
    assert len(lib.create_divEXT.argtypes) == 4 and len(lib.xdivEXT.argtypes) == 4 and len(lib.SetEXTDIVRotate.argtypes) == 4
    assert len(lib.qh_div_create.argtypes) == 5 and len(lib.qh_div_process.argtypes) == 7 and len(lib.qh_div_process_host.argtypes) == 7
    assert len(lib.qh_div_get.argtypes) == 7 and len(lib.qh_wdsp_xdivEXT_device.argtypes) == 5


def test_the_names_are_declared_with_the_reference_lines_beside_them():
    header = open(HEADER).read()
    for n in list(EXT) + DEVICE + BANK:
        assert re.search(r"\b%s\s*\(" % n, header), n
    for n, where in EXT.items():
        line = [l for l in header.splitlines() if re.search(r"\b%s\s*\(" % n, l)][0]
        assert "wdsp/" + where in line, (n, line)
    assert "10e. WDSP's diversity combiner (DIV)" in header
    assert "ids 0..31" in header and "array holds 2" in header                         # MAX_EXT_DIVS, div.c:104


def test_the_legacy_name_is_not_provided(qh):
    lib = qh.load()
    for n in ("xdivEXTF", "create_div", "xdiv", "flush_div"):
        assert not hasattr(lib, n), n
    assert "Not provided: xdivEXTF" in open(HEADER).read()


def test_the_python_class(qh):
    assert "WdspDiversity" in qh.__all__
    for m in ("set_run", "set_nr", "set_output", "set_rotate", "get", "process_ptr", "process_host", "synchronize", "close"):
        assert hasattr(qh.WdspDiversity, m), m
