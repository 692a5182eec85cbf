"""The second blanker's names are in the built library (no GPU): the EXT names a WDSP caller binds (wdsp/nobII.c:605-734), the device
hand-off and the bank, each with a ctypes prototype in quisk_amd/lib.py; and the Python class stands beside WdspNoiseBlanker."""
import os

EXT = ["create_nobEXT", "destroy_nobEXT", "flush_nobEXT", "xnobEXT", "SetEXTNOBRun", "SetEXTNOBMode", "SetEXTNOBBuffsize", "SetEXTNOBSamplerate",
       "SetEXTNOBTau", "SetEXTNOBHangtime", "SetEXTNOBAdvtime", "SetEXTNOBBacktau", "SetEXTNOBThreshold", "qh_wdsp_xnobEXT_device"]
BANK = ["qh_nob_create", "qh_nob_destroy", "qh_nob_delay", "qh_nob_set_run", "qh_nob_set_mode", "qh_nob_set_samplerate", "qh_nob_set_tau",
        "qh_nob_set_hangtime", "qh_nob_set_advtime", "qh_nob_set_backtau", "qh_nob_set_threshold", "qh_nob_flush", "qh_nob_process",
        "qh_nob_process_host", "qh_nob_synchronize"]


def test_the_names_are_exported_and_bound(qh):
    lib = qh.load()
    missing = [n for n in EXT + BANK if not hasattr(lib, n)]
    assert not missing, missing
    unbound = [n for n in EXT + BANK if getattr(lib, n).argtypes is None]
    assert not unbound, unbound
    assert len(lib.create_nobEXT.argtypes) == 10 and len(lib.qh_nob_create.argtypes) == 10


def test_the_legacy_and_pointer_names_are_not_provided(qh):
    lib = qh.load()
    for n in ("xnobEXTF", "pSetRCVRNOBRun", "pSetRCVRNOBMode", "pSetRCVRNOBThreshold"):
        assert not hasattr(lib, n), n
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "quiskhip.h")).read()
    assert "Not provided: xnobEXTF" in header and "pSetRCVRNOB*" in header


def test_the_python_class_stands_beside_the_first_blanker(qh):
    assert "WdspNoiseBlanker2" in qh.__all__
    a, b = qh.WdspNoiseBlanker, qh.WdspNoiseBlanker2
    shapes = [m for m in dir(a) if not m.startswith("_")]
    assert all(hasattr(b, m) for m in shapes) and hasattr(b, "set_mode") and not hasattr(a, "set_mode")
