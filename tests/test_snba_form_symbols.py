"""qh_rxa_set_snba_form / qh_rxa_snba_form (the selectable form of xsnba): exported by the library, declared in include/quiskhip.h and
bound in Python (quisk_amd/lib.py, RxaEngine).  No GPU needed: the library loads without one."""
import ctypes as C
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("qh_rxa_set_snba_form", "qh_rxa_snba_form")


def test_the_names_are_exported(qh):
    lib = qh.load()
    for name in NAMES:
        assert getattr(lib, name) is not None, name


def test_the_names_are_declared_in_the_header():
    text = open(os.path.join(ROOT, "include", "quiskhip.h")).read()
    assert re.search(r"\bint\s+qh_rxa_set_snba_form\s*\(\s*qh_rxa\s*\*\s*\w+\s*,\s*int\s+\w+\s*\)\s*;", text)
    assert re.search(r"\bint\s+qh_rxa_snba_form\s*\(\s*const\s+qh_rxa\s*\*\s*\w+\s*\)\s*;", text)


def test_the_names_are_bound_in_python(qh):
    lib = qh.load()
    assert lib.qh_rxa_set_snba_form.argtypes == [C.c_void_p, C.c_int]
    assert lib.qh_rxa_snba_form.argtypes == [C.c_void_p]
    assert callable(getattr(qh.RxaEngine, "set_snba_form")) and callable(getattr(qh.RxaEngine, "snba_form"))
    # a null engine: the setter reports it, the getter answers the default form
    assert lib.qh_rxa_set_snba_form(None, 1) != 0 and lib.qh_rxa_snba_form(None) == 0
