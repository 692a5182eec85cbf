"""The EMNR tables compiled into the library (quisk_amd/build.py: _emnr_tables_source -> qh_emnr_tables_gen.cpp) are WDSP's own compiled-in
fall-backs: wdsp/calculus.c (GG, GGS) and wdsp/zetahat.c, which emnr.c:207-225, 322-326 takes when `calculus` / `zetaHat.bin` are not in the
working directory."""
import hashlib
import json
import os
import re
import struct

import numpy as np


def _generated(tmp_path):
    from quisk_amd import build
    src = open(build._emnr_tables_source(str(tmp_path / "gen.cpp"))).read()
    out = {}
    for name, kind in (("kEmnrDefaultGG", "Q"), ("kEmnrDefaultGGS", "Q"), ("kEmnrDefaultZeta", "Q"), ("kEmnrDefaultRange", "Q"), ("kEmnrDefaultValid", "i")):
        body = re.search(name + r"\[\d+\] = \{(.*?)\};", src, re.S).group(1)
        toks = [t.strip() for t in body.replace("\n", " ").split(",") if t.strip()]
        if kind == "Q":
            out[name] = np.frombuffer(struct.pack("<%dQ" % len(toks), *[int(t[:-3], 16) for t in toks]), dtype="<f8")
        else:
            out[name] = np.array([int(t) for t in toks], dtype=np.int32)
    return out


def test_generated_tables_are_the_shipped_data(tmp_path):
    g = _generated(tmp_path)
    z = np.load(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "quisk_amd", "data", "wdsp_emnr_tables.npz"))
    assert np.array_equal(g["kEmnrDefaultGG"], z["GG"]) and np.array_equal(g["kEmnrDefaultGGS"], z["GGS"])
    assert np.array_equal(g["kEmnrDefaultValid"], z["zeta_valid"]) and np.array_equal(g["kEmnrDefaultRange"], z["zeta_range"])
    ok = z["zeta_valid"] > 0                                    # the cells getZeta reads (emnr.c:878-882)
    assert ok.sum() > 1000 and np.array_equal(g["kEmnrDefaultZeta"][ok], z["zeta_hat"][ok])
    none = z["zeta_hat"] == -1e300                              # the file's "no value" mark: 0 in the compiled-in table
    assert np.array_equal(g["kEmnrDefaultZeta"][~none], z["zeta_hat"][~none]) and not np.any(g["kEmnrDefaultZeta"][none]) and not np.any(ok & none)


def test_generated_tables_are_the_references_compiled_in_ones(tmp_path):
    """Pinned by tests/golden/emnr_tables_pin.json: the SHA-256 of the numbers of wdsp/calculus.c and wdsp/zetahat.c (little-endian float64,
    int32 for the valid flags) and the four range constants, read out of the reference files by tests/golden/make_emnr_tables_pin.py."""
    g = _generated(tmp_path)
    pin = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "emnr_tables_pin.json")))
    for key, name, dt in (("GG", "kEmnrDefaultGG", "<f8"), ("GGS", "kEmnrDefaultGGS", "<f8"), ("zeta", "kEmnrDefaultZeta", "<f8"),
                          ("valid", "kEmnrDefaultValid", "<i4")):
        a = np.ascontiguousarray(g[name], dtype=dt)
        assert a.size == pin[key]["count"] and hashlib.sha256(a.tobytes()).hexdigest() == pin[key]["sha256"], key
    assert list(g["kEmnrDefaultRange"]) == pin["range"]
