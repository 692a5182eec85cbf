#!/usr/bin/env python3
"""Pins WDSP's compiled-in EMNR fall-back tables -- wdsp/calculus.c (GG, GGS) and wdsp/zetahat.c (zetaHatDefaultData / Valid and the
four range constants), which emnr.c:207-225, 322-326 takes when `calculus` / `zetaHat.bin` are not in the working directory.  Usage:
`make_emnr_tables_pin.py <reference tree>`.  Reads the numbers out of the reference files and writes their SHA-256 (little-endian
float64 / int32 bytes), their counts and the range constants -- numbers only, no source text -- to tests/golden/emnr_tables_pin.json,
which tests/test_emnr_builtin_tables.py compares with the tables the library compiles in."""
import hashlib
import json
import os
import re
import sys

import numpy as np


def sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def main(ref):
    cal = open(os.path.join(ref, "wdsp", "calculus.c")).read()
    nums = np.array([float(x) for x in re.findall(r"[-+]?\d+\.\d+(?:[eE][-+]?\d+)?", cal)], dtype="<f8")
    assert nums.size == 2 * 241 * 241
    zh = open(os.path.join(ref, "wdsp", "zetahat.c")).read()
    data = re.search(r"zetaHatDefaultData\s*\[[^\]]*\]\s*=\s*\{(.*?)\};", zh, re.S).group(1)
    valid = re.search(r"zetaHatDefaultValid\s*\[[^\]]*\]\s*=\s*\{(.*?)\};", zh, re.S).group(1)
    zeta = np.array([float(t) for t in data.replace("\n", " ").split(",")], dtype="<f8")
    ok = np.array([int(t) for t in valid.replace("\n", " ").split(",")], dtype="<i4")
    rng = [float(re.search(r"zetaHatDefault%s\s*=\s*([^;]+);" % k, zh).group(1)) for k in ("Gmin", "Gmax", "Ximin", "Ximax")]
    out = {"GG": {"count": 241 * 241, "sha256": sha(nums[:241 * 241])},
           "GGS": {"count": 241 * 241, "sha256": sha(nums[241 * 241:])},
           "zeta": {"count": int(zeta.size), "sha256": sha(zeta)},
           "valid": {"count": int(ok.size), "sha256": sha(ok)},
           "range": rng}
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "emnr_tables_pin.json")
    json.dump(out, open(path, "w"), indent=1, sort_keys=True)
    print(path, out)


if __name__ == "__main__":
    if len(sys.argv) != 2:
        raise SystemExit("usage: make_emnr_tables_pin.py <reference tree>")
    main(sys.argv[1])
