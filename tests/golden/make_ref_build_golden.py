#!/usr/bin/env python3
"""Generates tests/golden/ref_build_golden.npz from the reference's own filter.c and quisk_wdsp.c (oracle/_ref, built by `make -C oracle
ref` from the reference tree where it lies), for the two tests that used to need that build at test time:

  tests/test_oracle_filter.py::test_bit_exact_against_reference_build -- filter.c's cDecimate / cDecim2HB45 outputs ("fir_<ntaps>_<d>_<lo>",
      "hb45_<lo>") on the test's seeded taps and input, call by call;
  tests/test_oracle_wdsp_shim.py -- quisk_wdsp.c's wdspFexchange0 over ragged calls ("shim_<in_size>_<in_rate>_*": the count each call
      returns, how many blocks it handed to fexchange0, and the SHA-256 of the whole work array afterwards, untouched tail included;
      then the same for one pass-through call with in_use = 0).

Inputs are regenerated from the same seeds by the tests; only outputs are stored."""
import ctypes as C
import hashlib
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from oracle import pyoracle as po                          # noqa: E402
import test_oracle_filter as tf                             # noqa: E402
import test_oracle_wdsp_shim as ts                          # noqa: E402


def sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def filter_outputs(g):
    for (ntaps, d), taps, x in tf.bit_exact_cases():
        f = po.RefFir(taps)
        for lo, hi in tf.BIT_EXACT_CUTS:
            g["fir_%d_%d_%d" % (ntaps, d, lo)] = f.cDecimate(x[lo:hi], d)
    h = po.RefHB45()
    x = tf.stream(5, 3001)
    g["hb45_0"], g["hb45_1001"] = h.cDecim2(x[:1001]), h.cDecim2(x[1001:])


def shim_outputs(g):
    L, ch = po.lib(), 3
    fx_t = C.CFUNCTYPE(None, C.c_int, C.c_void_p, C.c_void_p, C.POINTER(C.c_int))
    for in_size, in_rate in ts.PARAMS:
        chan = ts._channel(po, in_size, in_rate)
        calls = []

        def fexchange0(channel, pin, pout, perr):
            assert channel == ch
            calls.append(channel)
            L.wo_fexchange0(chan.h, pin, pout, perr)
        cb = fx_t(fexchange0)
        po.ref_wdsp_set_parameter(ch, in_size=in_size, fexchange0=C.cast(cb, C.c_void_p).value, in_use=1)
        ns, blocks, digests = [], [], []
        for k, a in ts.ragged_calls(in_size, in_rate):
            before = len(calls)
            ns.append(po.ref_wdsp_shim_lib().wdspFexchange0(ch, a.ctypes.data, k))
            blocks.append(len(calls) - before)
            digests.append(sha(a.view(np.float64)))
        # in_use = 0: the call that resets the ring (quisk_wdsp.c:33-38) -- also what keeps the next in_size from running past it
        po.ref_wdsp_set_parameter(ch, in_use=0)
        a = ts._input(in_rate)[:77].copy()
        key = "shim_%d_%d_" % (in_size, in_rate)
        g[key + "passthrough_n"] = np.array(po.ref_wdsp_shim_lib().wdspFexchange0(ch, a.ctypes.data, 77))
        g[key + "passthrough_sha256"] = np.array(sha(a.view(np.float64)))
        g[key + "n"], g[key + "blocks"], g[key + "sha256"] = np.array(ns), np.array(blocks), np.array(digests)


def main():
    po.build(ref=True)
    g = {}
    filter_outputs(g)
    shim_outputs(g)
    out = os.path.join(ROOT, "tests", "golden", "ref_build_golden.npz")
    np.savez_compressed(out, **g)
    print(out, os.path.getsize(out), "bytes;", len(g), "arrays")


if __name__ == "__main__":
    main()
