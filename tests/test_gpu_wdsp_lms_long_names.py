"""ANF / ANR beyond 64 taps under the WDSP names (SetRXAANRVals, SetRXAANFTaps ... of include/quiskhip.h, bound as quisk_wdsp.py binds
libwdsp), block at a time through fexchange0 against the oracle's, and a value outside the delay line refused where a WDSP caller can
see it: qh_wdsp_status().  Input, guard and gate are tests/test_gpu_rxa_lms_long.py's.  -m gpu."""
import ctypes as C

import numpy as np
import pytest

from conftest import rel_rms
from quisk_amd import synth
from test_gpu_rxa_lms_long import GATE, GUARD, _perturbed, _x
from test_gpu_wdsp_dropin import _open, _oracle, _run

pytestmark = pytest.mark.gpu
QH_ERR_INVALID = -2
IN, OUT = 1024, 256
SPANS = ((0, 20), (20, 40), (40, 50))


def _bind(lib):
    for f in ("ANF", "ANR"):
        for n in ("Run", "Taps", "Delay", "Position"):
            getattr(lib, "SetRXA%s%s" % (f, n)).argtypes = [C.c_int, C.c_int]
        getattr(lib, "SetRXA%sVals" % f).argtypes = [C.c_int, C.c_int, C.c_int, C.c_double, C.c_double]


def _reference(oracle, x):
    """ANR 256 / 32 from the start, ANF 128 / 16 from block 20 on; nothing new at block 40, where the names refuse a value"""
    o = _oracle(oracle, IN, 256, 192000, True, shift_freq=synth.shift_freq(0))
    o.SetRXAANRVals(256, 32, 2e-4, 0.05); o.SetRXAANRRun(1)
    out = [o.fexchange0(x[SPANS[0][0] * IN:SPANS[0][1] * IN])[0]]
    o.SetRXAANFVals(128, 16, 1e-4, 0.1); o.SetRXAANFRun(1)           # SetRXAANFTaps: the oracle binds Vals alone, the same flush
    out += [o.fexchange0(x[a * IN:b * IN])[0] for a, b in SPANS[1:]]
    return out


def test_long_filters_and_a_refusal_through_the_wdsp_names(qh, oracle):
    lib = qh.load()
    _bind(lib)
    x = _x()[0]
    ref = _reference(oracle, x)
    assert rel_rms(np.concatenate(_reference(oracle, _perturbed(x))), np.concatenate(ref)) < GUARD
    ch = 9
    _open(lib, ch, IN, 256, 192000, True, shift_freq=synth.shift_freq(0))
    try:
        lib.SetRXAANRVals(ch, 256, 32, 2e-4, 0.05); lib.SetRXAANRRun(ch, 1)
        assert lib.qh_wdsp_status() == 0, lib.qh_last_error()
        y = [_run(lib, ch, x[SPANS[0][0] * IN:SPANS[0][1] * IN], IN, OUT)]
        lib.SetRXAANFTaps(ch, 128); lib.SetRXAANFRun(ch, 1)
        assert lib.qh_wdsp_status() == 0, lib.qh_last_error()
        y.append(_run(lib, ch, x[SPANS[1][0] * IN:SPANS[1][1] * IN], IN, OUT))
        for name, v in (("SetRXAANFTaps", 2049), ("SetRXAANRTaps", 0), ("SetRXAANRDelay", 2048), ("SetRXAANFDelay", -1)):
            getattr(lib, name)(ch, v)
            assert lib.qh_wdsp_status() == QH_ERR_INVALID, (name, v)
            assert b"taps 1..2048, delay 0..2047" in lib.qh_last_error()
        lib.SetRXAANFVals(ch, 4096, 16, 1e-4, 0.1)
        assert lib.qh_wdsp_status() == QH_ERR_INVALID
        lib.SetRXAANFRun(ch, 1)                     # an accepted setter clears the status (run as it was: no flush, anf.c:170)
        assert lib.qh_wdsp_status() == 0
        y.append(_run(lib, ch, x[SPANS[2][0] * IN:SPANS[2][1] * IN], IN, OUT))
    finally:
        lib.CloseChannel(ch)
    errs = [rel_rms(a, b) for a, b in zip(y, ref)]
    print("ANR 256/32, + ANF 128/16, behind the refusals: %s" % " ".join("%.1e" % e for e in errs), flush=True)
    assert max(errs) < GATE, errs
