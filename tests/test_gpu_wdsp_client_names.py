"""The names piHPSDR, linHPSDR and Thetis call beside Quisk's, through the WDSP exports in the order such a client makes them: WDSPwisdom,
OpenChannel, SetRXAAGCThresh, SetRXAPanelPan, SetRXAPanelBinaural, RXANBPSetNC, SetRXABandpassWindow, fexchange0.  The getters return the
formulas' values (tests/wdsp_agc_knobs_ref.py), a refused value shows in qh_wdsp_status(), and the output is bit-equal to the same
settings made on a qh_rxa engine run inside the restated iobuffs (tests/wdsp_iobuffs_ref.py).  -m gpu.

Bit-equal, although the up-slew's raised cosine is computed twice (the library's and numpy's): the stream opens with one non-zero sample
and zeros for the rest of its first block, which the slew's delay and ramp (25 + 25 samples) turn into a block of zeros whatever the
cosine's last bits are; from the second block on the slew passes the samples as they are."""
import ctypes as C
import math

import numpy as np
import pytest

import wdsp_agc_knobs_ref as K
from wdsp_iobuffs_ref import Iobuffs

pytestmark = pytest.mark.gpu
D = C.c_double
CH, RATE, SIZE, NBLK = 9, 48000, 64, 70
SLEWS = dict(tdelayup=0.0005, tslewup=0.0005, tdelaydown=0.0, tslewdown=0.001)
BAND = (300.0, 3000.0)
FFT, FFT_RATE = 4096.0, 192000.0
THRESH, PAN = -100.0, 0.3


def signal():
    n = NBLK * SIZE
    t = np.arange(n) / float(RATE)
    rng = np.random.default_rng(12)
    env = 0.2 * (1.0 + 0.5 * np.sin(2.0 * np.pi * 9.0 * t))
    x = env * (np.exp(-2j * np.pi * 800.0 * t) + 0.4 * np.exp(-2j * np.pi * 2100.0 * t)) + 1e-4 * (rng.standard_normal(n) + 1j * rng.standard_normal(n))
    x[:SIZE] = 0.0
    x[0] = 1.0                                          # arms the up-slew; the delay swallows it
    return x


def client_calls(t, lead):
    """the settings, on the library's WDSP names (lead = [channel], doubles wrapped) or on an engine (lead = [0])"""
    d = D if lead[0] == CH else float
    t.SetRXAMode(*lead, 1)
    t.RXASetPassband(*lead, d(BAND[0]), d(BAND[1]))
    t.SetRXABandpassRun(*lead, 1)
    t.SetRXAAGCMode(*lead, 3)
    t.SetRXAAGCThresh(*lead, d(THRESH), d(FFT), d(FFT_RATE))
    t.SetRXAPanelPan(*lead, d(PAN))
    t.SetRXAPanelBinaural(*lead, 1)
    t.RXANBPSetNC(*lead, 1024)
    t.SetRXABandpassWindow(*lead, 0)


def test_a_pihpsdr_like_client(qh, tmp_path):
    lib = qh.load()
    for n, a in (("SetRXAMode", [C.c_int, C.c_int]), ("RXASetPassband", [C.c_int, D, D]), ("SetRXABandpassRun", [C.c_int, C.c_int]),
                 ("SetRXAAGCMode", [C.c_int, C.c_int]), ("SetRXAAGCHangThreshold", [C.c_int, C.c_int])):
        getattr(lib, n).argtypes = a
        getattr(lib, n).restype = None
    x = signal()
    lib.WDSPwisdom(str(tmp_path).encode() + b"/")
    assert lib.wisdom_get_status() == b""
    lib.OpenChannel(CH, SIZE, SIZE, RATE, RATE, RATE, 0, 1, D(SLEWS["tdelayup"]), D(SLEWS["tslewup"]), D(SLEWS["tdelaydown"]), D(SLEWS["tslewdown"]), 1)
    assert lib.qh_wdsp_status() == 0, lib.qh_last_error()
    try:
        client_calls(lib, [CH])
        assert lib.qh_wdsp_status() == 0, lib.qh_last_error()
        # the getters: the formulas' values
        v, k = D(0.0), C.c_int(0)
        g = K.thresh_to_max_gain(THRESH, FFT, FFT_RATE, band=BAND)
        lib.GetRXAAGCThresh(CH, C.byref(v), FFT, FFT_RATE)
        assert lib.qh_wdsp_status() == 0 and v.value == pytest.approx(THRESH, abs=1e-12)
        lib.GetRXAAGCTop(CH, C.byref(v))
        assert v.value == pytest.approx(20.0 * math.log10(g), abs=1e-12)
        lib.GetRXAAGCHangThreshold(CH, C.byref(k))
        assert k.value == 100                           # SetRXAAGCMode 3 sets hang_thresh 1.0 (wcpAGC.c:393)
        lib.GetRXAAGCHangLevel(CH, C.byref(v))
        assert v.value == pytest.approx(K.thresh_to_hang_level(1.0, max_gain=g), abs=1e-12)
        lib.SetRXAAGCHangLevel(CH, -20.0)
        lib.GetRXAAGCHangLevel(CH, C.byref(v))
        assert lib.qh_wdsp_status() == 0 and v.value == pytest.approx(-20.0, abs=1e-12)
        lib.SetRXAAGCHangThreshold(CH, 100)             # back to mode 3's
        # refused values show in qh_wdsp_status() and change nothing
        for call in (lambda: lib.SetRXAAGCThresh(CH, float("nan"), FFT, FFT_RATE), lambda: lib.SetRXAAGCThresh(CH, -90.0, 0.0, FFT_RATE),
                     lambda: lib.SetRXAAGCMaxInputLevel(CH, 0.0), lambda: lib.SetRXAPanelPan(CH, float("inf")),
                     lambda: lib.RXANBPSetNC(CH, 1000), lambda: lib.RXABPSNBASetNC(CH, 32), lambda: lib.SetRXABandpassNC(CH, 131072),
                     lambda: lib.SetRXABandpassWindow(CH, 2), lambda: lib.GetRXAAGCThresh(CH, C.byref(v), FFT, -1.0)):
            call()
            assert lib.qh_wdsp_status() != 0
        lib.GetRXAAGCTop(CH, C.byref(v))
        assert lib.qh_wdsp_status() == 0 and v.value == pytest.approx(20.0 * math.log10(g), abs=1e-12)
        # a channel that is not open: the status says so and the getter's result is left alone
        v.value = 123.0
        lib.GetRXAAGCTop(CH + 1, C.byref(v))
        assert lib.qh_wdsp_status() != 0 and v.value == 123.0
        # fexchange0
        got = []
        err = C.c_int(0)
        for b in range(NBLK):
            blk = np.ascontiguousarray(x[b * SIZE:(b + 1) * SIZE])
            out = np.full(SIZE, np.nan + 0j, dtype=np.complex128)
            lib.fexchange0(CH, blk.ctypes.data_as(C.c_void_p), out.ctypes.data_as(C.c_void_p), C.byref(err))
            assert lib.qh_wdsp_status() == 0, lib.qh_last_error()
            got.append(out)
    finally:
        lib.CloseChannel(CH)
    # the same settings on an engine, inside the restated iobuffs
    e = qh.RxaEngine(1, dsp_size=SIZE, in_rate=RATE, dsp_rate=RATE, out_rate=RATE)
    try:
        e.enable_meters(True)                           # WDSP's meters always run (OpenChannel)
        client_calls(e, [0])
        io = Iobuffs(lambda v: e.process_host(np.ascontiguousarray(v)[None, :])[0], SIZE, SIZE, RATE, RATE, RATE, **SLEWS)
        want = []
        for b in range(NBLK):
            y, _ = io.fexchange0(x[b * SIZE:(b + 1) * SIZE])
            want.append(y)
        assert io.upflag == 0
    finally:
        e.close()
    written = [b for b in range(NBLK) if not np.any(np.isnan(got[b]))]
    assert len(written) >= NBLK - 3 and written == list(range(written[0], NBLK))
    y, ref = np.concatenate([got[b] for b in written]), np.concatenate([want[b] for b in written])
    assert np.abs(ref[-20 * SIZE:]).max() > 0.05
    assert np.array_equal(y, ref)
    # pan 0.3 and binaural 1 are in it: Q = sin(0.3 PI) I's partner at gain2I = 1 (copy 0: I and Q are the chain's own)
    assert np.abs(y.imag).max() > 0.0 and not np.array_equal(y.real, y.imag)
