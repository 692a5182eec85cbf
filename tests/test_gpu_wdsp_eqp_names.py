"""The equalizer through the WDSP names (OpenChannel / SetRXAEQ* / SetRXAGrphEQ* / RXASetNC / RXASetMP / fexchange0), bound the way
quisk_wdsp.py binds libwdsp, against the restatement (tests/wdsp_eqp_ref.py).  -m gpu.

Two channels with the same settings, A with the equalizer and B without, fed the same blocks: both sit behind the same channel latency
and up-slew (wdsp/iobuffs.c), and behind the equalizer's spot their chains are linear (USB, fixed gain), so A = EQ_ref(B) once the slew
(35 ms) has left the equalizer's delay line -- the comparison starts 8192 output samples in.  The settings are made before the first block:
a setter acts on the block the DSP takes next, which the output shows a latency later."""
import ctypes as C

import numpy as np
import pytest

from conftest import rel_rms
from test_gpu_rxa_eqp import G10, G4, _signal
from wdsp_eqp_ref import Eqp

pytestmark = pytest.mark.gpu
D = C.c_double
FS, IN, OUT = 192000, 1024, 256
USB = 1
SKIP = 8192
NBLK = 96


def _open(lib, channel):
    lib.OpenChannel(channel, IN, 256, FS, 48000, 48000, 0, 1, D(0.010), D(0.025), D(0.0), D(0.010), 1)
    assert lib.qh_wdsp_status() == 0, lib.qh_last_error()
    lib.SetRXAShiftRun(channel, 0); lib.RXANBPSetRun(channel, 1); lib.SetRXAAMSQRun(channel, 0)
    lib.SetRXAMode(channel, USB)
    lib.RXASetPassband(channel, D(150.0), D(4000.0))
    lib.SetRXAAGCMode(channel, 0); lib.SetRXAAGCFixed(channel, D(10.0))
    lib.SetRXAPanelRun(channel, 0); lib.SetRXAEMNRRun(channel, 0)
    assert lib.qh_wdsp_status() == 0, lib.qh_last_error()


def _pair(lib, setup_a, setup_both=None):
    """the same blocks through A (channel 0, setup_a) and B (channel 1); returns (A's output, B's output)"""
    x = _signal(USB, 0, NBLK * IN, float(FS))
    for ch in (0, 1):
        _open(lib, ch)
    ya, yb = np.zeros(NBLK * OUT, dtype=np.complex128), np.zeros(NBLK * OUT, dtype=np.complex128)
    err = C.c_int(0)
    out = np.zeros(OUT, dtype=np.complex128)
    try:
        if setup_both:
            for ch in (0, 1):
                setup_both(lib, ch)
        setup_a(lib)
        assert lib.qh_wdsp_status() == 0, lib.qh_last_error()
        for b in range(NBLK):
            blk = np.ascontiguousarray(x[b * IN:(b + 1) * IN])
            for ch, y in ((0, ya), (1, yb)):
                lib.fexchange0(ch, blk.ctypes.data_as(C.c_void_p), out.ctypes.data_as(C.c_void_p), C.byref(err))
                assert err.value == 0 and lib.qh_wdsp_status() == 0, lib.qh_last_error()
                y[b * OUT:(b + 1) * OUT] = out
    finally:
        for ch in (0, 1):
            lib.CloseChannel(ch)
    return ya, yb


def _hold(ya, yb, ref, what):
    want = ref.process(yb)
    err = rel_rms(ya[SKIP:], want[SKIP:])
    print("%s through the WDSP names: relative RMS %.3g" % (what, err))
    assert np.any(want[SKIP:]) and err < 1e-9, err
    return want


def test_the_profile_setters_through_the_wdsp_names(qh):
    lib = qh.load()
    F, G = [0.0, 2500.0, 300.0, 900.0], [1.5, -8.0, 6.0, -3.0]              # unsorted, with a preamp

    def setup(lib):
        lib.SetRXAEQNC(0, 300)                                              # refused, reported through qh_wdsp_status, nothing changed
        assert lib.qh_wdsp_status() == -2
        lib.SetRXAEQNC(0, 1024); lib.SetRXAEQMP(0, 0)
        lib.SetRXAEQProfile(0, 3, (D * 4)(*F), (D * 4)(*G))
        lib.SetRXAEQCtfmode(0, 1); lib.SetRXAEQWintype(0, 1); lib.SetRXAEQRun(0, 1)

    ref = Eqp(48000, run=1)
    ref.SetRXAEQNC(1024); ref.SetRXAEQProfile(3, F, G); ref.SetRXAEQCtfmode(1); ref.SetRXAEQWintype(1)
    ya, yb = _pair(lib, setup)
    _hold(ya, yb, ref, "SetRXAEQProfile / NC / MP / Ctfmode / Wintype / Run")
    assert rel_rms(ya[SKIP:], yb[SKIP:]) > 1e-2


@pytest.mark.parametrize("which", ["SetRXAGrphEQ", "SetRXAGrphEQ10"])
def test_the_graphic_equalizers_through_the_wdsp_names(qh, which):
    lib = qh.load()
    g = G4 if which == "SetRXAGrphEQ" else G10

    def setup(lib):
        lib.SetRXAEQCtfmode(0, 1)                                           # the graphic setters put ctfmode back to 0 (eq.c:342,372)
        getattr(lib, which)(0, (C.c_int * len(g))(*g))
        lib.SetRXAEQRun(0, 1)

    ref = Eqp(48000, run=1)
    ref.SetRXAEQCtfmode(1)
    getattr(ref, which)(g)
    assert ref.ctfmode == 0
    ya, yb = _pair(lib, setup)
    _hold(ya, yb, ref, which)


def test_rxasetnc_and_rxasetmp_reach_the_equalizer(qh):
    """RXASetNC(4096) and RXASetMP(1) on both channels (RXA.c:941,954): A follows the restatement with nc 4096 and the minimum-phase taps
    the library designs for those settings (read from an engine of its own through debug_eqp), and not the one with nc 2048 and mp 0"""
    lib = qh.load()

    def setup_both(lib, ch):
        lib.RXASetNC(ch, 4096); lib.RXASetMP(ch, 1)

    def setup(lib):
        lib.SetRXAGrphEQ10(0, (C.c_int * 11)(*G10)); lib.SetRXAEQRun(0, 1)

    e = qh.RxaEngine(1, dsp_rate=48000, out_rate=48000)
    try:
        e.RXASetNC(0, 4096); e.RXASetMP(0, 1); e.SetRXAGrphEQ10(0, G10); e.SetRXAEQRun(0, 1)
        e.process_host(np.zeros((1, 1024), dtype=np.complex128))
        taps = e.debug_eqp(0)
    finally:
        e.close()
    assert taps is not None and len(taps) == 4096
    ref = Eqp(48000, run=1, nc=4096)
    ref.SetRXAGrphEQ10(G10)
    ref.mp = 1
    ref.use_taps(taps)
    ya, yb = _pair(lib, setup, setup_both)
    _hold(ya, yb, ref, "RXASetNC(4096) + RXASetMP(1)")
    old = Eqp(48000, run=1)
    old.SetRXAGrphEQ10(G10)
    assert rel_rms(ya[SKIP:], old.process(yb)[SKIP:]) > 1e-2
