"""The FM squelch through the WDSP names (OpenChannel / SetRXAMode / SetRXAFMSQ* / RXASetNC / fexchange0), bound the way quisk_wdsp.py binds
libwdsp, against the restatement (tests/wdsp_fmsq_ref.py).  -m gpu.

Three channels as in tests/test_gpu_rxa_fmsq.py: A with the squelch, C without, B in mode SPEC with an identity panel, all three behind
the same channel latency and up-slew (wdsp/iobuffs.c), so the restatement's gain, made from B's output, lines up with C's output sample for
sample.  The carrier comes on after 1.5 s here: B's output is slewed over its first 35 ms, so the trigger made from it is not the chain's
there, and longnoise (tau 0.1 s) must have forgotten that before the first tail count is taken from it (e^-23 by then).  The engine's own
state runs ahead of the delayed output by the latency, so the states are not compared here."""
import ctypes as C

import numpy as np
import pytest

from conftest import rel_rms
from wdsp_fmsq_ref import FmLoop, Fmsq, keyed_fm, margins

pytestmark = pytest.mark.gpu
D = C.c_double
FS, IN, OUT = 192000, 1024, 256
FM, SPEC = 5, 8


def _open(lib, channel, mode):
    lib.OpenChannel(channel, IN, 256, FS, 48000, 48000, 0, 1, D(0.010), D(0.025), D(0.0), D(0.010), 1)
    assert lib.qh_wdsp_status() == 0, lib.qh_last_error()
    lib.SetRXAShiftRun(channel, 0); lib.RXANBPSetRun(channel, 1); lib.SetRXAAMSQRun(channel, 0)
    lib.SetRXAMode(channel, mode)
    lib.RXASetPassband(channel, D(-8000.0), D(8000.0))
    lib.SetRXAAGCMode(channel, 0); lib.SetRXAAGCFixed(channel, D(0.0))
    lib.SetRXAPanelRun(channel, 0); lib.SetRXAEMNRRun(channel, 0)
    assert lib.qh_wdsp_status() == 0, lib.qh_last_error()


def _three(lib, x, setup, ref):
    """x through A (channel 0, squelch on), C (1) and B (2); returns (A's output, the restated g C, the restated gain, margins)"""
    for ch, mode in ((0, FM), (1, FM), (2, SPEC)):
        _open(lib, ch, mode)
    nb = x.size // IN
    ya, yr, gs = np.zeros(nb * OUT, dtype=np.complex128), [], []
    loop = FmLoop(48000.0)
    cross, tail, last = np.inf, np.inf, None
    err = C.c_int(0)
    blk_out = [np.zeros(OUT, dtype=np.complex128) for _ in range(3)]
    try:
        setup(lib)
        assert lib.qh_wdsp_status() == 0, lib.qh_last_error()
        for b in range(nb):
            blk = np.ascontiguousarray(x[b * IN:(b + 1) * IN])
            for ch in range(3):
                lib.fexchange0(ch, blk.ctypes.data_as(C.c_void_p), blk_out[ch].ctypes.data_as(C.c_void_p), C.byref(err))
                assert err.value == 0 and lib.qh_wdsp_status() == 0, lib.qh_last_error()
            ya[b * OUT:(b + 1) * OUT] = blk_out[0]
            yr.append(ref.process(loop.process(blk_out[2]), blk_out[1]))
            gs.append(ref.gain)
            av = ref.av if last is None else np.concatenate([[last], ref.av])
            cr, tl = margins(av, (ref.tail_thresh, ref.unmute_thresh), ref.tails)
            cross, tail, last = min(cross, cr), min(tail, tl), ref.av[-1]
    finally:
        for ch in range(3):
            lib.CloseChannel(ch)
    return ya, np.concatenate(yr), np.concatenate(gs), cross, tail


def _check(ya, yr, g, cross, tail):
    print("crossing margin %.3g, tail margin %.3g" % (cross, tail))
    assert cross > 1e-6 and tail > 1e-3, (cross, tail)
    assert np.sum((g[:-1] == 0.0) & (g[1:] != 0.0)) >= 1 and np.sum((g[:-1] != 0.0) & (g[1:] == 0.0)) >= 1      # opens and closes
    muted = g == 0.0
    assert not np.any(ya[muted]), int(np.sum(ya[muted] != 0))
    err = rel_rms(ya, yr)
    print("A against g C through the WDSP names: relative RMS %.3g" % err)
    assert err < 1e-9, err


@pytest.fixture(scope="module")
def late_carrier():
    return keyed_fm(int(3.4 * FS) // IN * IN, FS, seed=3, off=1.5, on=0.9)


def test_the_squelch_through_the_wdsp_names(qh, late_carrier):
    lib = qh.load()

    def setup(lib):
        lib.SetRXAFMSQThreshold(0, D(0.7)); lib.SetRXAFMSQMP(0, 0); lib.SetRXAFMSQNC(0, 1024); lib.SetRXAFMSQRun(0, 1)

    ref = Fmsq(48000, run=1, nc=1024)
    ref.SetRXAFMSQThreshold(0.7)
    _check(*_three(lib, late_carrier, setup, ref))


def test_rxasetnc_moves_the_squelchs_nc(qh, late_carrier):
    """RXASetNC forwards to SetRXAFMSQNC (RXA.c:942): the output follows the restatement at the new nc (512), which it does not at the old"""
    lib = qh.load()

    def setup(lib):
        for ch in range(3):
            lib.RXASetNC(ch, 512)
        lib.SetRXAFMSQThreshold(0, D(float("nan")))             # refused, reported through qh_wdsp_status, nothing changed
        assert lib.qh_wdsp_status() == -2
        lib.SetRXAFMSQRun(0, 1)

    ya, yr, g, cross, tail = _three(lib, late_carrier, setup, Fmsq(48000, run=1, nc=512))
    _check(ya, yr, g, cross, tail)
    old = Fmsq(48000, run=1, nc=2048)
    assert (old.nc - 1) // 2 - (512 - 1) // 2 > 700              # the two filters' delays differ by 768 samples: the gains cannot agree
