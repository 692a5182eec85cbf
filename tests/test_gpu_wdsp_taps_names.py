"""SetRXASpectrum, RXAGetaSipF and RXAGetaSipF1 bound as a WDSP caller binds them (wdsp/sender.c:111-122, wdsp/siphon.c:182-211).

Channel 0's DSP blocks feed display 3 on the device; the rows GetPixels hands out are held to the gates of tests/test_gpu_analyzer.py
against oracle.OracleAnalyzer fed with the oracle fexchange0's own signal behind nbp0 (HOOK_FMSQ), and RXAGetaSipF1's float pairs to
2^-23 relative RMS (one float ulp) against the restated siphon on its HOOK_AUDIO capture.  -m gpu."""
import ctypes as C

import numpy as np
import pytest

from conftest import rel_rms
from quisk_amd import synth
from rxa_taps_ref import Siphon
from rxa_taps_util import ARGS, NPIX, SIZE, compare_rows, oracle_rows, signal

pytestmark = pytest.mark.gpu
D = C.c_double
ULP = 2.0 ** -23
DISP = 3


def _open(lib, ch):
    lib.OpenChannel(ch, 1024, 256, 192000, 48000, 48000, 0, 1, D(0.010), D(0.025), D(0.0), D(0.010), 1)
    assert lib.qh_wdsp_status() == 0, lib.qh_last_error()
    lib.SetRXAShiftRun(ch, 1); lib.SetRXAShiftFreq(ch, D(synth.shift_freq(ch))); lib.RXANBPSetRun(ch, 1)
    lib.SetRXAMode(ch, 1); lib.RXASetPassband(ch, D(300.0), D(3000.0))
    lib.SetRXAAGCMode(ch, 0); lib.SetRXAAGCFixed(ch, D(6.0))
    assert lib.qh_wdsp_status() == 0, lib.qh_last_error()


def _oracle(po, ch):
    o = po.WdspChannel(1024, 256, 192000, 48000, 48000)
    o.SetRXAShiftRun(1); o.SetRXAShiftFreq(synth.shift_freq(ch)); o.RXANBPSetRun(1)
    o.SetRXAMode(1); o.RXASetPassband(300.0, 3000.0)
    o.SetRXAAGCMode(0); o.SetRXAAGCFixed(6.0)
    return o


def _blocks(lib, ch, x, each=None):
    out = np.zeros(x.size // 4, dtype=np.complex128)
    err = C.c_int(0)
    for b in range(x.size // 1024):
        blk = np.ascontiguousarray(x[b * 1024:(b + 1) * 1024])
        lib.fexchange0(ch, blk.ctypes.data_as(C.c_void_p), out[b * 256:].ctypes.data_as(C.c_void_p), C.byref(err))
        assert err.value == 0
        if each:
            each(b)
    return out


def _pixels(lib):
    pix, flag = np.zeros(NPIX, dtype=np.float32), C.c_int(0)
    lib.GetPixels(DISP, 0, pix.ctypes.data_as(C.c_void_p), C.byref(flag))
    return pix if flag.value else None


def _sip(lib, ch, size, iq=True):
    out = np.full(2 * size if iq else size, 7.0, dtype=np.float32)
    (lib.RXAGetaSipF1 if iq else lib.RXAGetaSipF)(ch, out.ctypes.data_as(C.c_void_p), size)
    return out


def test_the_three_names(qh, oracle):
    lib = qh.load()
    x = signal([1, 1], 72 * 1024, seed=12)
    ok = C.c_int(-1)
    _open(lib, 0); _open(lib, 1)
    try:
        lib.XCreateAnalyzer(DISP, C.byref(ok), SIZE, 1, 1, b"")
        assert ok.value == 0
        lib.SetDisplaySampleRate(DISP, 48000)
        lib.SetAnalyzer(DISP, *ARGS[:3], (C.c_int * 1)(0), *ARGS[4:])
        lib.SetRXASpectrum(0, 1, DISP, 0, 0)
        assert lib.qh_wdsp_status() == 0, lib.qh_last_error()
        # the oracle's fexchange0 over the same input: its DSP blocks' signal behind nbp0 and behind the AGC
        o = _oracle(oracle, 0)
        mid, aud = [], []
        o.set_stage_hook(lambda w, z, a: (mid if w == 0 else aud).append(z.copy()), sites=(0, 2))
        ref_out, _ = o.fexchange0(x[0, :44 * 1024])
        # 24 blocks with the sender on
        launches = lib.qh_wdsp_graph_launches()
        rows = []
        y = _blocks(lib, 0, x[0, :24 * 1024], each=lambda b: rows.append(_pixels(lib)))
        assert lib.qh_wdsp_status() == 0, lib.qh_last_error()
        rows = np.array([r for r in rows if r is not None])
        compare_rows(rows, oracle_rows(oracle, np.concatenate(mid[:24])), "GetPixels")
        assert lib.qh_wdsp_graph_launches() > launches
        assert rel_rms(y, ref_out[:24 * 256]) < 1e-9
        # channel 1: accepted, feeds nothing
        lib.SetRXASpectrum(1, 1, DISP, 0, 0)
        assert lib.qh_wdsp_status() == 0
        _blocks(lib, 1, x[1, :8 * 1024])
        assert _pixels(lib) is None
        # RXAGetaSipF1: the first call switches the siphon on and returns a flushed siphon's zeros
        assert not np.any(_sip(lib, 0, 4096))
        assert lib.qh_wdsp_status() == 0, lib.qh_last_error()
        # flag 0 stops the feed; 20 more blocks fill the siphon
        lib.SetRXASpectrum(0, 0, DISP, 0, 0)
        y2 = _blocks(lib, 0, x[0, 24 * 1024:44 * 1024])
        assert _pixels(lib) is None
        assert rel_rms(y2, ref_out[24 * 256:]) < 1e-9
        sip = Siphon(256)
        sip.push(np.concatenate(aud[24:44]))
        for size in (1, 256, 4096):
            got = _sip(lib, 0, size).view(np.complex64)
            r = rel_rms(got, sip.suck(size).astype(np.complex64))
            print("RXAGetaSipF1", size, r)
            assert r < ULP, (size, r)
            assert np.array_equal(_sip(lib, 0, size, iq=False), got.real)
        keep = _sip(lib, 0, 16)
        out = np.full(2 * 4097, 7.0, dtype=np.float32)
        lib.RXAGetaSipF1(0, out.ctypes.data_as(C.c_void_p), 4097)
        assert lib.qh_wdsp_status() != 0 and np.all(out == 7.0)
        assert np.array_equal(_sip(lib, 0, 16), keep)
        # a display that was never created: an error in qh_wdsp_status(), the audio as it was
        lib.SetRXASpectrum(0, 1, 9, 0, 0)
        y3 = _blocks(lib, 0, x[0, 44 * 1024:52 * 1024])
        assert lib.qh_wdsp_status() != 0
        ref3, _ = o.fexchange0(x[0, 44 * 1024:52 * 1024])
        assert rel_rms(y3, ref3) < 1e-9
        # DestroyAnalyzer between blocks leaves nothing dangling
        lib.SetRXASpectrum(0, 1, DISP, 0, 0)
        _blocks(lib, 0, x[0, 52 * 1024:56 * 1024])
        assert lib.qh_wdsp_status() == 0, lib.qh_last_error()
        lib.DestroyAnalyzer(DISP)
        _blocks(lib, 0, x[0, 56 * 1024:60 * 1024])
        assert lib.qh_wdsp_status() != 0
        o.close()
    finally:
        lib.CloseChannel(0); lib.CloseChannel(1)
        lib.DestroyAnalyzer(DISP)
