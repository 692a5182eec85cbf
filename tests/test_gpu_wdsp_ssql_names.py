"""xssql through the WDSP names (OpenChannel, fexchange0, SetRXASSQLRun / Threshold / TauMute / TauUnMute) against the restatement
(tests/rxa_ssql_ref.py) applied to a WDSP channel without the squelch and with an identity panel, the default panel following.  A
setter reaches the samples of the block it precedes, which leave fexchange0 LAT blocks later (the exchange's two-block latency,
test_gpu_wdsp_dropin.py): the restatement takes it there.  -m gpu."""
import ctypes as C

import numpy as np
import pytest

from conftest import rel_rms
from quisk_amd import synth
from rxa_audio_peak_ref import panel
from rxa_ssql_ref import Ssql, edges, syllabic

pytestmark = pytest.mark.gpu
D = C.c_double
IN, OUT = 1024, 256
LAT = 2


def _open(lib, ch, shift):
    lib.OpenChannel(ch, IN, 256, 192000, 48000, 48000, 0, 1, D(0.010), D(0.025), D(0.0), D(0.010), 1)
    lib.SetRXAShiftRun(ch, 1)
    lib.SetRXAShiftFreq(ch, D(shift))
    lib.RXANBPSetRun(ch, 1)
    lib.SetRXAMode(ch, 1)
    lib.RXASetPassband(ch, D(300.0), D(3000.0))
    assert lib.qh_wdsp_status() == 0, lib.qh_last_error()


def _block(lib, ch, x):
    out = np.zeros(OUT, dtype=np.complex128)
    err = C.c_int(0)
    blk = np.ascontiguousarray(x)
    lib.fexchange0(ch, blk.ctypes.data_as(C.c_void_p), out.ctypes.data_as(C.c_void_p), C.byref(err))
    assert err.value == 0
    return out


def test_names_against_restatement(qh):
    lib = qh.load()
    A, B = 5, 6
    shift = synth.shift_freq(0)
    for ch in (A, B):
        _open(lib, ch, shift)
    lib.SetRXAPanelGain1(B, D(1.0))
    ref = Ssql(48000)
    script = {0: [("SetRXASSQLRun", (1,))], 300: [("SetRXASSQLThreshold", (0.2,))], 500: [("SetRXASSQLTauMute", (0.2,))],
              700: [("SetRXASSQLTauUnMute", (0.05,))], 800: [("SetRXASSQLRun", (0,))], 840: [("SetRXASSQLRun", (1,))]}
    nblk = 1300
    t = np.arange(nblk * IN) / 192000.0
    x = 0.3 * syllabic(nblk * IN, 192000.0, seed=3) * np.exp(-2j * np.pi * ((shift * t) % 1.0))
    ya, yr, gr = [], [], []
    pending = {}
    launches0 = lib.qh_wdsp_graph_launches()
    try:
        for k in range(nblk):
            for name, args in script.get(k, []):
                getattr(lib, name)(A, *[D(v) if isinstance(v, float) else v for v in args])
                assert lib.qh_wdsp_status() == 0, (name, lib.qh_last_error())
                pending.setdefault(k + LAT, []).append((name, args))
            blk = x[k * IN:(k + 1) * IN]
            ya.append(_block(lib, A, blk))
            for name, args in pending.pop(k, []):
                getattr(ref, name)(*args)
            yr.append(panel(ref.process(_block(lib, B, blk))))
            gr.append(ref.gain)
        ya, yr, gr = np.concatenate(ya), np.concatenate(yr), np.concatenate(gr)
        op, cl = edges(gr)
        assert op >= 2 and cl >= 2, (op, cl)
        assert not np.any(ya[gr == 0.0])
        assert rel_rms(ya, yr) < 1e-9, rel_rms(ya, yr)
        # OpenChannel switches the launch replay on: what was compared above came out of replayed graphs, not plain launches only.
        # Parameters stood still for every call but the ones behind a setter (A's six; B has none): at least half of those replayed
        steady = 2 * nblk - len(script)
        assert lib.qh_wdsp_graph_launches() - launches0 >= steady // 2, (lib.qh_wdsp_graph_launches() - launches0, steady)
    finally:
        lib.CloseChannel(A)
        lib.CloseChannel(B)


def test_names_refused_values_reported(qh):
    lib = qh.load()
    ch = 7
    _open(lib, ch, synth.shift_freq(0))
    try:
        lib.SetRXASSQLTauMute(ch, D(-1.0))
        assert lib.qh_wdsp_status() != 0
        lib.SetRXASSQLThreshold(ch, D(float("nan")))
        assert lib.qh_wdsp_status() != 0
        lib.SetRXASSQLTauUnMute(ch, D(0.0))
        assert lib.qh_wdsp_status() == 0
    finally:
        lib.CloseChannel(ch)
