"""xcbl / xspeak / xmpeak through the WDSP names (OpenChannel, fexchange0, SetRXACBLRun / SetRXASPCW* / SetRXAmpeak*) against the
restatement (tests/rxa_audio_peak_ref.py) applied to a WDSP channel without the stages.  The up-slew acts on the input, ahead of the
chain, and the stages sit behind everything else, so the restated stages applied to the stage-off channel's fexchange0 output (its
leading zeros included) is the stage-on channel's output.  A setter reaches the samples of the block it precedes, which leave
fexchange0 LAT blocks later (the exchange's two-block latency, test_gpu_wdsp_dropin.py): the restatement takes it there.  -m gpu."""
import ctypes as C

import numpy as np
import pytest

from conftest import rel_rms
from quisk_amd import synth
from rxa_audio_peak_ref import AudioPeakChain

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


def test_names_seeded_walk_against_restatement(qh):
    lib = qh.load()
    A, B = 5, 6
    shift = synth.shift_freq(0)
    for ch in (A, B):
        _open(lib, ch, shift)
    ref = AudioPeakChain(48000.0)
    # (name, args) applied to A and the restatement; the others to A and B alike
    new = [("SetRXASPCWRun", (1,)), ("SetRXASPCWFreq", (650.0,)), ("SetRXASPCWBandwidth", (60.0,)), ("SetRXASPCWGain", (1.2,)),
           ("SetRXAmpeakRun", (1,)), ("SetRXAmpeakFilFreq", (0, 900.0)), ("SetRXAmpeakFilBw", (1, 90.0)), ("SetRXAmpeakFilGain", (1, 1.8)),
           ("SetRXAmpeakFilEnable", (0, 0)), ("SetRXAmpeakFilEnable", (0, 1)), ("SetRXAmpeakNpeaks", (1,)), ("SetRXAmpeakNpeaks", (2,)),
           ("SetRXACBLRun", (1,)), ("SetRXACBLRun", (0,)), ("SetRXASPCWRun", (0,)), ("SetRXAmpeakRun", (0,))]
    other = [("SetRXAMode", (1,)), ("SetRXAMode", (4,)), ("RXASetPassband", (D(200.0), D(2800.0))),
             ("RXASetPassband", (D(300.0), D(3000.0))), ("SetRXAAGCMode", (2,)), ("SetRXAAGCMode", (3,)), ("SetRXAAGCTop", (D(70.0),))]
    rng = np.random.default_rng(5)
    nblk, walk = 180, 120                 # the seeded walk, then a stretch in which the parameters stand still
    x = synth.make_input_numpy(1, nblk * IN)[0]
    ya, yb = [], []
    pending = {}
    launches0 = lib.qh_wdsp_graph_launches()
    steady = 0                              # fexchange0 calls with no setter on their channel since the call before
    try:
        for k in range(nblk):
            touched = set()
            if k % 6 == 3 and k < walk:
                for _ in range(2):
                    if rng.random() < 0.7:
                        name, args = new[int(rng.integers(0, len(new)))]
                        getattr(lib, name)(A, *[D(v) if isinstance(v, float) else v for v in args])
                        pending.setdefault(k + LAT, []).append((name, args))
                        touched.add(A)
                    else:
                        name, args = other[int(rng.integers(0, len(other)))]
                        getattr(lib, name)(A, *args)
                        getattr(lib, name)(B, *args)
                        touched.update((A, B))
                    assert lib.qh_wdsp_status() == 0, (name, lib.qh_last_error())
            steady += 2 - len(touched)
            blk = x[k * IN:(k + 1) * IN]
            ya.append(_block(lib, A, blk))
            for name, args in pending.pop(k, []):
                getattr(ref, name)(*args)
            yb.append(ref.process(_block(lib, B, blk)))
        ya, yb = np.concatenate(ya), np.concatenate(yb)
        assert np.any(ya != 0)
        assert rel_rms(ya, yb) < 1e-9, rel_rms(ya, yb)
        # OpenChannel switches the launch replay on: what was compared above came out of replayed graphs, not plain launches only
        assert lib.qh_wdsp_graph_launches() - launches0 >= steady // 2, (lib.qh_wdsp_graph_launches() - launches0, steady)
    finally:
        lib.CloseChannel(A)
        lib.CloseChannel(B)


def test_names_invalid_index_reported(qh):
    lib = qh.load()
    ch = 7
    _open(lib, ch, synth.shift_freq(0))
    try:
        lib.SetRXAmpeakNpeaks(ch, 3)
        assert lib.qh_wdsp_status() != 0
        lib.SetRXAmpeakFilFreq(ch, 2, D(800.0))
        assert lib.qh_wdsp_status() != 0
        lib.SetRXAmpeakFilEnable(ch, -1, 1)
        assert lib.qh_wdsp_status() != 0
        lib.SetRXAmpeakNpeaks(ch, 1)
        assert lib.qh_wdsp_status() == 0
    finally:
        lib.CloseChannel(ch)
