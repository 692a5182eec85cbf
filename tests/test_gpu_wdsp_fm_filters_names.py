"""The five FM filter names of WDSP (SetRXAFMAFFilter, SetRXAFMNCde / MPde / NCaud / MPaud, wdsp/fmd.c:278-384) on two open channels,
bound the way quisk_wdsp.py binds libwdsp: through fexchange0 with host pointers and through qh_wdsp_fexchange0_device with the samples
on the GPU.  The reference is the composition of tests/rxa_fm_filters_ref.py run through the oracle's fexchange0 (the same channel
latency and up-slew, wdsp/iobuffs.c).  Gate 1e-6 relative RMS.  -m gpu.

Where the comparison begins.  A channel that opens feeds its chain 10 ms of zeros and a 25 ms ramp (the up-slew works on the input ring,
iobuffs.c:104-150).  On the zeros nbp0 puts out rounding noise, the FM loop takes its angle, and what the loop does there is no function
of the input (tests/test_gpu_wdsp_fmsq_names.py starts its carrier late for the same reason): the library and the oracle each run their
own loop until the ramp arrives -- with create_rxa's own filters and no hook as well, before this feature as after.  What that leaves
behind is forgotten by the dc removal with 20 ms and by the CTCSS notch with 1 / (3 * 0.0002 * 48000) = 35 ms (iir.c:40: the pole radius
1 - 3 bw): seen through the default filters 1.1 in the first 2048 samples, then a factor 3.4 less per 2048 samples (7e-6 at 20480).
The gate is therefore held from 0.768 s on (36864 samples: 1e-10 of the start by that decay), over 11264 samples; the head's figure is
printed."""
import ctypes as C

import numpy as np
import pytest

from conftest import rel_rms
from rxa_fm_filters_ref import BAND_B, FM, RxaFmRef, fm_tone

pytestmark = pytest.mark.gpu
D = C.c_double
IN, RATE = 64, 48000
CLIP32 = 2147483647.0
NBLK = 752
FROM = 36864


def _open(lib, channel):
    lib.OpenChannel(channel, IN, IN, RATE, RATE, RATE, 0, 1, D(0.010), D(0.025), D(0.0), D(0.010), 1)
    assert lib.qh_wdsp_status() == 0, lib.qh_last_error()
    lib.SetRXAMode(channel, FM)
    lib.RXASetPassband(channel, D(-8000.0), D(8000.0))
    lib.SetRXAAGCMode(channel, 0); lib.SetRXAAGCFixed(channel, D(0.0))
    assert lib.qh_wdsp_status() == 0, lib.qh_last_error()


def _ref():
    r = RxaFmRef(IN, IN, RATE, RATE, RATE)
    r.SetRXAMode(FM); r.RXASetPassband(-8000.0, 8000.0); r.SetRXAAGCMode(0); r.SetRXAAGCFixed(0.0)
    return r


def _settings(lib, refs, a, b):
    """channel a: band B, a short minimum-phase audio filter; channel b: a short de-emphasis filter; then the refusals"""
    lib.SetRXAFMAFFilter(a, D(BAND_B[0]), D(BAND_B[1])); refs[0].SetRXAFMAFFilter(*BAND_B)
    lib.SetRXAFMNCaud(a, 512); refs[0].SetRXAFMNCaud(512)
    lib.SetRXAFMMPaud(a, 1); refs[0].SetRXAFMMPaud(1)
    lib.SetRXAFMNCde(b, 1024); refs[1].SetRXAFMNCde(1024)
    lib.SetRXAFMMPde(b, 0); refs[1].SetRXAFMMPde(0)
    assert lib.qh_wdsp_status() == 0, lib.qh_last_error()
    lib.SetRXAFMAFFilter(b, D(0.0), D(3000.0))
    assert lib.qh_wdsp_status() == -2
    lib.SetRXAFMNCde(b, 1000)
    assert lib.qh_wdsp_status() == -2


def _x():
    return [fm_tone(NBLK * IN, RATE, carrier=500.0 * (c + 1), tone=800.0 + 300.0 * c, seed=70 + c, sigma=0.002) for c in range(2)]


def _held(y, r, what):
    for c in range(2):
        err = rel_rms(y[c][FROM:], r[c][FROM:])
        print("%s: channel %d against the composition through the oracle's fexchange0, relative RMS %.3g from sample %d on (%.3g over the %d ahead)"
              % (what, c, err, FROM, rel_rms(y[c][:FROM], r[c][:FROM]), FROM))
        assert y[c].size == r[c].size == NBLK * IN
        assert np.max(np.abs(r[c][FROM:])) > 1e-4
        assert err < 1e-6, (what, c, err)


def test_host_pointers(qh):
    lib = qh.load()
    a, b = 2, 3
    x, refs = _x(), [_ref(), _ref()]
    for ch in (a, b):
        _open(lib, ch)
    try:
        _settings(lib, refs, a, b)
        y = [np.zeros(NBLK * IN, dtype=np.complex128) for _ in range(2)]
        err = C.c_int(0)
        out = np.zeros(IN, dtype=np.complex128)
        for k in range(NBLK):
            for i, ch in enumerate((a, b)):
                blk = np.ascontiguousarray(x[i][k * IN:(k + 1) * IN])
                lib.fexchange0(ch, blk.ctypes.data_as(C.c_void_p), out.ctypes.data_as(C.c_void_p), C.byref(err))
                assert err.value == 0 and lib.qh_wdsp_status() == 0, lib.qh_last_error()
                y[i][k * IN:(k + 1) * IN] = out
    finally:
        for ch in (a, b):
            lib.CloseChannel(ch)
    r = [refs[i].o.fexchange0(x[i])[0] for i in range(2)]
    for ref in refs:
        ref.close()
    _held(y, r, "fexchange0")


def test_samples_on_the_device(qh):
    import torch
    lib = qh.load()
    dev = torch.device("cuda", 0)
    stream = torch.cuda.Stream(dev)
    a, b = 4, 5
    x, refs = _x(), [_ref(), _ref()]
    seg = 16 * IN
    for ch in (a, b):
        _open(lib, ch)
        lib.qh_wdsp_set_parameter(ch, IN, 1)
    try:
        _settings(lib, refs, a, b)
        y = [[], []]
        for pos in range(0, NBLK * IN, seg):
            for i, ch in enumerate((a, b)):
                with torch.cuda.stream(stream):
                    work = torch.zeros(seg + 2 * IN, dtype=torch.complex128, device=dev)
                    work[:seg] = torch.from_numpy(x[i][pos:pos + seg] * CLIP32).to(dev)
                    n = lib.qh_wdsp_fexchange0_device(ch, C.c_void_p(work.data_ptr()), seg, C.c_void_p(stream.cuda_stream))
                    assert lib.qh_wdsp_status() == 0, lib.qh_last_error()
                    got = work[:n].cpu()
                stream.synchronize()
                y[i].append(got.numpy() / CLIP32)
    finally:
        for ch in (a, b):
            lib.qh_wdsp_set_parameter(ch, 0, 0)
            lib.wdspFexchange0(ch, None, 0)
            lib.CloseChannel(ch)
    y = [np.concatenate(v) for v in y]
    assert y[0].size == NBLK * IN
    r = [refs[i].o.fexchange0(x[i])[0] for i in range(2)]
    for ref in refs:
        ref.close()
    _held(y, r, "qh_wdsp_fexchange0_device")
