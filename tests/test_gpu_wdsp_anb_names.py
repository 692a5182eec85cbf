"""WDSP's blanker through its EXT names (create_anbEXT, xanbEXT, SetEXTANB*, wdsp/nob.c:307-422), bound with ctypes the way a WDSP
caller binds them, against the restatement tests/wdsp_anb_ref.py: bit-exact like test_gpu_anb.py, under the same condition on the input
(a trigger margin of at least 1e-9 on the restatement).  -m gpu."""
import ctypes as C

import numpy as np
import pytest

from conftest import rel_rms
from quisk_amd import synth
from test_gpu_wdsp_dropin import _open, _oracle
from wdsp_anb_ref import Anb

pytestmark = pytest.mark.gpu
D = C.c_double
MARGIN = 1e-9
TYP = dict(tau=1e-4, hangtime=1e-4, advtime=1e-4, backtau=0.05, threshold=30.0)
OTHER = dict(tau=3e-4, hangtime=0.0, advtime=2e-4, backtau=0.02, threshold=12.0)


def _create(lib, id_, run, size, rate, p):
    lib.create_anbEXT(id_, run, size, D(rate), D(p["tau"]), D(p["hangtime"]), D(p["advtime"]), D(p["backtau"]), D(p["threshold"]))
    assert lib.qh_wdsp_status() == 0, lib.qh_last_error()


def _x(n, seed):
    x = synth.impulsive_input(1, n, seed=seed, scale=0.8)[0]
    for edge in (4096, 8192 + 64, 20480):
        x[edge - 1:edge + 1] += 50.0
    return x


def _call(lib, id_, blk, in_place):
    buf = np.ascontiguousarray(blk).copy()
    out = buf if in_place else np.full_like(buf, np.nan)
    lib.xanbEXT(id_, buf.ctypes.data_as(C.c_void_p), out.ctypes.data_as(C.c_void_p))
    assert lib.qh_wdsp_status() == 0, lib.qh_last_error()
    if not in_place:
        assert np.array_equal(buf, blk)                     # the input is left alone
    return out


def test_two_ids_side_by_side_in_place_and_not(qh):
    lib = qh.load()
    rate, size, nblk = 192000, 1024, 40
    xa, xb = _x(size * nblk, 3), _x(size * nblk, 4)
    _create(lib, 4, 1, size, rate, TYP)
    _create(lib, 9, 1, size, rate, OTHER)
    ra, rb = Anb(rate, **TYP), Anb(rate, **OTHER)
    try:
        ya = np.concatenate([_call(lib, 4, xa[k * size:(k + 1) * size], True) for k in range(nblk)])     # in == out, the callers' way
        yb = []
        for k in range(nblk):                               # the two ids interleaved, this one with buffers apart
            yb.append(_call(lib, 9, xb[k * size:(k + 1) * size], False))
        yb = np.concatenate(yb)
    finally:
        lib.destroy_anbEXT(4)
        lib.destroy_anbEXT(9)
    wa, wb = ra.process(xa), rb.process(xb)
    print("anb names: margins %.3e %.3e, triggers %d %d" % (ra.margin, rb.margin, ra.triggers, rb.triggers))
    assert ra.margin >= MARGIN and rb.margin >= MARGIN
    assert np.count_nonzero(wa == 0) > 200 and np.count_nonzero(wb == 0) > 200
    assert np.array_equal(ya, wa) and np.array_equal(yb, wb)


def test_setters_buffsize_flush_and_run(qh):
    lib = qh.load()
    rate = 192000
    x = _x(40000, 8)
    ref = Anb(rate, run=0, **TYP)
    _create(lib, 0, 0, 500, rate, TYP)
    ys, rs = [], []
    pos = 0

    def go(size, count):
        nonlocal pos
        for _ in range(count):
            ys.append(_call(lib, 0, x[pos:pos + size], True)); rs.append(ref.process(x[pos:pos + size]))
            pos += size
    try:
        go(500, 3)                                          # created with run = 0: copies
        assert np.array_equal(np.concatenate(ys), x[:1500])
        lib.SetEXTANBRun(0, 1); ref.SetRun(1)
        go(500, 10)
        lib.SetEXTANBBuffsize(0, 2048)
        go(2048, 4)
        lib.SetEXTANBThreshold(0, D(9.0)); ref.SetThreshold(9.0)
        go(2048, 2)
        lib.SetEXTANBTau(0, D(2e-4)); ref.SetTau(2e-4)
        lib.SetEXTANBBuffsize(0, 1)
        go(1, 5)
        lib.SetEXTANBBuffsize(0, 1500)
        lib.SetEXTANBHangtime(0, D(0.0)); ref.SetHangtime(0.0)
        go(1500, 2)
        lib.SetEXTANBAdvtime(0, D(3e-4)); ref.SetAdvtime(3e-4)
        go(1500, 2)
        lib.SetEXTANBBacktau(0, D(0.01)); ref.SetBacktau(0.01)
        go(1500, 2)
        lib.flush_anbEXT(0); ref.flush()
        go(1500, 2)
        lib.SetEXTANBSamplerate(0, 96000); ref.SetSamplerate(96000)
        go(1500, 3)
        assert lib.qh_wdsp_status() == 0, lib.qh_last_error()
        # refused values are reported and change nothing
        lib.SetEXTANBTau(0, D(0.003))
        assert lib.qh_wdsp_status() == -2
        lib.SetEXTANBSamplerate(0, 0)
        assert lib.qh_wdsp_status() == -2
        lib.SetEXTANBBuffsize(0, 0)
        assert lib.qh_wdsp_status() == -2
        go(1500, 2)
    finally:
        lib.destroy_anbEXT(0)
    y, r = np.concatenate(ys), np.concatenate(rs)
    print("anb names setters: margin %.3e, %d triggers" % (ref.margin, ref.triggers))
    assert ref.margin >= MARGIN and np.count_nonzero(r == 0) > 200
    assert np.array_equal(y, r)


def test_device_pointers(qh):
    import torch
    lib = qh.load()
    rate, size, nblk = 192000, 4096, 8
    x = _x(size * nblk, 21)
    ref = Anb(rate, **TYP)
    _create(lib, 31, 1, size, rate, TYP)
    s = torch.cuda.Stream()
    try:
        with torch.cuda.stream(s):
            d = torch.from_numpy(x).cuda()
            o = torch.zeros_like(d)
            for k in range(nblk):
                src = d[k * size:(k + 1) * size]
                dst = src if k % 2 else o[k * size:(k + 1) * size]       # every other block in place
                assert lib.qh_wdsp_xanbEXT_device(31, src.data_ptr(), dst.data_ptr(), s.cuda_stream) == 0, lib.qh_last_error()
                if k % 2:
                    o[k * size:(k + 1) * size] = src
            y = o.cpu().numpy()
    finally:
        lib.destroy_anbEXT(31)
    want = ref.process(x)
    assert ref.margin >= MARGIN and np.count_nonzero(want == 0) > 100
    assert np.array_equal(y, want)


def test_bad_ids_are_reported_and_do_nothing(qh):
    lib = qh.load()
    buf = np.ones(64, dtype=np.complex128)
    keep = buf.copy()
    for id_ in (-1, 32, 17):                                 # out of range twice, then an id nobody created
        lib.xanbEXT(id_, buf.ctypes.data_as(C.c_void_p), buf.ctypes.data_as(C.c_void_p))
        assert lib.qh_wdsp_status() == -2, id_
        assert b"ANB id" in lib.qh_last_error()
        for name, arg in (("SetEXTANBRun", 1), ("SetEXTANBBuffsize", 64), ("SetEXTANBSamplerate", 48000), ("SetEXTANBTau", D(1e-4)),
                          ("SetEXTANBHangtime", D(1e-4)), ("SetEXTANBAdvtime", D(1e-4)), ("SetEXTANBBacktau", D(0.05)), ("SetEXTANBThreshold", D(30.0))):
            getattr(lib, name)(id_, arg)
            assert lib.qh_wdsp_status() == -2, (name, id_)
        lib.flush_anbEXT(id_)
        assert lib.qh_wdsp_status() == -2
        lib.destroy_anbEXT(id_)
        assert lib.qh_wdsp_status() == -2
    assert np.array_equal(buf, keep)
    lib.create_anbEXT(32, 1, 64, D(48000.0), D(1e-4), D(1e-4), D(1e-4), D(0.05), D(30.0))
    assert lib.qh_wdsp_status() == -2
    lib.create_anbEXT(5, 1, 64, D(48000.0), D(0.01), D(1e-4), D(1e-4), D(0.05), D(30.0))       # tau beyond the delay line
    assert lib.qh_wdsp_status() == -2
    lib.xanbEXT(5, buf.ctypes.data_as(C.c_void_p), buf.ctypes.data_as(C.c_void_p))             # ... so id 5 was not created
    assert lib.qh_wdsp_status() == -2 and np.array_equal(buf, keep)
    _create(lib, 5, 1, 64, 48000, TYP)
    lib.create_anbEXT(5, 1, 64, D(48000.0), D(1e-4), D(1e-4), D(1e-4), D(0.05), D(30.0))       # twice
    assert lib.qh_wdsp_status() == -2
    lib.destroy_anbEXT(5)
    assert lib.qh_wdsp_status() == 0


def test_blanker_in_front_of_fexchange0(qh, oracle):
    """xanbEXT, in place, on every block on its way into fexchange0 -- what the reference's callers do -- gives what the restatement
    followed by the oracle's channel gives, at the channel's tolerance (test_gpu_wdsp_dropin.py: 1e-9)."""
    lib = qh.load()
    in_size, rate, ch, id_ = 1024, 192000, 3, 2
    n = in_size * 48
    x = synth.make_input_numpy(1, n, fs=float(rate))[0] * 8.0          # mean magnitude near the average's start value
    rng = np.random.default_rng(12)
    for p in rng.integers(2000, n - 10, size=30):
        x[p:p + 2] += 40.0 * (1.0 + rng.random())
    prm = dict(TYP, threshold=20.0)
    ref = Anb(rate, **prm)
    blanked = ref.process(x)
    print("anb + fexchange0: margin %.3e, %d triggers" % (ref.margin, ref.triggers))
    assert ref.margin >= MARGIN and ref.triggers >= 30 and np.count_nonzero(blanked == 0) > 30 * 20         # every planted pulse: at least adv_count + 1 = 20 zeros
    _open(lib, ch, in_size, 256, rate, nbp=True, shift_freq=10000.0)
    _create(lib, id_, 1, in_size, rate, prm)
    out = np.zeros(n // 4, dtype=np.complex128)
    err = C.c_int(0)
    try:
        for b in range(n // in_size):
            blk = np.ascontiguousarray(x[b * in_size:(b + 1) * in_size]).copy()
            lib.xanbEXT(id_, blk.ctypes.data_as(C.c_void_p), blk.ctypes.data_as(C.c_void_p))
            assert lib.qh_wdsp_status() == 0, lib.qh_last_error()
            lib.fexchange0(ch, blk.ctypes.data_as(C.c_void_p), out[b * 256:].ctypes.data_as(C.c_void_p), C.byref(err))
            assert err.value == 0
    finally:
        lib.destroy_anbEXT(id_)
        lib.CloseChannel(ch)
    want, errs = _oracle(oracle, in_size, 256, rate, True, 10000.0).fexchange0(blanked)
    plain, _ = _oracle(oracle, in_size, 256, rate, True, 10000.0).fexchange0(x)
    assert errs == 0
    assert rel_rms(out, want) < 1e-9, rel_rms(out, want)
    assert rel_rms(plain, want) > 1e-3                                   # the blanker made a difference to compare
