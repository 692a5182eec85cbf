"""WDSP's second blanker through its EXT names (create_nobEXT, xnobEXT, SetEXTNOB*, wdsp/nobII.c:605-734), bound with ctypes the way a
WDSP caller binds them, against the restatement tests/wdsp_nob_ref.py: bit-exact like test_gpu_nob.py, under the same condition on the
input (a trigger margin of at least 1e-9 on the restatement).  -m gpu."""
import ctypes as C

import numpy as np
import pytest

from quisk_amd import synth
from wdsp_nob_ref import Nob

pytestmark = pytest.mark.gpu
D = C.c_double
MARGIN = 1e-9
TYP = dict(slewtime=1e-4, hangtime=1e-4, advtime=1e-4, backtau=0.05, threshold=30.0)
OTHER = dict(slewtime=3e-4, hangtime=0.0, advtime=2e-4, backtau=0.02, threshold=12.0)


def _create(lib, id_, run, mode, size, rate, p):
    lib.create_nobEXT(id_, run, mode, size, D(rate), D(p["slewtime"]), D(p["hangtime"]), D(p["advtime"]), D(p["backtau"]), D(p["threshold"]))
    assert lib.qh_wdsp_status() == 0, lib.qh_last_error()


def _x(n, seed):
    x = synth.impulsive_input(1, n, seed=seed, scale=0.8)[0]
    for edge in (4096, 8192 + 64, 20480):
        x[edge - 1:edge + 1] += 50.0
    return x


def _call(lib, id_, blk, in_place):
    buf = np.ascontiguousarray(blk).copy()
    out = buf if in_place else np.full_like(buf, np.nan)
    lib.xnobEXT(id_, buf.ctypes.data_as(C.c_void_p), out.ctypes.data_as(C.c_void_p))
    assert lib.qh_wdsp_status() == 0, lib.qh_last_error()
    if not in_place:
        assert np.array_equal(buf, blk)                     # the input is left alone
    return out


def test_three_ids_side_by_side_in_place_and_not(qh):
    lib = qh.load()
    rate, size, nblk = 192000, 1024, 40
    xs = [_x(size * nblk, s) for s in (3, 4, 6)]
    ids, modes, prms = (4, 9, 30), (4, 2, 1), (TYP, OTHER, TYP)
    refs = [Nob(rate, m, **p) for m, p in zip(modes, prms)]
    for id_, m, p in zip(ids, modes, prms):
        _create(lib, id_, 1, m, size, rate, p)
    ys = [[], [], []]
    try:
        for k in range(nblk):                               # the ids interleaved; the first in == out, the callers' way
            for j, id_ in enumerate(ids):
                ys[j].append(_call(lib, id_, xs[j][k * size:(k + 1) * size], j == 0))
    finally:
        for id_ in ids:
            lib.destroy_nobEXT(id_)
    for j, r in enumerate(refs):
        want = r.process(xs[j])
        print("nob names id %d: margin %.3e, %d triggers, %d blanks" % (ids[j], r.margin, r.triggers, r.blanks))
        assert r.margin >= MARGIN and r.blanks > 5
        assert np.array_equal(np.concatenate(ys[j]), want), j


def test_setters_buffsize_flush_and_run(qh):
    lib = qh.load()
    rate = 192000
    x = _x(120000, 8)
    ref = Nob(rate, 1, run=0, **TYP)
    _create(lib, 0, 0, 1, 500, rate, TYP)
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
        lib.SetEXTNOBRun(0, 1); ref.SetRun(1)
        go(500, 20)
        lib.SetEXTNOBBuffsize(0, 2048)                      # n changes, nothing is flushed
        go(2048, 5)
        lib.SetEXTNOBThreshold(0, D(9.0)); ref.SetThreshold(9.0)
        go(2048, 3)
        lib.SetEXTNOBMode(0, 4); ref.SetMode(4)
        go(2048, 4)
        lib.SetEXTNOBTau(0, D(2e-4)); ref.SetTau(2e-4)
        lib.SetEXTNOBBuffsize(0, 1)
        go(1, 5)
        lib.SetEXTNOBBuffsize(0, 3000)
        lib.SetEXTNOBHangtime(0, D(0.0)); ref.SetHangtime(0.0)
        go(3000, 3)
        lib.SetEXTNOBAdvtime(0, D(3e-4)); ref.SetAdvtime(3e-4)
        go(3000, 3)
        lib.SetEXTNOBBacktau(0, D(0.01)); ref.SetBacktau(0.01)
        go(3000, 3)
        lib.flush_nobEXT(0); ref.flush()
        go(3000, 3)
        lib.SetEXTNOBSamplerate(0, 96000); ref.SetSamplerate(96000)
        go(3000, 4)
        assert lib.qh_wdsp_status() == 0, lib.qh_last_error()
        # refused values are reported and change nothing
        for name, arg in (("SetEXTNOBTau", D(0.003)), ("SetEXTNOBSamplerate", 0), ("SetEXTNOBBuffsize", 0), ("SetEXTNOBMode", 5),
                          ("SetEXTNOBHangtime", D(0.0021)), ("SetEXTNOBAdvtime", D(-1e-6)), ("SetEXTNOBBacktau", D(0.0)),
                          ("SetEXTNOBThreshold", D(float("nan")))):
            getattr(lib, name)(0, arg)
            assert lib.qh_wdsp_status() == -2, name
        go(3000, 3)
    finally:
        lib.destroy_nobEXT(0)
    y, r = np.concatenate(ys), np.concatenate(rs)
    print("nob names setters: margin %.3e, %d triggers, %d blanks" % (ref.margin, ref.triggers, ref.blanks))
    assert ref.margin >= MARGIN and ref.blanks > 20
    assert np.array_equal(y, r)


def test_device_pointers_and_switching_between_the_two_entries(qh):
    import torch
    lib = qh.load()
    rate, size, nblk = 192000, 4096, 12
    x = _x(size * nblk, 21)
    ref = Nob(rate, 4, **TYP)
    _create(lib, 31, 1, 4, size, rate, TYP)
    s = torch.cuda.Stream()
    try:
        with torch.cuda.stream(s):
            d = torch.from_numpy(x).cuda()
            o = torch.zeros_like(d)
            host = {}
            for k in range(nblk):
                src = d[k * size:(k + 1) * size]
                if k % 3 == 2:                                           # every third block through xnobEXT, from the host
                    s.synchronize()
                    host[k] = _call(lib, 31, x[k * size:(k + 1) * size], False)
                    continue
                dst = src if k % 2 else o[k * size:(k + 1) * size]       # every other one in place
                assert lib.qh_wdsp_xnobEXT_device(31, src.data_ptr(), dst.data_ptr(), s.cuda_stream) == 0, lib.qh_last_error()
                if k % 2:
                    o[k * size:(k + 1) * size] = src
            y = o.cpu().numpy()
        for k, v in host.items():
            y[k * size:(k + 1) * size] = v
    finally:
        lib.destroy_nobEXT(31)
    want = ref.process(x)
    print("nob names device: margin %.3e, %d blanks" % (ref.margin, ref.blanks))
    assert ref.margin >= MARGIN and ref.blanks > 5
    assert np.array_equal(y, want)
    # ... and the host entry alone gives the same samples
    _create(lib, 31, 1, 4, size, rate, TYP)
    try:
        again = np.concatenate([_call(lib, 31, x[k * size:(k + 1) * size], True) for k in range(nblk)])
    finally:
        lib.destroy_nobEXT(31)
    assert np.array_equal(again, want)


def test_bad_ids_are_reported_and_do_nothing(qh):
    lib = qh.load()
    buf = np.ones(64, dtype=np.complex128)
    keep = buf.copy()
    for id_ in (-1, 32, 17):                                 # out of range twice, then an id nobody created
        lib.xnobEXT(id_, buf.ctypes.data_as(C.c_void_p), buf.ctypes.data_as(C.c_void_p))
        assert lib.qh_wdsp_status() == -2, id_
        assert b"NOB id" in lib.qh_last_error()
        for name, arg in (("SetEXTNOBRun", 1), ("SetEXTNOBMode", 1), ("SetEXTNOBBuffsize", 64), ("SetEXTNOBSamplerate", 48000),
                          ("SetEXTNOBTau", D(1e-4)), ("SetEXTNOBHangtime", D(1e-4)), ("SetEXTNOBAdvtime", D(1e-4)), ("SetEXTNOBBacktau", D(0.05)),
                          ("SetEXTNOBThreshold", D(30.0))):
            getattr(lib, name)(id_, arg)
            assert lib.qh_wdsp_status() == -2, (name, id_)
        lib.flush_nobEXT(id_)
        assert lib.qh_wdsp_status() == -2
        lib.destroy_nobEXT(id_)
        assert lib.qh_wdsp_status() == -2
        assert lib.qh_wdsp_xnobEXT_device(id_, None, None, None) == -2
    assert np.array_equal(buf, keep)
    lib.create_nobEXT(32, 1, 0, 64, D(48000.0), D(1e-4), D(1e-4), D(1e-4), D(0.05), D(30.0))
    assert lib.qh_wdsp_status() == -2
    lib.create_nobEXT(5, 1, 0, 64, D(48000.0), D(0.01), D(1e-4), D(1e-4), D(0.05), D(30.0))     # a slew time beyond awave[]
    assert lib.qh_wdsp_status() == -2
    lib.create_nobEXT(5, 1, 7, 64, D(48000.0), D(1e-4), D(1e-4), D(1e-4), D(0.05), D(30.0))      # no such mode
    assert lib.qh_wdsp_status() == -2
    lib.xnobEXT(5, buf.ctypes.data_as(C.c_void_p), buf.ctypes.data_as(C.c_void_p))               # ... so id 5 was not created
    assert lib.qh_wdsp_status() == -2 and np.array_equal(buf, keep)
    _create(lib, 5, 1, 0, 64, 48000, TYP)
    lib.create_nobEXT(5, 1, 0, 64, D(48000.0), D(1e-4), D(1e-4), D(1e-4), D(0.05), D(30.0))      # twice
    assert lib.qh_wdsp_status() == -2
    lib.destroy_nobEXT(5)
    assert lib.qh_wdsp_status() == 0
