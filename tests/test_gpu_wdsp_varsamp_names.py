"""WDSP's variable-ratio resampler through its V names (create_varsampV, xvarsampV, destroy_varsampV, wdsp/varsamp.c:228-250), bound
with ctypes the way a WDSP caller binds them, against the restatement tests/wdsp_varsamp_ref.py: the counts exactly, the samples within
the bound test_gpu_varsamp.py derives; and the device form against the host form, bit for bit.  -m gpu."""
import ctypes as C

import numpy as np
import pytest

from wdsp_varsamp_ref import Varsamp

pytestmark = pytest.mark.gpu
EPS = 2.0 ** -52
CUTS = [0, 1, 2, 100, 1500, 1500, 3000]
VAR = [1.0, 1.01, 0.97, 1.0003, 0.96, 1.04]


def _x(n, seed):
    rng = np.random.default_rng(seed)
    return 0.3 * (rng.standard_normal(n) + 1j * rng.standard_normal(n)) + np.exp(2j * np.pi * 0.043 * np.arange(n))


def _call(lib, ptr, blk, var, in_place, room):
    buf = np.full(max(room, len(blk), 1), np.nan, dtype=np.complex128)
    buf[:len(blk)] = blk
    out = buf if in_place else np.full(max(room, 1), np.nan, dtype=np.complex128)
    got = C.c_int(-1)
    lib.xvarsampV(buf.ctypes.data_as(C.c_void_p), out.ctypes.data_as(C.c_void_p), len(blk), C.c_double(var), C.byref(got), ptr)
    assert lib.qh_wdsp_status() == 0, lib.qh_last_error()
    if not in_place:
        assert np.array_equal(buf[:len(blk)], blk)              # the input is left alone
        assert np.all(np.isnan(out[got.value:].real))           # nothing behind the count
    return out[:got.value].copy()


def _check(what, y, ref_y, B, rsize):
    assert len(y) == len(ref_y), (what, len(y), len(ref_y))
    if not len(y):
        return 0.0
    err, bound = np.abs(y - ref_y), (rsize + 4) * EPS * B
    ratio = float(np.max(err / np.maximum(bound, 1e-300)))
    assert np.all(err <= bound), (what, ratio)
    return ratio


@pytest.mark.parametrize("rates,R", [((48000, 48000), 1024), ((48000, 96000), 64), ((96000, 48000), 64)])
def test_two_pointers_side_by_side_in_place_and_not(qh, oracle, rates, R):
    lib = qh.load()
    xa, xb = _x(3000, 3), _x(3000, 4)
    pa, pb = lib.create_varsampV(rates[0], rates[1], R), lib.create_varsampV(rates[0], rates[1], R)
    assert pa and pb and pa != pb and lib.qh_wdsp_status() == 0, lib.qh_last_error()
    ra, rb = Varsamp(rates[0], rates[1], R), Varsamp(rates[0], rates[1], R)         # run 1, fc 0, fc_low -1, gain 1, var 1, varmode 1
    worst = 0.0
    try:
        for k, (a, b) in enumerate(zip(CUTS[:-1], CUTS[1:])):
            va, vb = VAR[k], VAR[-1 - k]
            room = lib.qh_wdsp_varsampV_max_out(pa, b - a, C.c_double(va))
            assert room >= 0
            ya = _call(lib, pa, xa[a:b], va, True, room)                             # input == output, the two pointers interleaved
            yb = _call(lib, pb, xb[a:b], vb, False, lib.qh_wdsp_varsampV_max_out(pb, b - a, C.c_double(vb)))
            wa, Ba = ra.process(xa[a:b], va)
            wb, Bb = rb.process(xb[a:b], vb)
            worst = max(worst, _check(("a", k), ya, wa, Ba, ra.rsize), _check(("b", k), yb, wb, Bb, rb.rsize))
    finally:
        lib.destroy_varsampV(pa)
        lib.destroy_varsampV(pb)
    assert lib.qh_wdsp_status() == 0
    print("varsamp V names %s R %d: worst |y - ref| / bound %.4f" % (rates, R, worst))


def test_the_device_form_gives_the_bits_of_the_host_form(qh, oracle):
    import torch
    lib = qh.load()
    x = _x(3000, 9)
    ph, pd = lib.create_varsampV(48000, 44100, 256), lib.create_varsampV(48000, 44100, 256)
    assert ph and pd
    s = torch.cuda.Stream()
    try:
        with torch.cuda.stream(s):
            d = torch.from_numpy(x).cuda()
            for k, (a, b) in enumerate(zip(CUTS[:-1], CUTS[1:])):
                var = VAR[k]
                room = max(lib.qh_wdsp_varsampV_max_out(pd, b - a, C.c_double(var)), 1)
                want = _call(lib, ph, x[a:b], var, False, room)
                cnt = torch.full((1,), -1, dtype=torch.int32, device="cuda")
                in_place = k % 2 == 1
                if in_place:                                    # every other call in place, in a buffer with room for the output
                    o = torch.full((max(room, b - a),), float("nan"), dtype=torch.complex128, device="cuda")
                    o[:b - a] = d[a:b]
                    src = o
                else:
                    o = torch.full((room,), float("nan"), dtype=torch.complex128, device="cuda")
                    src = d[a:] if a < len(x) else d
                assert lib.qh_wdsp_xvarsampV_device(pd, src.data_ptr(), o.data_ptr(), b - a, C.c_double(var), cnt.data_ptr(), s.cuda_stream) == 0, lib.qh_last_error()
                c = int(cnt.cpu()[0])                           # (on s, behind the call: nothing else is waited for)
                y = o.cpu().numpy()
                assert c == len(want), (k, c, len(want))
                assert np.array_equal(y[:c], want), k
                if not in_place:
                    assert np.all(np.isnan(y[c:].real))
    finally:
        lib.destroy_varsampV(ph)
        lib.destroy_varsampV(pd)


def test_bad_pointers_and_values_are_reported_and_do_nothing(qh, oracle):
    lib = qh.load()
    buf = np.ones(64, dtype=np.complex128)
    keep = buf.copy()
    got = C.c_int(7)
    bogus = C.c_void_p(buf.ctypes.data)
    lib.xvarsampV(buf.ctypes.data_as(C.c_void_p), buf.ctypes.data_as(C.c_void_p), 64, C.c_double(1.0), C.byref(got), bogus)
    assert lib.qh_wdsp_status() == -2 and got.value == 0 and np.array_equal(buf, keep)
    lib.destroy_varsampV(bogus)
    assert lib.qh_wdsp_status() == -2
    for args in ((0, 48000, 64), (48000, -1, 64), (48000, 48000, 0), (48000, 48000 * 17, 64), (48000, 48000, 1 << 20)):
        assert not lib.create_varsampV(*args), args
        assert lib.qh_wdsp_status() == -2, args
    p = lib.create_varsampV(48000, 48000, 64)
    assert p and lib.qh_wdsp_status() == 0
    ref = Varsamp(48000, 48000, 64)
    try:
        x = _x(600, 2)
        y0 = _call(lib, p, x[:300], 1.01, False, 400)
        for var in (0.0, -1.0, float("nan"), 2.5):
            out = np.full(400, np.nan, dtype=np.complex128)
            lib.xvarsampV(x[300:].ctypes.data_as(C.c_void_p), out.ctypes.data_as(C.c_void_p), 300, C.c_double(var), C.byref(got), p)
            assert lib.qh_wdsp_status() == -2 and got.value == 0 and np.all(np.isnan(out.real)), var
        y1 = _call(lib, p, x[300:], 0.99, False, 400)           # the refused calls left the state alone
        w0, B0 = ref.process(x[:300], 1.01)
        w1, B1 = ref.process(x[300:], 0.99)
        _check("first", y0, w0, B0, 140)
        _check("second", y1, w1, B1, 140)
    finally:
        lib.destroy_varsampV(p)
    lib.destroy_varsampV(p)                                     # twice: the pointer is no longer known
    assert lib.qh_wdsp_status() == -2
