"""WDSP's fixed-ratio resampler through its V and FV names (create_resampleV, xresampleV, destroy_resampleV and the FV three,
wdsp/resample.c:206-228, 332-354), bound with ctypes the way a WDSP caller binds them, against a one-channel qh_resample bank, bit for
bit; input == output where the reference allows it and refused where it does not; the device forms against the host forms.  -m gpu."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
CUTS = [0, 1, 2, 100, 1500, 1500, 3000]
KINDS = {"V": (np.complex128, "c64"), "FV": (np.float32, "r32")}


def _x(n, seed, kind):
    rng = np.random.default_rng(seed)
    x = 0.3 * (rng.standard_normal(n) + 1j * rng.standard_normal(n)) + np.exp(2j * np.pi * 0.043 * np.arange(n))
    return x if kind == "V" else x.real.astype(np.float32)


def _call(lib, kind, ptr, blk, in_place, room):
    buf = np.full(max(room, len(blk), 1), np.nan, dtype=blk.dtype)
    buf[:len(blk)] = blk
    out = buf if in_place else np.full(max(room, 1), np.nan, dtype=blk.dtype)
    got = C.c_int(-1)
    getattr(lib, "xresample" + kind)(buf.ctypes.data_as(C.c_void_p), out.ctypes.data_as(C.c_void_p), len(blk), C.byref(got), ptr)
    assert lib.qh_wdsp_status() == 0, lib.qh_last_error()
    if not in_place:
        assert np.array_equal(buf[:len(blk)], blk)              # the input is left alone
        assert np.all(np.isnan(out[got.value:].real))           # nothing behind the count
    return out[:got.value].copy()


@pytest.mark.parametrize("kind", ["V", "FV"])
@pytest.mark.parametrize("rates", [(48000, 44100), (44100, 48000), (96000, 48000)])
def test_the_names_give_the_banks_bits(qh, oracle, kind, rates):
    lib = qh.load()
    x = _x(3000, 3, kind)
    bank = qh.WdspResampler(1, *rates, dtype=KINDS[kind][1])    # run 1, fc 0, ncoef 0, gain 1: what create_resampleV fixes
    p = getattr(lib, "create_resample" + kind)(*rates)
    assert p and lib.qh_wdsp_status() == 0, lib.qh_last_error()
    total = 0
    try:
        for a, b in zip(CUTS[:-1], CUTS[1:]):
            room = lib.qh_wdsp_resampleV_max_out(p, b - a)
            assert room == bank.max_out(b - a)
            y = _call(lib, kind, p, x[a:b], False, room)
            wy, wc = bank.process_host(x[None, a:b])
            assert len(y) == wc[0] and np.array_equal(y, wy[0, :wc[0]]), (a, b)
            total += len(y)
    finally:
        getattr(lib, "destroy_resample" + kind)(p)
    assert lib.qh_wdsp_status() == 0 and total == -(-3000 * bank.L() // bank.M())


@pytest.mark.parametrize("kind", ["V", "FV"])
def test_in_place_where_the_reference_allows_it(qh, oracle, kind):
    lib = qh.load()
    x = _x(3000, 4, kind)
    create, destroy = getattr(lib, "create_resample" + kind), getattr(lib, "destroy_resample" + kind)
    pa, pb = create(96000, 48000), create(96000, 48000)         # L 1 <= M 2: the reference never reads a sample it has overwritten
    assert pa and pb and pa != pb
    try:
        for a, b in zip(CUTS[:-1], CUTS[1:]):
            room = lib.qh_wdsp_resampleV_max_out(pa, b - a)
            ya, yb = _call(lib, kind, pa, x[a:b], True, room), _call(lib, kind, pb, x[a:b], False, room)
            assert np.array_equal(ya, yb), (a, b)
    finally:
        destroy(pa)
        destroy(pb)
    p = create(48000, 96000)                                    # L 2 > M 1: xresample would overwrite in[1] with out[1] before reading it
    assert p
    try:
        buf = np.zeros(2 * 400, dtype=x.dtype)
        buf[:400] = x[:400]
        keep = buf.copy()
        got = C.c_int(7)
        getattr(lib, "xresample" + kind)(buf.ctypes.data_as(C.c_void_p), buf.ctypes.data_as(C.c_void_p), 400, C.byref(got), p)
        assert lib.qh_wdsp_status() == -2 and got.value == 0 and np.array_equal(buf, keep)
        # the refused call moved nothing: out of place, the stream starts where a fresh one does
        y = _call(lib, kind, p, x[:400], False, 800)
        q = create(48000, 96000)
        try:
            assert np.array_equal(y, _call(lib, kind, q, x[:400], False, 800)) and len(y) == 800
        finally:
            destroy(q)
    finally:
        destroy(p)


@pytest.mark.parametrize("kind", ["V", "FV"])
def test_the_device_forms_give_the_bits_of_the_host_forms(qh, oracle, kind):
    import torch
    lib = qh.load()
    x = _x(3000, 9, kind)
    tdt = torch.complex128 if kind == "V" else torch.float32
    es = x.dtype.itemsize
    create, destroy = getattr(lib, "create_resample" + kind), getattr(lib, "destroy_resample" + kind)
    xdev = getattr(lib, "qh_wdsp_xresample%s_device" % kind)
    ph, pd = create(96000, 44100), create(96000, 44100)         # L 147 <= M 320: every other call in place
    assert ph and pd
    s = torch.cuda.Stream()
    try:
        with torch.cuda.stream(s):
            d = torch.from_numpy(x).cuda()
            for k, (a, b) in enumerate(zip(CUTS[:-1], CUTS[1:])):
                room = max(lib.qh_wdsp_resampleV_max_out(pd, b - a), 1)
                want = _call(lib, kind, ph, x[a:b], False, room)
                cnt = C.c_int(-1)
                in_place = k % 2 == 1
                if in_place:
                    o = torch.full((max(room, b - a),), float("nan"), dtype=tdt, device="cuda")
                    o[:b - a] = d[a:b]
                    src = o.data_ptr()
                else:
                    o = torch.full((room,), float("nan"), dtype=tdt, device="cuda")
                    src = d.data_ptr() + es * min(a, len(x) - 1)
                assert xdev(pd, src, o.data_ptr(), b - a, C.byref(cnt), s.cuda_stream) == 0, lib.qh_last_error()
                y = o.cpu().numpy()                             # (on s, behind the call: nothing else is waited for)
                assert cnt.value == len(want), (k, cnt.value, len(want))
                assert np.array_equal(y[:cnt.value], want), k
                if not in_place:
                    assert np.all(np.isnan(y[cnt.value:].real))
        # where L > M the device form refuses d_in == d_out as the host form does
        q = create(48000, 96000)
        try:
            o = torch.zeros(64, dtype=tdt, device="cuda")
            cnt = C.c_int(5)
            assert xdev(q, o.data_ptr(), o.data_ptr(), 16, C.byref(cnt), None) == -2 and cnt.value == 0 and lib.qh_wdsp_status() == -2
        finally:
            destroy(q)
    finally:
        destroy(ph)
        destroy(pd)


def test_bad_pointers_and_values_are_reported_and_do_nothing(qh, oracle):
    lib = qh.load()
    buf = np.ones(64, dtype=np.complex128)
    keep = buf.copy()
    out = np.full(64, np.nan, dtype=np.complex128)
    got = C.c_int(7)
    bogus = C.c_void_p(buf.ctypes.data)
    lib.xresampleV(buf.ctypes.data_as(C.c_void_p), out.ctypes.data_as(C.c_void_p), 64, C.byref(got), bogus)
    assert lib.qh_wdsp_status() == -2 and got.value == 0 and np.array_equal(buf, keep) and np.all(np.isnan(out.real))
    lib.destroy_resampleV(bogus)
    assert lib.qh_wdsp_status() == -2
    assert lib.qh_wdsp_resampleV_max_out(bogus, 10) == -2
    for args in ((0, 48000), (48000, -1), (48000, 44101), (2000000000, 44100)):
        for kind in ("V", "FV"):
            assert not getattr(lib, "create_resample" + kind)(*args), (kind, args)
            assert lib.qh_wdsp_status() == -2, (kind, args)
    p, f = lib.create_resampleV(48000, 44100), lib.create_resampleFV(48000, 44100)
    assert p and f and lib.qh_wdsp_status() == 0
    try:
        # a V pointer is not an FV pointer
        got = C.c_int(7)
        lib.xresampleFV(buf.ctypes.data_as(C.c_void_p), out.ctypes.data_as(C.c_void_p), 64, C.byref(got), p)
        assert lib.qh_wdsp_status() == -2 and got.value == 0 and np.all(np.isnan(out.real))
        lib.destroy_resampleFV(p)
        assert lib.qh_wdsp_status() == -2
        lib.xresampleV(buf.ctypes.data_as(C.c_void_p), out.ctypes.data_as(C.c_void_p), -1, C.byref(got), p)
        assert lib.qh_wdsp_status() == -2 and got.value == 0
        lib.xresampleV(buf.ctypes.data_as(C.c_void_p), out.ctypes.data_as(C.c_void_p), 64, C.byref(got), p)
        assert lib.qh_wdsp_status() == 0 and got.value == 59    # ceil(64 * 147 / 160)
    finally:
        lib.destroy_resampleV(p)
        lib.destroy_resampleFV(f)
    assert lib.qh_wdsp_status() == 0
    lib.destroy_resampleV(p)                                    # twice: the pointer is no longer known
    assert lib.qh_wdsp_status() == -2
    got = C.c_int(7)
    lib.xresampleV(buf.ctypes.data_as(C.c_void_p), out.ctypes.data_as(C.c_void_p), 64, C.byref(got), p)   # destroy, then use
    assert lib.qh_wdsp_status() == -2 and got.value == 0


def test_pointers_of_three_kinds_alive_at_once(qh, oracle):
    """A create_resampleV, a create_resampleFV and a create_varsampV pointer side by side: every x and destroy name handed a pointer
    of another family or kind reports QH_ERR_INVALID, leaves the count 0 and the output as it was (test_bad_pointers_and_values_...
    above holds only the V pointer under the FV names); and destroying one leaves the other two giving the bits of twins that never
    had such a neighbour, one 64-sample call each."""
    lib = qh.load()
    vp = lambda a: a.ctypes.data_as(C.c_void_p)
    xc, xf = _x(128, 7, "V"), _x(128, 7, "FV")

    def rs(kind, p, blk):
        return _call(lib, kind, p, blk, False, 96)

    def vs(p, blk):
        out, got = np.full(96, np.nan, dtype=np.complex128), C.c_int(-1)
        lib.xvarsampV(vp(blk), vp(out), len(blk), C.c_double(1.01), C.byref(got), p)
        assert lib.qh_wdsp_status() == 0, lib.qh_last_error()
        return out[:got.value].copy()

    made = [lib.create_resampleV(48000, 44100), lib.create_resampleFV(48000, 44100), lib.create_varsampV(48000, 48000, 64)]
    twins = [lib.create_resampleV(48000, 44100), lib.create_resampleFV(48000, 44100), lib.create_varsampV(48000, 48000, 64)]
    assert all(made) and all(twins) and len(set(made + twins)) == 6
    v, f, s = made
    try:
        calls = {"xresampleV": lambda p, o, g: lib.xresampleV(vp(xc), vp(o), 64, C.byref(g), p),
                 "xresampleFV": lambda p, o, g: lib.xresampleFV(vp(xf), vp(o), 64, C.byref(g), p),
                 "xvarsampV": lambda p, o, g: lib.xvarsampV(vp(xc), vp(o), 64, C.c_double(1.0), C.byref(g), p)}
        strangers = {"xresampleV": (f, s), "xresampleFV": (v, s), "xvarsampV": (v, f)}
        for name, ptrs in strangers.items():
            for p in ptrs:
                out, got = np.full(96, np.nan, dtype=np.complex128), C.c_int(7)
                calls[name](p, out, got)
                assert lib.qh_wdsp_status() == -2 and got.value == 0 and np.all(np.isnan(out.real)), (name, made.index(p))
                getattr(lib, "destroy_" + name[1:])(p)
                assert lib.qh_wdsp_status() == -2, (name, made.index(p))
        assert lib.qh_wdsp_resampleV_max_out(s, 64) == -2
        assert lib.qh_wdsp_varsampV_max_out(v, 64, 1.0) == -2 and lib.qh_wdsp_varsampV_max_out(f, 64, 1.0) == -2
        # the refused calls and destroys left all three alone
        assert np.array_equal(rs("V", v, xc[:64]), rs("V", twins[0], xc[:64]))
        assert np.array_equal(rs("FV", f, xf[:64]), rs("FV", twins[1], xf[:64]))
        assert np.array_equal(vs(s, xc[:64]), vs(twins[2], xc[:64]))
        lib.destroy_resampleFV(f)
        assert lib.qh_wdsp_status() == 0
        made[1] = None
        assert np.array_equal(rs("V", v, xc[64:]), rs("V", twins[0], xc[64:]))
        assert np.array_equal(vs(s, xc[64:]), vs(twins[2], xc[64:]))
        lib.destroy_varsampV(s)
        assert lib.qh_wdsp_status() == 0
        made[2] = None
        assert np.array_equal(rs("V", v, xc[:64]), rs("V", twins[0], xc[:64]))
    finally:
        for p, t, kind in zip(made, twins, ("resampleV", "resampleFV", "varsampV")):
            for q in (p, t):
                if q:
                    getattr(lib, "destroy_" + kind)(q)
