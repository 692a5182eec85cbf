"""WDSP's diversity combiner through its EXT names (create_divEXT, xdivEXT, SetEXTDIV*, wdsp/div.c:104-187), bound with ctypes the way a
WDSP caller binds them, against the restatement tests/wdsp_div_ref.py bit for bit; the device form against the host form; and the whole
family in front of the receiver on the device: xanbEXT on two receivers -> xdivEXT -> fexchange0.  -m gpu."""
import ctypes as C

import numpy as np
import pytest

from quisk_amd import synth
from test_gpu_wdsp_dropin import _open
from wdsp_div_ref import Div

pytestmark = pytest.mark.gpu
D = C.c_double
U64 = np.uint64
INVALID = -2
CLIP32 = 2147483647.0


def _same(a, b):
    return np.array_equal(np.ascontiguousarray(a).view(U64), np.ascontiguousarray(b).view(U64))


def _rows(nr, n, seed):
    rng = np.random.default_rng(seed)
    return [rng.standard_normal(n) + 1j * rng.standard_normal(n) for _ in range(nr)]


def _ptrs(arrays):
    return (C.c_void_p * len(arrays))(*[a.ctypes.data if a is not None else None for a in arrays])


def _rotate(lib, id_, ir, qr):
    ir, qr = np.asarray(ir, dtype=np.float64), np.asarray(qr, dtype=np.float64)
    lib.SetEXTDIVRotate(id_, len(ir), ir.ctypes.data, qr.ctypes.data)
    assert lib.qh_wdsp_status() == 0, lib.qh_last_error()


def _x(lib, id_, rows, onto=None, n=None):
    """xdivEXT on copies of the rows; onto=k: out == in[k].  Returns (out, the rows as the call left them)."""
    ins = [np.array(r) for r in rows]
    n = len(ins[0]) if n is None else n
    out = ins[onto] if onto is not None else np.full(len(ins[0]), np.nan + 1j * np.nan)
    lib.xdivEXT(id_, n, _ptrs(ins), out.ctypes.data)
    return out, ins


def _ref(d, rows, onto=None):
    ins = [np.array(r) for r in rows]
    out = ins[onto] if onto is not None else np.full(len(ins[0]), np.nan + 1j * np.nan)
    return d.xdiv(ins, out)


def test_two_ids_with_different_nr_against_the_restatement(qh):
    lib = qh.load()
    lib.create_divEXT(3, 1, 2, 256)
    assert lib.qh_wdsp_status() == 0, lib.qh_last_error()
    lib.create_divEXT(17, 1, 5, 64)
    assert lib.qh_wdsp_status() == 0, lib.qh_last_error()
    a, b = Div(1, 2), Div(1, 5)
    try:
        ra, rb = _rows(2, 700, 1), _rows(5, 1300, 2)    # (nsamples is what counts, not the size the id was created with)
        out, ins = _x(lib, 3, ra)
        assert lib.qh_wdsp_status() == 0 and _same(out, ra[0]) and all(_same(p, q) for p, q in zip(ins, ra))     # created: output 0
        rng = np.random.default_rng(5)
        ia, qa, ib, qb = rng.uniform(-2, 2, 2), rng.uniform(-2, 2, 2), rng.uniform(-2, 2, 5), rng.uniform(-2, 2, 5)
        _rotate(lib, 3, ia, qa); a.SetRotate(2, ia, qa)
        _rotate(lib, 17, ib, qb); b.SetRotate(5, ib, qb)
        lib.SetEXTDIVOutput(3, 2); a.SetOutput(2)
        lib.SetEXTDIVOutput(17, 5); b.SetOutput(5)
        lib.flush_divEXT(3)
        assert lib.qh_wdsp_status() == 0
        for onto in (None, 0, 1):                       # buffers apart, then the callers' way: out == in[0], out == in[1]
            out, ins = _x(lib, 3, ra, onto)
            assert lib.qh_wdsp_status() == 0, lib.qh_last_error()
            assert _same(out, _ref(a, ra, onto)), onto
            assert all(_same(p, q) for k, (p, q) in enumerate(zip(ins, ra)) if k != onto)                       # the other inputs are left alone
            out, ins = _x(lib, 17, rb, onto)
            assert lib.qh_wdsp_status() == 0 and _same(out, _ref(b, rb, onto)), onto
        out, _ = _x(lib, 17, rb, onto=4)
        assert _same(out, _ref(b, rb, 4))
        # in[0] and in[1] the same buffer and out laid over it: both read the running sum
        ins = [np.array(ra[0])]
        lib.xdivEXT(3, 700, _ptrs([ins[0], ins[0]]), ins[0].ctypes.data)
        assert lib.qh_wdsp_status() == 0, lib.qh_last_error()
        same = np.array(ra[0])
        assert _same(ins[0], a.xdiv([same, same], same)) and not ins[0].view(U64).any()
        # a copy onto itself does nothing; run = 0 gives receiver 0; Buffsize stores and nsamples still counts
        lib.SetEXTDIVOutput(3, 1); a.SetOutput(1)
        out, _ = _x(lib, 3, ra, onto=1)
        assert lib.qh_wdsp_status() == 0 and _same(out, ra[1])
        out, _ = _x(lib, 3, ra, onto=0)
        assert _same(out, ra[1])
        lib.SetEXTDIVRun(3, 0); a.SetRun(0)
        lib.SetEXTDIVBuffsize(3, 16)
        out, _ = _x(lib, 3, ra)
        assert lib.qh_wdsp_status() == 0 and _same(out, ra[0])
        out, _ = _x(lib, 3, ra, n=0)                    # nothing to do
        assert lib.qh_wdsp_status() == 0 and np.isnan(out).all()
    finally:
        lib.destroy_divEXT(3)
        lib.destroy_divEXT(17)
    assert lib.qh_wdsp_status() == 0


def test_nr_and_output_in_either_order(qh):
    lib = qh.load()
    rows = _rows(3, 300, 7)
    ir, qr = [0.5, -1.0, 0.25], [1.0, 0.0, -0.75]
    got = []
    for id_, first in ((0, "nr"), (1, "output")):
        lib.create_divEXT(id_, 1, 2, 300)
        assert lib.qh_wdsp_status() == 0, lib.qh_last_error()
        try:
            _rotate(lib, id_, ir, qr)
            for what in ((first, "output") if first == "nr" else (first, "nr")):
                (lib.SetEXTDIVNr if what == "nr" else lib.SetEXTDIVOutput)(id_, 3)
                assert lib.qh_wdsp_status() == 0, (first, what, lib.qh_last_error())        # output 3 above nr 2 is no error until a call
            out, _ = _x(lib, id_, rows)
            assert lib.qh_wdsp_status() == 0, lib.qh_last_error()
            got.append(out)
        finally:
            lib.destroy_divEXT(id_)
    d = Div(1, 3)
    d.SetOutput(3)
    d.SetRotate(3, ir, qr)
    assert _same(got[0], _ref(d, rows)) and _same(got[1], got[0])


def test_refused_calls_are_reported_and_change_nothing(qh):
    lib = qh.load()
    rows = _rows(2, 100, 9)
    keep = np.full(100, 3.0 - 4.0j)
    out = keep.copy()
    for id_ in (-1, 32, 21):                            # out of range twice, then an id nobody created
        lib.xdivEXT(id_, 100, _ptrs(rows), out.ctypes.data)
        assert lib.qh_wdsp_status() == INVALID and b"DIV id" in lib.qh_last_error()
        for name, arg in (("SetEXTDIVRun", 1), ("SetEXTDIVBuffsize", 64), ("SetEXTDIVNr", 2), ("SetEXTDIVOutput", 1)):
            getattr(lib, name)(id_, arg)
            assert lib.qh_wdsp_status() == INVALID, (name, id_)
        one = np.ones(2)
        lib.SetEXTDIVRotate(id_, 2, one.ctypes.data, one.ctypes.data)
        assert lib.qh_wdsp_status() == INVALID
        lib.flush_divEXT(id_)
        assert lib.qh_wdsp_status() == INVALID
        lib.destroy_divEXT(id_)
        assert lib.qh_wdsp_status() == INVALID
        assert lib.qh_wdsp_xdivEXT_device(id_, 100, _ptrs(rows), out.ctypes.data, None) == INVALID
    for args in ((32, 1, 2, 64), (4, 1, 0, 64), (4, 1, 9, 64), (4, 1, 2, -1)):
        lib.create_divEXT(*args)
        assert lib.qh_wdsp_status() == INVALID, args
    lib.xdivEXT(4, 100, _ptrs(rows), out.ctypes.data)   # ... so id 4 was not created
    assert lib.qh_wdsp_status() == INVALID and _same(out, keep)
    lib.create_divEXT(4, 1, 2, 64)
    assert lib.qh_wdsp_status() == 0, lib.qh_last_error()
    try:
        lib.create_divEXT(4, 1, 2, 64)                  # twice
        assert lib.qh_wdsp_status() == INVALID
        ir, qr = np.array([0.5, 2.0]), np.array([-1.0, 0.25])
        _rotate(lib, 4, ir, qr)
        lib.SetEXTDIVOutput(4, 2)
        d = Div(1, 2)
        d.SetOutput(2)
        d.SetRotate(2, ir, qr)
        want = _ref(d, rows)
        bad = np.array([1.0, np.nan])
        big = np.ones(9)
        for call in (lambda: lib.SetEXTDIVNr(4, 0), lambda: lib.SetEXTDIVNr(4, 9), lambda: lib.SetEXTDIVOutput(4, 9), lambda: lib.SetEXTDIVOutput(4, -1),
                     lambda: lib.SetEXTDIVRotate(4, 9, big.ctypes.data, big.ctypes.data), lambda: lib.SetEXTDIVRotate(4, 2, None, qr.ctypes.data),
                     lambda: lib.SetEXTDIVRotate(4, 2, bad.ctypes.data, qr.ctypes.data), lambda: lib.SetEXTDIVBuffsize(4, -1)):
            call()
            assert lib.qh_wdsp_status() == INVALID
            got, _ = _x(lib, 4, rows)                   # every setting is as it was
            assert lib.qh_wdsp_status() == 0 and _same(got, want)
        # pointers: a null one among those the call reads, out overlapping an input without being it, nsamples < 0
        buf = np.concatenate([rows[0], rows[1]])
        for ins, o, n in (([rows[0], None], out, 100), (None, out, 100), ([rows[0], rows[1]], None, 100), ([rows[0], rows[1]], out, -1),
                          ([buf[:100], buf[100:]], buf[50:150], 100), ([buf[:100], buf[100:]], buf[1:101], 100)):
            before = buf.copy()
            lib.xdivEXT(4, n, _ptrs(ins) if ins is not None else None, o.ctypes.data if o is not None else None)
            assert lib.qh_wdsp_status() == INVALID, (n,)
            assert _same(out, keep) and _same(buf, before)
        lib.SetEXTDIVOutput(4, 0)                       # only in[0] is read now: a null in[1] and an out over in[1] are the caller's business
        lib.xdivEXT(4, 100, _ptrs([rows[0], None]), out.ctypes.data)
        assert lib.qh_wdsp_status() == 0 and _same(out, rows[0])
        out[:] = keep
        lib.SetEXTDIVOutput(4, 2)
        lib.SetEXTDIVNr(4, 1)                           # output 2 above nr 1: refused at the call, nothing written
        lib.xdivEXT(4, 100, _ptrs(rows), out.ctypes.data)
        assert lib.qh_wdsp_status() == INVALID and _same(out, keep)
    finally:
        lib.destroy_divEXT(4)
    assert lib.qh_wdsp_status() == 0
    lib.SetEXTDIVRun(4, 1)                              # destroyed
    assert lib.qh_wdsp_status() == INVALID


def test_device_form_equals_the_host_form(qh):
    import torch
    lib = qh.load()
    nr, n = 3, 1500
    rows = _rows(nr, n, 11)
    ir, qr = np.array([1.0, -0.5, 0.3]), np.array([0.0, 0.7, -1.1])
    for id_ in (6, 7):
        lib.create_divEXT(id_, 1, nr, n)
        assert lib.qh_wdsp_status() == 0, lib.qh_last_error()
        _rotate(lib, id_, ir, qr)
    s = torch.cuda.Stream()
    try:
        for output in (3, 1, 0):
            for id_ in (6, 7):
                lib.SetEXTDIVOutput(id_, output)
            for onto in (None, 0, 2):
                want, _ = _x(lib, 6, rows, onto)
                assert lib.qh_wdsp_status() == 0, lib.qh_last_error()
                with torch.cuda.stream(s):
                    d = [torch.from_numpy(r).cuda() for r in rows]
                    o = d[onto] if onto is not None else torch.full((n + 8,), 5.0 + 0j, dtype=torch.complex128, device="cuda")
                    ptrs = (C.c_void_p * nr)(*[t.data_ptr() for t in d])
                    assert lib.qh_wdsp_xdivEXT_device(7, n, ptrs, o.data_ptr(), s.cuda_stream) == 0, lib.qh_last_error()
                    got = o.cpu().numpy()               # (on `s`: ordered behind the id's work by the call itself)
                    left = [t.cpu().numpy() for t in d]
                s.synchronize()
                assert _same(got[:n], want), (output, onto)
                assert onto is not None or np.all(got[n:] == 5.0)
                assert all(_same(left[k], rows[k]) for k in range(nr) if k != onto)
        with torch.cuda.stream(s):                      # out inside an input: refused, nothing written
            d = torch.from_numpy(np.concatenate(rows)).cuda()
            keep = d.clone()
            ptrs = (C.c_void_p * nr)(*[d.data_ptr() + 16 * n * k for k in range(nr)])
            lib.SetEXTDIVOutput(7, 3)
            assert lib.qh_wdsp_xdivEXT_device(7, n, ptrs, d.data_ptr() + 16 * 5, s.cuda_stream) == INVALID
            assert lib.qh_wdsp_status() == INVALID
        s.synchronize()
        assert torch.equal(d.view(torch.int64), keep.view(torch.int64))
    finally:
        lib.destroy_divEXT(6)
        lib.destroy_divEXT(7)


def test_blankers_combiner_and_receiver_on_the_device(qh):
    """xanbEXT on each of two receivers -> xdivEXT -> fexchange0, every step on device buffers and nothing waited for in between (channel
    0), against the same three steps through the host-pointer names (channel 1): the same bits."""
    import torch
    lib = qh.load()
    in_size, rate, nblk = 256, 48000, 16
    n = in_size * nblk
    rng = np.random.default_rng(31)
    base = synth.make_input_numpy(1, n, fs=float(rate))[0] * CLIP32
    rx = [base + 0.05 * CLIP32 * (rng.standard_normal(n) + 1j * rng.standard_normal(n)),
          base * np.exp(0.9j) + 0.05 * CLIP32 * (rng.standard_normal(n) + 1j * rng.standard_normal(n))]
    for r in rx:
        for p in rng.integers(100, n - 10, size=6):
            r[p:p + 2] += 40.0 * CLIP32
    prm = (D(float(rate)), D(1e-4), D(1e-4), D(1e-4), D(0.05), D(20.0))
    ir, qr = np.array([1.0, 0.6]), np.array([0.0, -0.8])
    for ch in (0, 1):
        _open(lib, ch, in_size, 256, rate, nbp=True, nc=256)
        lib.qh_wdsp_set_parameter(ch, in_size, 1)
    for id_ in range(4):                                # ANB 0, 1: the device chain's receivers; 2, 3: the host chain's
        lib.create_anbEXT(id_, 1, in_size, *prm)
        assert lib.qh_wdsp_status() == 0, lib.qh_last_error()
    for id_ in (0, 1):
        lib.create_divEXT(id_, 1, 2, in_size)
        assert lib.qh_wdsp_status() == 0, lib.qh_last_error()
        _rotate(lib, id_, ir, qr)
        lib.SetEXTDIVOutput(id_, 2)
    s = torch.cuda.Stream()
    got_d, got_h = [], []
    try:
        for b in range(nblk):
            seg = [np.ascontiguousarray(r[b * in_size:(b + 1) * in_size]) for r in rx]
            with torch.cuda.stream(s):
                d = [torch.from_numpy(x).cuda() for x in seg]
                work = torch.zeros(3 * in_size, dtype=torch.complex128, device="cuda")
                for k in range(2):                      # in place, the callers' way
                    assert lib.qh_wdsp_xanbEXT_device(k, d[k].data_ptr(), d[k].data_ptr(), s.cuda_stream) == 0, lib.qh_last_error()
                ptrs = (C.c_void_p * 2)(d[0].data_ptr(), d[1].data_ptr())
                assert lib.qh_wdsp_xdivEXT_device(0, in_size, ptrs, work.data_ptr(), s.cuda_stream) == 0, lib.qh_last_error()
                m = lib.qh_wdsp_fexchange0_device(0, C.c_void_p(work.data_ptr()), in_size, C.c_void_p(s.cuda_stream))
                assert lib.qh_wdsp_status() == 0, lib.qh_last_error()
                got_d.append(work[:m].cpu())
            h = [x.copy() for x in seg]
            hw = np.zeros(3 * in_size, dtype=np.complex128)
            for k in range(2):
                lib.xanbEXT(2 + k, h[k].ctypes.data, h[k].ctypes.data)
                assert lib.qh_wdsp_status() == 0, lib.qh_last_error()
            lib.xdivEXT(1, in_size, _ptrs(h), hw.ctypes.data)
            assert lib.qh_wdsp_status() == 0, lib.qh_last_error()
            m = lib.wdspFexchange0(1, hw.ctypes.data_as(C.c_void_p), in_size)
            got_h.append(hw[:m].copy())
        s.synchronize()
    finally:
        for id_ in range(4):
            lib.destroy_anbEXT(id_)
        for id_ in (0, 1):
            lib.destroy_divEXT(id_)
        for ch in (0, 1):
            lib.qh_wdsp_set_parameter(ch, 0, 0)
            lib.wdspFexchange0(ch, None, 0)             # not in use: the shim rewinds its ring, nothing is left for the next test
            lib.CloseChannel(ch)
    yd, yh = np.concatenate([t.numpy() for t in got_d]), np.concatenate(got_h)
    assert yd.size == yh.size and yd.size > 0
    assert np.abs(yh).max() > 1e6                       # there is audio in it
    assert _same(yd, yh)
