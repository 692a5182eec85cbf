"""qh_div_* (WDSP's diversity combiner, xdiv, wdsp/div.c:67-95) against the literal restatement tests/wdsp_div_ref.py, bit for bit: every
comparison is on the uint64 view of the doubles.  The block keeps nothing from call to call and no sample looks at another one, so what
can go wrong is the order and the rounding of the sum, the ragged ends of a wavefront (64) and of the kernel's tile (1024 samples, four
per lane), the path of every nr (each is a loop unrolled on its own), the rows a call may and may not touch, and offsets beyond 2^31.
Rows carry a sentinel pattern beyond n and in every row the call must not touch; it has to survive.  -m gpu."""
import functools

import numpy as np
import pytest

from wdsp_div_ref import mix

pytestmark = pytest.mark.gpu

U64 = np.uint64
SENT = 0x7FF8DEADBEEF0001                               # a NaN nobody computes
INVALID = -2
SIZES = [1, 2, 63, 64, 255, 256, 257, 1000, 1023, 1024, 1025, 2500]


def _bits(z):
    return np.ascontiguousarray(z, dtype=np.complex128).view(U64)


def _same(a, b):
    return np.array_equal(_bits(a), _bits(b))


@functools.lru_cache(maxsize=None)
def _input(ng, rows, n, seed):
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((ng, rows, n)) + 1j * rng.standard_normal((ng, rows, n))
    x.setflags(write=False)
    return x


def _rot(seed):
    """eight rotate pairs: 0, +-1, (0, 1) and random values"""
    rng = np.random.default_rng(seed)
    ir, qr = rng.uniform(-2, 2, 8), rng.uniform(-2, 2, 8)
    ir[:4], qr[:4] = [1.0, 0.0, -1.0, 0.0], [0.0, 1.0, 0.0, 0.0]
    p = rng.permutation(8)
    return ir[p], qr[p]


def _settings(run, nr, output, seed):
    ir, qr = _rot(seed)
    return dict(run=run, nr=nr, output=output, ir=ir, qr=qr)


def _apply(div, sets):
    for g, s in enumerate(sets):
        div.set_run(s["run"], g)
        div.set_nr(s["nr"], g)
        div.set_output(s["output"], g)
        div.set_rotate(s["ir"], s["qr"], g)


def _want(sets, x, onto=None):
    """the restatement, group by group; x [ng, rows, n]"""
    return np.stack([mix(s["run"], s["nr"], s["output"], s["ir"], s["qr"], x[g], onto=onto) for g, s in enumerate(sets)])


def _device(div, sets, x, rx_stride=None, group_stride=None, out_stride=None, onto=None, expect=0):
    """x [ng, rows, n] laid out in a sentinel-filled device buffer with these strides, one call, and the checks every call gets: rows the
    call does not write and everything beyond n keep their bits.  Returns the output rows [ng, n] (what lies there if the call is refused)."""
    import torch
    ng, rows, n = x.shape
    rx = rx_stride or n + 5
    gs = group_stride or rows * rx + 3
    os_ = gs if onto is not None else (out_stride or n + 7)
    host = np.full(2 * ((ng - 1) * gs + rows * rx + 16), SENT, dtype=U64).view(np.complex128)
    for g in range(ng):
        for i in range(rows):
            host[g * gs + i * rx:g * gs + i * rx + n] = x[g, i]
    buf = torch.from_numpy(host).cuda()
    if onto is None:
        obuf = torch.from_numpy(np.full(2 * (ng * os_ + 16), SENT, dtype=U64).view(np.complex128)).cuda()
        optr = obuf.data_ptr()
    else:
        obuf, optr = buf, buf.data_ptr() + onto * rx * 16
    before_in = buf.cpu().numpy().copy()
    before_out = obuf.cpu().numpy().copy()
    rc = div._L.qh_div_process(div._h, buf.data_ptr(), rx, gs, optr, os_, n)
    div.synchronize()
    assert rc == expect, (rc, div._L.qh_last_error())
    after_in, after_out = buf.cpu().numpy(), obuf.cpu().numpy()
    o0 = onto * rx if onto is not None else 0
    written = np.zeros(after_out.shape, dtype=bool)
    for g in range(ng):
        written[o0 + g * os_:o0 + g * os_ + n] = True
    assert np.array_equal(_bits(after_out)[np.repeat(~written, 2)], _bits(before_out)[np.repeat(~written, 2)]), "the call wrote outside its output rows"
    if onto is None:
        assert np.array_equal(_bits(after_in), _bits(before_in)), "the call wrote to its input"
    if rc != 0:
        assert np.array_equal(_bits(after_out), _bits(before_out)), "a refused call wrote"
    return np.stack([after_out[o0 + g * os_:o0 + g * os_ + n] for g in range(ng)])


THREE = [_settings(1, 1, 1, 11), _settings(1, 2, 1, 12), _settings(1, 8, 8, 13)]       # mix of 1, a copy of receiver 1 of 2, mix of 8


@pytest.fixture(scope="module")
def three(qh):
    div = qh.WdspDiversity(3, 2)
    yield div
    div.close()


@pytest.mark.parametrize("n", SIZES)
def test_three_groups_with_different_settings_in_one_launch(three, n):
    x = _input(3, 8, n, 100 + n)
    _apply(three, THREE)
    assert _same(_device(three, THREE, x), _want(THREE, x))
    second = [dict(THREE[0], run=0), dict(THREE[1], output=2), THREE[2]]                # run = 0 beside a mix of 2 and a mix of 8
    _apply(three, second)
    y = _device(three, second, x)
    assert _same(y, _want(second, x)) and _same(y[0], x[0, 0])


def test_n_zero_leaves_everything_alone(three):
    _apply(three, THREE)
    x = _input(3, 8, 4, 5)
    import torch
    buf = torch.from_numpy(np.array(x)).cuda()
    out = torch.full((3, 4), 7.0 + 0j, dtype=torch.complex128, device="cuda")
    three.process_ptr(buf.data_ptr(), 4, 32, out.data_ptr(), 4, 0)
    three.process_ptr(0, 0, 0, 0, 0, 0)                 # (no rows are needed for no samples)
    three.synchronize()
    assert _same(buf.cpu().numpy(), x) and _same(out.cpu().numpy(), np.full((3, 4), 7.0 + 0j))
    assert three.process_host(np.zeros((3, 8, 0), dtype=np.complex128)).shape == (3, 0)


@pytest.mark.parametrize("n", [64, 1025, 2049])
def test_every_nr_mixes_and_copies(qh, n):
    """nr = 1 .. 8, each an unrolled path of its own, at a whole wavefront, just past a tile and past two"""
    div = qh.WdspDiversity(8, 1)
    try:
        sets = [_settings(1, g + 1, g + 1, 20 + g) for g in range(8)]
        _apply(div, sets)
        x = _input(8, 8, n, 300 + n)
        assert _same(_device(div, sets, x), _want(sets, x))
        assert _same(div.process_host(x), _want(sets, x))
        sets = [_settings(1, g + 1, g, 30 + g) for g in range(8)]                       # every group copies its last receiver
        _apply(div, sets)
        y = _device(div, sets, x)
        assert _same(y, _want(sets, x)) and all(_same(y[g], x[g, g]) for g in range(8))
    finally:
        div.close()


def test_the_rounding_and_the_signed_zero_cases(qh):
    div = qh.WdspDiversity(2, 1)
    try:
        v = 1.0 + 2.0 ** -30
        div.set_output(1)
        div.set_rotate([v], [1.0], 0)
        div.set_rotate([-1.0], [-1.0], 1)
        x = np.zeros((2, 1, 70), dtype=np.complex128)
        x[0] = v + 1j
        y = div.process_host(x)
        assert np.all(y[0].real == 2.0 ** -29) and np.all(y[0].imag == v + v)          # a fused multiply-add would give 2^-29 + 2^-60
        assert not _bits(y[1]).any()                                                    # +0.0, never -0.0
        sets = [dict(run=1, nr=1, output=1, ir=[v], qr=[1.0]), dict(run=1, nr=1, output=1, ir=[-1.0], qr=[-1.0])]
        assert _same(y, _want(sets, x))
    finally:
        div.close()


@pytest.mark.parametrize("n", [1, 257, 1500])
def test_out_laid_over_a_receiver(qh, n):
    div = qh.WdspDiversity(2, 3)
    try:
        x = _input(2, 3, n, 400 + n)
        differed = False
        for k in range(3):
            sets = [_settings(1, 3, 3, 40 + k), _settings(1, 3, 3, 50 + k)]
            _apply(div, sets)
            want = _want(sets, x, onto=k)
            assert _same(_device(div, sets, x, onto=k), want), k
            assert _same(div.process_host(x, onto=k), want), k
            differed = differed or not _same(want, _want(sets, x))
        assert differed                                 # (the aliasing made a difference to compare)
        # copy mode onto in[output]: nothing is written; onto another receiver: a copy
        sets = [_settings(1, 3, 1, 60), _settings(1, 3, 1, 61)]
        _apply(div, sets)
        y = _device(div, sets, x, onto=1)
        assert _same(y, x[:, 1]) and _same(y, _want(sets, x, onto=1))
        y = _device(div, sets, x, onto=2)
        assert _same(y, x[:, 1]) and _same(y, _want(sets, x, onto=2))
        assert _same(div.process_host(x, onto=2), x[:, 1])
        # one group mixes, the other copies the very row: the mix is the aliased one, the copy does nothing
        sets = [_settings(1, 3, 3, 62), _settings(0, 3, 3, 63)]
        _apply(div, sets)
        assert _same(_device(div, sets, x, onto=0), _want(sets, x, onto=0))
    finally:
        div.close()


def test_strides_well_above_n(qh):
    div = qh.WdspDiversity(3, 2)
    try:
        _apply(div, THREE)
        x = _input(3, 8, 300, 7)
        assert _same(_device(div, THREE, x, rx_stride=1111, group_stride=8 * 1111 + 4097, out_stride=5003), _want(THREE, x))
    finally:
        div.close()


def test_rows_beyond_two_to_the_31_samples_apart(qh):
    """two groups whose rows lie 2^31 + 64 complex samples apart inside one allocation: g * group_stride does not fit 32 bits"""
    import torch
    n, nr = 300, 2
    gs = 2 ** 31 + 64
    need = (gs + nr * n + 64) * 16
    free, _ = torch.cuda.mem_get_info()
    if free < need + (1 << 30):
        print("skipped: %.1f GB free, the case needs %.1f GB" % (free / 1e9, need / 1e9))
        pytest.skip("not enough free device memory for rows 2^31 + 64 samples apart")
    big = torch.empty(gs + nr * n + 64, dtype=torch.complex128, device="cuda")
    sent = torch.full((2 * (nr * n + 64),), SENT, dtype=torch.int64, device="cuda").view(torch.complex128)
    x = _input(2, nr, n, 9)
    sets = [_settings(1, 2, 2, 70), _settings(1, 2, 2, 71)]
    div = qh.WdspDiversity(2, 2)
    try:
        _apply(div, sets)
        for onto in (None, 1):
            for g in range(2):
                big[g * gs:g * gs + nr * n + 64] = sent
                for i in range(nr):
                    big[g * gs + i * n:g * gs + i * n + n] = torch.from_numpy(np.array(x[g, i])).cuda()
            if onto is None:
                out = torch.full((2 * 2 * (n + 8),), SENT, dtype=torch.int64, device="cuda").view(torch.complex128)
                div.process_ptr(big.data_ptr(), n, gs, out.data_ptr(), n + 8, n)
                div.synchronize()
                o = out.cpu().numpy().reshape(2, n + 8)
                assert _same(o[:, :n], _want(sets, x))
                assert np.all(_bits(o[:, n:]) == SENT)
            else:
                div.process_ptr(big.data_ptr(), n, gs, big.data_ptr() + onto * n * 16, gs, n)
                div.synchronize()
                want = _want(sets, x, onto=onto)
                for g in range(2):
                    blk = big[g * gs:g * gs + nr * n + 64].cpu().numpy()
                    assert _same(blk[onto * n:onto * n + n], want[g]), g
                    assert _same(blk[:onto * n], x[g, :onto].reshape(-1))               # the receivers before it are as they were
                    assert np.all(_bits(blk[nr * n:]) == SENT)
    finally:
        div.close()
        del big
        torch.cuda.empty_cache()


def test_setters_act_on_the_next_call_and_get_returns_them(qh):
    div = qh.WdspDiversity(3, 2)
    try:
        for g in range(3):                              # create_div: output 0, rotates 0
            s = div.get(g)
            assert (s["run"], s["nr"], s["output"]) == (1, 2, 0) and not s["irotate"].any() and not s["qrotate"].any()
        x = _input(3, 4, 130, 3)
        assert _same(div.process_host(x), x[:, 0])
        div.set_output(2)                               # -1: every group; mixing before any rotate is set gives zeros
        assert not _bits(div.process_host(x)).any()
        ir, qr = _rot(80)
        div.set_rotate(ir[:3], qr[:3])                  # three values although nr is 2: the call's own count
        sets = [dict(run=1, nr=2, output=2, ir=ir[:3], qr=qr[:3])] * 3
        assert _same(div.process_host(x), _want(sets, x))
        div.set_nr(3, 1)                                # nr after output: group 1 now copies receiver 2 of 3
        sets = [sets[0], dict(sets[0], nr=3), sets[0]]
        y = div.process_host(x)
        assert _same(y, _want(sets, x)) and _same(y[1], x[1, 2])
        div.set_output(3, 1)                            # ... and mixes the three
        sets[1] = dict(sets[1], output=3)
        assert _same(div.process_host(x), _want(sets, x))
        div.set_run(0, 2)
        assert _same(div.process_host(x)[2], x[2, 0])
        s = div.get(1)
        assert (s["run"], s["nr"], s["output"]) == (1, 3, 3)
        assert np.array_equal(s["irotate"][:3], ir[:3]) and np.array_equal(s["qrotate"][:3], qr[:3]) and not s["irotate"][3:].any()
        assert div.get(2)["run"] == 0 and div.get(0)["output"] == 2
    finally:
        div.close()


def _snapshot(div):
    return [(s["run"], s["nr"], s["output"], s["irotate"].tobytes(), s["qrotate"].tobytes()) for s in (div.get(g) for g in range(div.ngroups))]


def test_refusals_write_nothing_and_change_nothing(qh):
    lib = qh.load()
    div = qh.WdspDiversity(2, 2)
    try:
        sets = [_settings(1, 2, 2, 90), _settings(1, 2, 2, 91)]
        _apply(div, sets)
        keep = _snapshot(div)
        ok = np.ones(8)
        bad = ok.copy()
        bad[1] = np.inf
        nan = ok.copy()
        nan[0] = np.nan
        for call in (lambda: lib.qh_div_set_nr(div._h, 0, 0), lambda: lib.qh_div_set_nr(div._h, -1, 9), lambda: lib.qh_div_set_output(div._h, 1, 9),
                     lambda: lib.qh_div_set_output(div._h, 1, -1), lambda: lib.qh_div_set_rotate(div._h, 0, 9, ok.ctypes.data, ok.ctypes.data),
                     lambda: lib.qh_div_set_rotate(div._h, 0, -1, ok.ctypes.data, ok.ctypes.data),
                     lambda: lib.qh_div_set_rotate(div._h, 0, 2, None, ok.ctypes.data), lambda: lib.qh_div_set_rotate(div._h, 0, 2, ok.ctypes.data, None),
                     lambda: lib.qh_div_set_rotate(div._h, -1, 2, bad.ctypes.data, ok.ctypes.data),
                     lambda: lib.qh_div_set_rotate(div._h, 1, 1, ok.ctypes.data, nan.ctypes.data), lambda: lib.qh_div_set_run(div._h, 2, 1)):
            assert call() == INVALID
            assert _snapshot(div) == keep
        assert lib.qh_div_set_rotate(div._h, 0, 1, ok.ctypes.data, bad.ctypes.data) == 0       # (the value that is not finite lies beyond nr)
        _apply(div, sets)
        keep = _snapshot(div)
        x = _input(2, 2, 200, 4)
        assert _same(_device(div, sets, x), _want(sets, x))
        # an output row that starts inside a receiver's row, one that is another group's row, strides below n, n < 0
        import torch
        n = 200
        buf = torch.from_numpy(np.array(x).reshape(-1)).cuda()
        mine = buf.clone()
        p = buf.data_ptr()
        sep = torch.zeros(2 * n, dtype=torch.complex128, device="cuda")
        for args in ((p, n, 2 * n, p + 16 * 7, 2 * n, n),                  # seven samples into receiver 0
                     (p, n, 2 * n, p + 16 * (n - 1), 2 * n, n),            # straddles receivers 0 and 1
                     (p, n, 2 * n, p + 16 * 2 * n, 2 * n, n),              # group 0 onto group 1's receiver 0 (and group 1 beyond the rows)
                     (p, n, 2 * n, p + 16 * n, n, n),                      # receiver 1 of group 0, but out_stride is not group_stride
                     (p, n - 1, 2 * n, sep.data_ptr(), n, n), (p, n, n - 1, sep.data_ptr(), n, n), (p, n, 2 * n, sep.data_ptr(), n - 1, n),
                     (p, n, 2 * n, sep.data_ptr(), n, -1), (0, n, 2 * n, sep.data_ptr(), n, n), (p, n, 2 * n, 0, n, n)):
            assert lib.qh_div_process(div._h, *args) == INVALID, args
        div.synchronize()
        assert torch.equal(buf.view(torch.int64), mine.view(torch.int64)) and not sep.view(torch.int64).any().item()
        # a receiver row that is not read may be written: group-wise copies of receiver 0 with the output on receiver 1
        div.set_output(0)
        copies = [dict(s, output=0) for s in sets]
        assert _same(_device(div, copies, x, onto=1), x[:, 0])
        # output > nr at the call: refused whole, nothing written; the setters stayed order-free
        div.set_output(2)
        div.set_nr(1, 1)
        assert div.get(1)["output"] == 2 and div.get(1)["nr"] == 1
        keep = _snapshot(div)
        _device(div, [sets[0], dict(sets[1], nr=1)], x, expect=INVALID)
        with pytest.raises(qh.QuiskHipError):
            div.process_host(x)
        assert _snapshot(div) == keep
        div.set_run(0, 1)                               # ... but run = 0 never looks at output (div.c:93-94)
        y = _device(div, [sets[0], dict(sets[1], nr=1, run=0)], x)
        assert _same(y[1], x[1, 0]) and _same(y[0], _want(sets[:1], x[:1])[0])
    finally:
        div.close()
    for args in ((0, 1, 0), (0, 1, 9), (0, 0, 2)):
        assert not lib.qh_div_create(0, args[1], 1, args[2], None)


def test_no_group_sees_another(qh):
    div = qh.WdspDiversity(3, 4)
    try:
        sets = [_settings(1, 4, 4, 95), _settings(1, 4, 4, 96), _settings(1, 4, 4, 97)]
        _apply(div, sets)
        x = np.array(_input(3, 4, 1300, 6))
        y0 = _device(div, sets, x)
        sets[1] = _settings(1, 4, 4, 98)
        _apply(div, sets[:2])
        x[1] = _input(1, 4, 1300, 8)[0]
        y1 = _device(div, sets, x)
        assert _same(y0[0], y1[0]) and _same(y0[2], y1[2]) and not _same(y0[1], y1[1])
        assert _same(y1, _want(sets, x))
    finally:
        div.close()
