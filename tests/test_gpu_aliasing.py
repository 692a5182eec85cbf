"""The in-place contract of the device entry points (include/quiskhip.h): which of them may be handed output rows that lie over their
input rows, and that every other one refuses such a call -- QH_ERR_INVALID, a message that names the entry point and the overlap, not a
byte written, no state moved -- while layouts whose rows are disjoint (interleaved rows, a matrix right behind the other's last row, rows
that touch without sharing a byte) are accepted and compute what the same call far apart computes.  -m gpu.

Every layout lies inside ONE allocation with room for the worst case: a call that is not refused must still stay inside it."""
import ctypes as C
import os

import numpy as np
import pytest
import torch          # before libquiskhip: one HIP runtime per process (torch's)

from conftest import rel_rms
from quisk_amd import synth

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
GOLD = os.path.join(os.path.dirname(__file__), "golden", "filter_golden.npz")
GUARD = 256                                 # bytes in front of and behind every layout
SENTINEL = 0xA5
REFUSED = ["a_same", "b_plus_one", "c_minus_k", "f_touch"]
ACCEPTED = ["d_interleaved", "e_behind", "f_clear"]
NCH = 3


def _up(x, a=16):
    return (x + a - 1) // a * a


def layout(kind, nch, lin, lout, uo):
    """(total bytes, in_off, in_stride, out_off, out_stride), all in bytes, for an input matrix of nch rows of lin bytes and an output
    matrix of nch rows of lout bytes whose samples are uo bytes."""
    S = _up(max(lin, lout))
    if kind == "a_same":                    # out == in, one stride
        i0, si, o0, so = GUARD, S, GUARD, S
    elif kind == "b_plus_one":              # out = in + one sample
        i0, si, o0, so = GUARD, S, GUARD + uo, S
    elif kind == "c_minus_k":               # the output starts ahead of the input; its tail lies over the input's head
        k = _up(max(lout // 2, 16))
        i0, si, o0, so = GUARD + k, S, GUARD, S
    elif kind == "d_interleaved":           # rows interleaved: disjoint
        i0, si, o0, so = GUARD, 2 * S, GUARD + S, 2 * S
    elif kind == "e_behind":                # the output matrix right behind the input's last row: nch * in_stride from in reaches into it
        si = _up(lin) + 48
        i0, so = GUARD, S
        o0 = i0 + (nch - 1) * si + lin
    elif kind in ("f_touch", "f_clear"):    # the output's last row ends one sample into (exactly at) the input's first row
        si, so = S, S
        i0 = GUARD + _up((nch - 1) * so + lout)
        o0 = i0 - ((nch - 1) * so + lout) + (uo if kind == "f_touch" else 0)
    else:
        raise ValueError(kind)
    assert i0 >= GUARD and o0 >= GUARD and o0 % uo == 0
    total = max(i0 + (nch - 1) * si + lin, o0 + (nch - 1) * so + lout) + GUARD
    return total, i0, si, o0, so


class Arena:
    """One device allocation holding a layout, filled with the sentinel, the input rows written in."""

    def __init__(self, total):
        self.buf = torch.full((total,), SENTINEL, dtype=torch.uint8, device=DEV)
        self.base = self.buf.data_ptr()

    def put(self, off, stride, rows):
        for c, r in enumerate(rows):
            b = np.ascontiguousarray(r).view(np.uint8)
            self.buf[off + c * stride:off + c * stride + b.size].copy_(torch.from_numpy(b.copy()))

    def get(self, off, stride, nbytes, dtype, nch):
        torch.cuda.synchronize()
        h = self.buf.cpu().numpy()
        return np.stack([h[off + c * stride:off + c * stride + nbytes].copy().view(dtype) for c in range(nch)])

    def snapshot(self):
        torch.cuda.synchronize()
        return self.buf.clone()


def noise(seed, nch, n, dt=np.complex128):
    rng = np.random.default_rng(seed)
    return (rng.standard_normal((nch, n)) + 1j * rng.standard_normal((nch, n))).astype(dt)


def far_apart(call, x, lout, odt):
    """The same call with the two matrices in allocations of their own: its output rows."""
    nch = x.shape[0]
    lin = x.shape[1] * x.itemsize
    xi = torch.from_numpy(np.ascontiguousarray(x).view(np.uint8).reshape(nch, lin).copy()).to(DEV)
    yo = torch.full((nch, max(lout, 16)), SENTINEL, dtype=torch.uint8, device=DEV)
    torch.cuda.synchronize()
    call(xi.data_ptr(), lin, yo.data_ptr(), max(lout, 16))
    torch.cuda.synchronize()
    return yo.cpu().numpy()[:, :lout].copy().view(odt)


# ---- the entry points: make() -> object, call(obj, in_ptr, in_stride_bytes, out_ptr, out_stride_bytes, n), out bytes per row ----------
class Spec:
    def __init__(self, name, make, call, n_out, ui, uo, idt, odt, warm=0):
        self.name, self.make, self.call, self.n_out, self.ui, self.uo, self.idt, self.odt, self.warm = (
            name, make, call, n_out, ui, uo, idt, odt, warm)


def _taps(key):
    return np.load(GOLD)[key]


def spec_fir(qh, decim, dtype):
    es = 16 if dtype == 0 else 8
    return Spec("qh_fir_process", lambda: qh.FirBank(NCH, _taps("taps98"), decim, dtype=dtype),
                lambda o, i, si, p, so, n: o.process_ptr(i, si // es, n, p, so // es), lambda o, n: o.out_count(n),
                es, es, np.complex128 if es == 16 else np.complex64, np.complex128 if es == 16 else np.complex64)


def spec_rat(qh, key, interp, decim, dtype):
    es = 16 if dtype == 0 else 8
    return Spec("qh_rat_process", lambda: qh.RationalFir(NCH, _taps(key), interp, decim, dtype=dtype),
                lambda o, i, si, p, so, n: o.process_ptr(i, si // es, n, p, so // es), lambda o, n: o.out_count(n),
                es, es, np.complex128 if es == 16 else np.complex64, np.complex128 if es == 16 else np.complex64)


def spec_hbc(qh, nstage, dtype):
    es = 16 if dtype == 0 else 8
    return Spec("qh_hbc_process", lambda: qh.HalfBandCascade(NCH, nstage, dtype=dtype),
                lambda o, i, si, p, so, n: o.process_ptr(i, si // es, n, p, so // es), lambda o, n: n >> nstage,
                es, es, np.complex128 if es == 16 else np.complex64, np.complex128 if es == 16 else np.complex64)


def spec_nb(qh):
    return Spec("qh_nb_process", lambda: qh.NoiseBlanker(NCH, 192000, 2),
                lambda o, i, si, p, so, n: o.process_ptr(i, si // 16, p, so // 16, n), lambda o, n: n,
                16, 16, np.complex128, np.complex128)


def spec_qrx(qh, fs):
    return Spec("qh_qrx_process", lambda: qh.QuiskRxBank(NCH, fs, 3),
                lambda o, i, si, p, so, n: o.process_ptr(i, si // 16, n, p, so // 16), lambda o, n: o.out_count(n),
                16, 16, np.complex128, np.complex128)


def spec_qps(qh, fs, play):
    return Spec("qh_qps_process", lambda: qh.QuiskProcessBank(NCH, fs, 3, 2700, playback_rate=play),
                lambda o, i, si, p, so, n: o.process_ptr(i, si // 16, n, p, so // 16), lambda o, n: o.out_capacity(n),
                16, 16, np.complex128, np.complex128, warm=1)


def spec_qagc(qh):
    def make():
        a = qh.QuiskAgc(NCH, 48000)
        a.set_agc(-1, 80.0)
        return a
    return Spec("qh_qagc_process2", make, lambda o, i, si, p, so, n: o.process2_ptr(i, si // 16, p, so // 16, n),
                lambda o, n: n, 16, 16, np.complex128, np.complex128, warm=1)


def _pan_taps():
    k = np.arange(1023) - 511
    return np.sinc(k / 32.0) / 32.0 * np.blackman(1023)


def spec_pan(qh):
    def make():
        p = qh.Panadapter(NCH, 16384, 1024, 1536000.0)
        p.attach_fir(_pan_taps(), 32)
        return p
    return Spec("qh_pan_feed_decimate", make, lambda o, i, si, p, so, n: o.feed_decimate_ptr(i, si // 16, n, p, so // 16),
                lambda o, n: n // 32, 16, 16, np.complex128, np.complex128)


def _rxa(qh, nch, nc=0, at48=False, nbp=True, shift=True, modes=(1,)):
    e = qh.RxaEngine(nch, in_rate=48000) if at48 else qh.RxaEngine(nch)
    for c in range(nch):
        m = modes[c % len(modes)]
        e.SetRXAShiftRun(c, 1 if shift else 0); e.SetRXAShiftFreq(c, synth.shift_freq(c)); e.RXANBPSetRun(c, 1 if nbp else 0)
        e.SetRXAMode(c, m); e.SetRXAAGCMode(c, 0); e.SetRXAAGCFixed(c, 0.0)
        e.RXASetPassband(c, *((300.0, 3000.0) if m == 1 else (-4000.0, 4000.0) if m == 6 else (-8000.0, 8000.0)))
        if nc:
            e.RXASetNC(c, nc)
    return e


def spec_rxa_audio(qh):
    fmt = qh.AudioFormat("i16", volume=1.0, prescale=2147483647.0)
    return Spec("qh_rxa_process_audio", lambda: _rxa(qh, NCH),
                lambda o, i, si, p, so, n: o.process_audio_ptr(i, si // 16, p, so, n // 1024, fmt), lambda o, n: n // 4,
                16, 4, np.complex128, np.int16)


def spec_audio_pack(qh):
    fmt = qh.AudioFormat("i16", volume=1.0)

    def call(o, i, si, p, so, n):
        L = qh.load()
        rc = L.qh_audio_pack(0, None, i, si // 16, NCH, n, C.byref(fmt), p, so)
        if rc:
            raise qh.QuiskHipError("libquiskhip error %d: %s" % (rc, L.qh_last_error().decode(errors="replace")))
    return Spec("qh_audio_pack", lambda: None, call, lambda o, n: n, 16, 4, np.complex128, np.int16)


def _specs_refused(qh):
    out = []
    for dtype in (0, 1):
        for decim in (1, 2):
            out += [(spec_fir(qh, decim, dtype), n) for n in (97, 99, 20000)]            # P = 98: P - 1, P + 1, several tiles
        out += [(spec_rat(qh, "taps36", 2, 1, dtype), n) for n in (16, 18, 20000)]       # hist 17
        out += [(spec_rat(qh, "taps98", 2, 3, dtype), n) for n in (48, 50, 20000)]       # hist 48
        out += [(spec_hbc(qh, 3, dtype), n) for n in (40, 48, 24000)]
    out += [(spec_nb(qh), n) for n in (100, 20000)]
    out += [(spec_qrx(qh, 48000), n) for n in (480, 9600)]          # one step: the Rx filter reads the caller's rows and writes the caller's rows
    out += [(spec_qrx(qh, 192000), n) for n in (1920, 38400)]
    out += [(spec_qps(qh, 48000, 48000), 9600), (spec_qps(qh, 48000, 192000), 9600)]       # playback above the decimated rate: out grows 4x faster
    out += [(spec_qagc(qh), n) for n in (100, 4800)]
    out += [(spec_pan(qh), 16384 * 2)]
    out += [(spec_rxa_audio(qh), 1024 * 4), (spec_audio_pack(qh), 3000)]
    return out


def _ids(specs):
    return ["%s-%d-%d" % (s.name, i, n) for i, (s, n) in enumerate(specs)]


import quisk_amd as _qh_names      # noqa: E402  (the specs only hold constructors: nothing is loaded or run at collection)
_SPECS = _specs_refused(_qh_names)


def _inputs(spec, n, seed):
    x = noise(seed, NCH, n, spec.idt)
    if spec.name in ("qh_qps_process", "qh_rxa_process_audio"):
        x = np.stack([synth.make_mode_input_numpy("usb", c + seed, n) for c in range(NCH)]).astype(spec.idt) * (1.0 if spec.name == "qh_rxa_process_audio" else 2.0 ** 28)
    if spec.name == "qh_qagc_process2":
        x = x * 0.3
    if spec.name == "qh_audio_pack":
        x = x * 2.0 ** 29
    return x


def _legal(spec, obj, x, n):
    lout = spec.n_out(obj, n) * spec.uo
    return far_apart(lambda i, si, p, so: spec.call(obj, i, si, p, so, n), x, lout, spec.odt)


def _twins(spec, n):
    a, b = spec.make(), spec.make()
    for k in range(spec.warm + 1):                  # state that is not the initial one: delay lines, phases, an AGC past its first call
        xw = _inputs(spec, n, 100 + k)
        ya, yb = _legal(spec, a, xw, n), _legal(spec, b, xw, n)
        assert np.array_equal(ya, yb)
    return a, b


# (qh_qagc_process2 with d_src == d_dst and one stride is qh_qagc_process: test_qagc_in_place_is_qagc_process)
@pytest.mark.parametrize("idx,kind", [pytest.param(i, k, id="%s-%s" % (name, k)) for i, name in enumerate(_ids(_SPECS)) for k in REFUSED
                                      if not (_SPECS[i][0].name == "qh_qagc_process2" and k == "a_same")])
def test_overlapping_rows_are_refused(qh, idx, kind):
    """QH_ERR_INVALID with the entry point's name and "overlap", not a byte of the arena written, and the next two legal calls
    bit-identical to a twin that never saw the refused one (delay lines, phases, AGC state, the panadapter's count unmoved)."""
    spec, n = _SPECS[idx]
    obj, twin = _twins(spec, n)
    lin = n * spec.ui
    lout = spec.n_out(obj, n) * spec.uo
    total, i0, si, o0, so = layout(kind, NCH, lin, lout, spec.uo)
    ar = Arena(total)
    x = _inputs(spec, n, 7)
    ar.put(i0, si, x)
    before = ar.snapshot()
    try:
        spec.call(obj, ar.base + i0, si, ar.base + o0, so, n)
        torch.cuda.synchronize()
        got = ar.get(o0, so, lout, spec.odt, NCH)
        want = _legal(spec, _fresh_after_warm(spec, n), x, n)
        same = np.array_equal(got, want)
        pytest.fail("%s, layout %s: returned QH_OK [%s]" % (spec.name, kind, "output as the far-apart call's" if same else "WRONG OUTPUT"))
    except qh.QuiskHipError as err:
        msg = str(err)
        assert spec.name in msg and "overlap" in msg, msg
    torch.cuda.synchronize()
    assert torch.equal(ar.buf, before), "%s wrote into the arena of a refused call" % spec.name
    # no state moved: the next legal call continues bit-identically to a twin that never saw the refused call
    for k in range(2):
        xn = _inputs(spec, n, 30 + k)
        assert np.array_equal(_legal(spec, obj, xn, n), _legal(spec, twin, xn, n)), (spec.name, kind, k)


def _fresh_after_warm(spec, n):
    a, _ = _twins(spec, n)
    return a


@pytest.mark.parametrize("kind", ACCEPTED)
@pytest.mark.parametrize("idx", range(len(_SPECS)), ids=_ids(_SPECS))
def test_disjoint_rows_are_accepted(qh, idx, kind):
    """Interleaved rows, a matrix right behind the other's last row, rows that end exactly where the other's begin: three consecutive
    calls, bit-identical to the twin whose matrices lie apart."""
    spec, n = _SPECS[idx]
    obj, twin = _twins(spec, n)
    lin = n * spec.ui
    for k in range(3):
        lout = spec.n_out(obj, n) * spec.uo           # (a decimator's count moves with its phase)
        total, i0, si, o0, so = layout(kind, NCH, lin, lout, spec.uo)
        ar = Arena(total)
        x = _inputs(spec, n, 40 + k)
        ar.put(i0, si, x)
        torch.cuda.synchronize()
        spec.call(obj, ar.base + i0, si, ar.base + o0, so, n)
        got = ar.get(o0, so, lout, spec.odt, NCH)
        assert np.array_equal(got, _legal(spec, twin, x, n)), (spec.name, kind, k)     # (qps: rows out_capacity long, sentinel past the count)
        # the input rows are as they were
        assert np.array_equal(ar.get(i0, si, lin, spec.idt, NCH), x)


@pytest.mark.parametrize("kind", ["d_interleaved", "e_behind"])
@pytest.mark.parametrize("what", ["fir64", "fir32", "rat", "hbc"])
def test_disjoint_layouts_match_the_oracle(qh, oracle, what, kind):
    """The accepted layouts against the filter.c restatement at the parity tests' tolerances (1e-12 / 2e-5 relative RMS), three calls
    in a row (P - 1, P + 1, several tiles) so that the delay line crosses both of its paths."""
    dtype = 1 if what == "fir32" else 0
    if what.startswith("fir"):
        spec, refs = spec_fir(qh, 2, dtype), [oracle.OracleFir(_taps("taps98")) for _ in range(NCH)]
        step = lambda r, x: r.cDecimate(x, 2)                       # noqa: E731
        ns = (97, 99, 20000)
    elif what == "rat":
        spec, refs = spec_rat(qh, "taps98", 2, 3, 0), [oracle.OracleFir(_taps("taps98")) for _ in range(NCH)]
        step = lambda r, x: r.cInterpDecim(x, 2, 3)                 # noqa: E731
        ns = (48, 50, 20000)
    else:
        spec, refs = spec_hbc(qh, 3, 0), [[oracle.OracleHB45() for _ in range(3)] for _ in range(NCH)]

        def step(r, x):
            for s in r:
                x = s.cDecim2(x)
            return x
        ns = (40, 48, 24000)
    tol = 2e-5 if dtype == 1 else 1e-12
    obj = spec.make()
    got_all, want_all = [], []
    for k, n in enumerate(ns):
        lin, lout = n * spec.ui, spec.n_out(obj, n) * spec.uo
        total, i0, si, o0, so = layout(kind, NCH, lin, lout, spec.uo)
        ar = Arena(total)
        x = noise(60 + k, NCH, n)
        ar.put(i0, si, x.astype(spec.idt))
        torch.cuda.synchronize()
        spec.call(obj, ar.base + i0, si, ar.base + o0, so, n)
        got_all.append(ar.get(o0, so, lout, spec.odt, NCH))
        want_all.append(np.stack([step(refs[c], x.astype(spec.idt).astype(np.complex128)[c]) for c in range(NCH)]))
    got, want = np.concatenate(got_all, axis=1), np.concatenate(want_all, axis=1)
    assert got.shape == want.shape
    for c in range(NCH):
        assert rel_rms(got[c], want[c]) < tol, (what, kind, c)


def test_qagc_in_place_is_qagc_process(qh):
    """qh_qagc_process2 with d_src == d_dst and one stride is qh_qagc_process: bit for bit, call after call."""
    n = 4800
    a, b = qh.QuiskAgc(NCH, 48000), qh.QuiskAgc(NCH, 48000)
    for k in range(4):
        x = torch.from_numpy(noise(80 + k, NCH, n) * (0.3 + k)).to(DEV)
        xa, xb = x.clone(), x.clone()
        torch.cuda.synchronize()
        a.process_ptr(xa.data_ptr(), n, n)
        b.process2_ptr(xb.data_ptr(), n, xb.data_ptr(), n, n)
        torch.cuda.synchronize()
        assert torch.equal(xa, xb), k
    # the same buffer with another stride is an overlap like any other
    xs = torch.zeros((NCH, 2 * n), dtype=torch.complex128, device=DEV)
    torch.cuda.synchronize()
    with pytest.raises(qh.QuiskHipError, match="qh_qagc_process2.*overlap"):
        b.process2_ptr(xs.data_ptr(), 2 * n, xs.data_ptr(), n, n)


# ---- the packed sources: one buffer of src_bytes ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("where", ["one_sample_over", "touching", "far"])
@pytest.mark.parametrize("what", ["unpack_iq", "rxa_packed"])
def test_packed_source_and_output_rows(qh, what, where):
    """qh_unpack_iq and qh_rxa_process_packed measure the source in bytes: output rows that share one byte with its src_bytes are
    refused (nothing written, the engine's state unmoved); rows that end where it begins are accepted and equal the far-apart call.
    (Interleaving output rows with the channels' records is not a layout here: the source is declared as src_bytes in one piece.)"""
    nch, n = NCH, 1024 * 4
    fmt = qh.IqFormat.le24(gain=1.0 / 2 ** 31)
    chan_stride = n * 6
    src_bytes = nch * chan_stride
    rng = np.random.default_rng(5)
    raw = rng.integers(0, 256, src_bytes, dtype=np.uint8)
    if what == "unpack_iq":
        lout = n * 16
        make = lambda: None                                                     # noqa: E731

        def call(o, s, p, so):
            qh.ingest.unpack_ptr(s, src_bytes, fmt, nch, chan_stride, n, p, so // 16)
    else:
        lout = (n // 1024) * 256 * 16
        make = lambda: _rxa(qh, nch)                                            # noqa: E731

        def call(o, s, p, so):
            o.process_packed_ptr(s, src_bytes, fmt, chan_stride, p, so // 16, n // 1024)
    so = _up(lout)
    span = (nch - 1) * so + lout
    shift = {"one_sample_over": 16, "touching": 0, "far": -4096}[where]        # bytes of the source under the output's last sample
    o0 = GUARD + 4096
    s0 = o0 + span - shift
    total = max(s0 + src_bytes, o0 + span) + GUARD + 4096
    ar = Arena(total)
    ar.buf[s0:s0 + src_bytes].copy_(torch.from_numpy(raw))
    obj, twin = make(), make()
    # far-apart reference
    src = torch.from_numpy(raw).to(DEV)
    ref = torch.zeros((nch, so), dtype=torch.uint8, device=DEV)
    before = ar.snapshot()
    torch.cuda.synchronize()
    if where == "one_sample_over":
        with pytest.raises(qh.QuiskHipError) as ei:
            call(obj, ar.base + s0, ar.base + o0, so)
        assert ("qh_unpack_iq" if what == "unpack_iq" else "qh_rxa_process_packed") in str(ei.value) and "overlap" in str(ei.value)
        torch.cuda.synchronize()
        assert torch.equal(ar.buf, before)
    else:
        call(obj, ar.base + s0, ar.base + o0, so)
        torch.cuda.synchronize()
        assert torch.equal(ar.buf[s0:s0 + src_bytes].cpu(), torch.from_numpy(raw))
    call(twin, src.data_ptr(), ref.data_ptr(), so)
    torch.cuda.synchronize()
    want = ref.cpu().numpy()[:, :lout].copy().view(np.complex128)
    if where != "one_sample_over":
        assert np.array_equal(ar.get(o0, so, lout, np.complex128, nch), want)
    elif obj is not None:           # no state moved: the engine's first accepted call is its twin's first call
        y1 = torch.zeros_like(ref)
        torch.cuda.synchronize()
        call(obj, src.data_ptr(), y1.data_ptr(), so)
        torch.cuda.synchronize()
        assert torch.equal(y1[:, :lout], ref[:, :lout])


def test_udp17_buffers_may_not_overlap(qh):
    """qh_unpack_udp17: the source and each of the five outputs, and every pair of outputs, share no byte -- else QH_ERR_INVALID and
    nothing written; laid end to end without a gap they are accepted and equal the call with buffers of their own."""
    import quisk_amd
    L = quisk_amd.load()
    npk, pb = 4, 1442
    nrec = npk * ((pb - 2) // 6)
    rng = np.random.default_rng(17)
    raw = rng.integers(0, 256, npk * pb, dtype=np.uint8)
    sizes = [npk * pb, nrec * 16, nrec * 16, nrec * 4, 32, 16]           # source, ch0, ch1, marks, counts, dc_sum

    def run(ptrs):
        rc = L.qh_unpack_udp17(0, None, ptrs[0], npk, pb, 1.0, 0, 0.0, 0.0, ptrs[1], ptrs[2], ptrs[3], ptrs[4], ptrs[5])
        return rc, L.qh_last_error().decode(errors="replace")

    def pack(offs):
        total = max(o + s for o, s in zip(offs, sizes)) + GUARD
        ar = Arena(total)
        ar.buf[offs[0]:offs[0] + sizes[0]].copy_(torch.from_numpy(raw))
        return ar
    # end to end, 16-byte aligned: accepted
    offs, o = [], GUARD
    for s in sizes:
        offs.append(o)
        o += _up(s)
    ar = pack(offs)
    torch.cuda.synchronize()
    rc, msg = run([ar.base + x for x in offs])
    assert rc == 0, msg
    torch.cuda.synchronize()
    sep = [torch.zeros(_up(s), dtype=torch.uint8, device=DEV) for s in sizes]
    sep[0][:sizes[0]].copy_(torch.from_numpy(raw))
    torch.cuda.synchronize()
    rc, msg = run([t.data_ptr() for t in sep])
    assert rc == 0, msg
    torch.cuda.synchronize()
    counts = sep[4].cpu().numpy().view(np.int64)
    assert counts[0] + counts[1] == nrec
    lens = [sizes[0], int(counts[0]) * 16, int(counts[1]) * 16, int(counts[2]) * 4, 32, 16]
    for j in range(1, 6):
        assert torch.equal(ar.buf[offs[j]:offs[j] + lens[j]].cpu(), sep[j][:lens[j]].cpu()), j
    # each pair made to share the last 16 bytes of the earlier buffer (the later one moved back): refused, the arena untouched
    for i in range(6):
        for j in range(i + 1, 6):
            o2 = list(offs)
            o2[j] = offs[i] + _up(sizes[i]) - 16
            assert o2[j] >= offs[i]
            # keep the remaining buffers clear of the pair and of each other
            top = max(o2[i] + sizes[i], o2[j] + sizes[j])
            for k in range(6):
                if k not in (i, j):
                    o2[k] = _up(top) + 16 * 64 * k + sum(_up(s) for s in sizes[:k])
            ar2 = pack(o2)
            before = ar2.snapshot()
            rc, msg = run([ar2.base + x for x in o2])
            assert rc != 0 and "qh_unpack_udp17" in msg and "overlap" in msg, (i, j, rc, msg)
            torch.cuda.synchronize()
            assert torch.equal(ar2.buf, before), (i, j)


# ---- qh_rxa_process: overlap allowed ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shift", ["k1", "k255", "kn_out", "interleaved"])
@pytest.mark.parametrize("chain", ["front_only", "front_nbp", "band48k_nc2048", "band48k_nc16384", "mixed"])
def test_rxa_partial_overlaps(qh, chain, shift):
    """include/quiskhip.h, qh_rxa_process: output rows may lie over the input rows.  out = in + k samples (k = 1, 255, n_out) with the
    input's stride, and rows interleaved: within 1e-11 of the twin whose matrices lie apart, call after call."""
    nch, ncall = 4, 3
    at48 = chain.startswith("band48k")
    nc = 16384 if chain.endswith("16384") else 2048 if at48 else 0
    nb = 40 if nc == 16384 else 20          # (a call longer than the 16384-tap filter's delay: every call's output has signal in it)
    n_in, n_out = (nb * 256, nb * 256) if at48 else (nb * 1024, nb * 256)
    modes = (1, 6, 5) if chain == "mixed" else (1,)
    kinds = {1: "usb", 6: "am", 5: "fm"}

    def make():
        return _rxa(qh, nch, nc=nc, at48=at48, nbp=chain != "front_only", shift=not at48, modes=modes)
    ea, eb = make(), make()
    k = {"k1": 1, "k255": 255, "kn_out": n_out, "interleaved": None}[shift]
    if k is None:
        stride = 2 * n_in
        total = nch * stride
        i_off, o_off = 0, n_in
    else:
        stride = n_in
        total = nch * stride + k
        i_off, o_off = 0, k
    arena = torch.zeros(total + 64, dtype=torch.complex128, device=DEV)
    y = torch.empty((nch, n_out), dtype=torch.complex128, device=DEV)
    for call in range(ncall):
        xh = np.stack([synth.make_mode_input_numpy(kinds[modes[c % len(modes)]], c + 20 * call, n_in) for c in range(nch)])
        x = torch.from_numpy(xh).to(DEV)
        xin = arena[i_off:i_off + nch * stride].view(nch, stride)[:, :n_in]
        xin.copy_(x)
        torch.cuda.synchronize()
        ea.process_ptr(x.data_ptr(), n_in, y.data_ptr(), n_out, nb)
        ea.synchronize()
        eb.process_ptr(arena.data_ptr() + 16 * i_off, stride, arena.data_ptr() + 16 * o_off, stride, nb)
        eb.synchronize()
        got = torch.stack([arena[o_off + c * stride:o_off + c * stride + n_out] for c in range(nch)])
        scale = float(y.abs().max().item())
        assert scale > 1e-3
        assert float((got - y).abs().max().item()) <= 1e-11 * scale, (chain, shift, call)
    ea.close(); eb.close()


# ---- the *_host forms: h_out == h_in works like the reference's in-place primitives --------------------------------------------------
@pytest.mark.parametrize("what", ["fir", "hbc", "rat", "nb", "qrx", "qps", "rxa"])
def test_host_forms_take_h_out_equal_h_in(qh, what):
    import quisk_amd
    L = quisk_amd.load()
    nch = NCH
    if what == "fir":
        mk, n = (lambda: qh.FirBank(nch, _taps("taps98"), 2)), 5000
        run = lambda o, p, s, n_: L.qh_fir_process_host(o._h, p, s, n_, p, s, C.byref(C.c_int(0)))               # noqa: E731
    elif what == "hbc":
        mk, n = (lambda: qh.HalfBandCascade(nch, 3)), 4096
        run = lambda o, p, s, n_: L.qh_hbc_process_host(o._h, p, s, n_, p, s)                                    # noqa: E731
    elif what == "rat":
        mk, n = (lambda: qh.RationalFir(nch, _taps("taps36"), 2)), 3000
        run = lambda o, p, s, n_: L.qh_rat_process_host(o._h, p, s, n_, p, s, C.byref(C.c_int(0)))               # noqa: E731
    elif what == "nb":
        mk, n = (lambda: qh.NoiseBlanker(nch, 192000, 2)), 6000
        run = lambda o, p, s, n_: L.qh_nb_process_host(o._h, p, s, p, s, n_)                                     # noqa: E731
    elif what == "qrx":
        mk, n = (lambda: qh.QuiskRxBank(nch, 192000, 3)), 19200
        run = lambda o, p, s, n_: L.qh_qrx_process_host(o._h, p, s, n_, p, s, C.byref(C.c_int(0)))               # noqa: E731
    elif what == "qps":
        mk, n = (lambda: qh.QuiskProcessBank(nch, 48000, 3, 2700, playback_rate=96000)), 4800
        run = lambda o, p, s, n_: L.qh_qps_process_host(o._h, p, s, n_, p, s, C.byref(C.c_int(0)))               # noqa: E731
    else:
        mk, n = (lambda: _rxa(qh, nch)), 1024 * 6
        run = lambda o, p, s, n_: L.qh_rxa_process_host(o._h, p, s, p, s, n_ // 1024)                           # noqa: E731
    a, b = mk(), mk()
    for k in range(3):
        x = np.stack([synth.make_mode_input_numpy("usb", c + 9 * k, n) for c in range(nch)]) * (2.0 ** 28 if what in ("qrx", "qps") else 1.0)
        want = b.process_host(x)
        stride = max(n, want.shape[1], a.out_capacity(n) if what == "qps" else 0)
        buf = np.zeros((nch, stride), dtype=np.complex128)
        buf[:, :n] = x
        assert run(a, buf.ctypes.data, stride, n) == 0, L.qh_last_error()
        assert np.array_equal(buf[:, :want.shape[1]], want), (what, k)
