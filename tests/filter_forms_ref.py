"""Plain float64 references, per-sample error bounds and the shared case material for the three stand-alone filter banks
(FirBank, RationalFir, HalfBandCascade).  numpy only; the references are direct sums, no transform.

Bounds are per output sample and per part (real, imaginary).  Where a function returns a bound or a scale for both parts it comes
packed in one complex array: `.real` belongs to the real part of the output, `.imag` to the imaginary part.

    RationalFir       |got - want| <= (K + 4) u S[m]          direct sums of K products in T, taps rounded to T, one multiply by U
    HalfBandCascade   |got - want| <= B_nstage[m]             B_0 = 0,  B_s = |h| (*)v2 B_(s-1) + 26 u (|h| (*)v2 |x_(s-1)|)
    FirBank, fp32     |got - want| <= 16 E                    E = the largest per-sample error of os_model in complex64 for the case
    FirBank, fp64     |got - want| <= TOL64 rms(want)

u = 2^-24 (fp32) or 2^-53 (fp64).  os_model is no reference for values: it is an overlap-save filter on 4096-point tiles in the bank's
own precision, and its error against the direct sum is the rounding scale of a transform-domain filter in that precision.  The margin of
16 covers what the kernel does differently from numpy's transform: radix order, float twiddle tables, and `fold` products summed ahead
of the inverse transform.
"""
import functools

import numpy as np

U32, U64 = 2.0 ** -24, 2.0 ** -53
TOL64, TOL32 = 1e-12, 2e-5          # the project's stream tolerances (tests/test_gpu_fir_parity.py), here held per sample
NFFT = 4096                         # qh_stage.hpp kStageNfft
NT = 256                            # lanes of a workgroup: one polyphase block is NT outputs
SPLITS = [0, 1, 7, 333, 2, 64, 1000, 5, 0, 588]
F64, F32 = 0, 1


def unit(dtype):
    return U64 if dtype == F64 else U32


def ctype(dtype):
    return np.complex128 if dtype == F64 else np.complex64


def rms(v):
    v = np.asarray(v)
    return float(np.sqrt(np.mean(np.abs(v) ** 2))) if v.size else 0.0


# ---------------------------------------------------------------------------------------------------------------------------
# references
# ---------------------------------------------------------------------------------------------------------------------------
def _with_history(x, nh, hist):
    """x [..., n] behind its nh preceding samples (zeros, or the last nh of `hist`), in float64 parts."""
    x = np.asarray(x)
    x = x.astype(np.complex128)                         # exact for complex64 values
    pre = np.zeros(x.shape[:-1] + (nh,), dtype=np.complex128)
    if hist is not None and nh > 0:
        h = np.asarray(hist).astype(np.complex128)
        assert h.shape[-1] >= nh, "history shorter than the filter's memory"
        pre[...] = h[..., h.shape[-1] - nh:]
    return np.concatenate([pre, x], axis=-1)


def fir_decimate(x, taps, d, phase0=0, hist=None):
    """y[m] = sum_k h[k] x[d m + (d - 1 - phase0) - k] by direct sums in float64, m < (phase0 + n) // d, over the last axis of x.
    `hist` holds the samples ahead of x[0] (the last ntaps - 1 are used; zeros when None).  Taps may be complex.
    Returns (y, A) with A[m] = sum_k |h[k]| |x[...]| per part (packed, see the module's head)."""
    taps = np.asarray(taps)
    nt = taps.size
    hr = np.ascontiguousarray(taps.real, dtype=np.float64)
    hi = np.ascontiguousarray(taps.imag, dtype=np.float64) if np.iscomplexobj(taps) else np.zeros(nt)
    xp = _with_history(x, nt - 1, hist)
    n = xp.shape[-1] - (nt - 1)
    nout = (phase0 + n) // d
    shape = xp.shape[:-1] + (nout,)
    yr, yi, ar, ai = (np.zeros(shape) for _ in range(4))
    if nout == 0:
        return yr + 1j * yi, ar + 1j * ai
    xr, xi = np.ascontiguousarray(xp.real), np.ascontiguousarray(xp.imag)
    axr, axi = np.abs(xr), np.abs(xi)
    first = d - 1 - phase0 + nt - 1                     # position in xp of x[d 0 + (d - 1 - phase0) - 0]
    for k in range(nt):
        a, b = hr[k], hi[k]
        if a == 0.0 and b == 0.0:
            continue
        s = slice(first - k, first - k + d * (nout - 1) + 1, d)
        yr += a * xr[..., s]
        yi += a * xi[..., s]
        ar += abs(a) * axr[..., s]
        ai += abs(a) * axi[..., s]
        if b != 0.0:
            yr -= b * xi[..., s]
            yi += b * xr[..., s]
            ar += abs(b) * axi[..., s]
            ai += abs(b) * axr[..., s]
    return yr + 1j * yi, ar + 1j * ai


def rational_count(n, U, D, phase0):
    """Outputs of a call of n samples and the phase it leaves (qh_polyphase.hip count_for, qh_rat_process)."""
    span = n * U
    m = 0 if phase0 >= span else (span - phase0 + D - 1) // D
    return m, phase0 + m * D - span


def rational(x, taps, U, D, phase0=0, hist=None):
    """The formula at the head of qh_polyphase.hip: with p = phase0 + m D, i = p // U, ph = p % U and K = ceil(ntaps / U),
    y[m] = U sum_{k < K} taps[ph + k U] x[i - k] (taps beyond ntaps are zero), by direct sums in float64 over the last axis.
    Returns (y, S) with S[m] = U sum_k |taps[ph + k U]| |x[i - k]| per part (packed)."""
    taps = np.asarray(taps, dtype=np.float64)
    K = (taps.size + U - 1) // U
    c = np.zeros(U * K)
    c[:taps.size] = taps
    xp = _with_history(x, K - 1, hist)
    n = xp.shape[-1] - (K - 1)
    nout, _ = rational_count(n, U, D, phase0)
    p = phase0 + D * np.arange(nout, dtype=np.int64)
    i, ph = p // U, p % U
    shape = xp.shape[:-1] + (nout,)
    yr, yi, sr, si = (np.zeros(shape) for _ in range(4))
    xr, xi = np.ascontiguousarray(xp.real), np.ascontiguousarray(xp.imag)
    for k in range(K):
        ck = c[ph + k * U]
        idx = i - k + (K - 1)
        vr, vi = xr[..., idx], xi[..., idx]
        yr += ck * vr
        yi += ck * vi
        sr += np.abs(ck) * np.abs(vr)
        si += np.abs(ck) * np.abs(vi)
    return U * (yr + 1j * yi), U * (sr + 1j * si)


def hb45_taps():
    """The 43 taps at delays 0 .. 42 of Quisk's 45-tap half-band (filter.c:382-385; the library's qh_hb45_taps, restated so that the
    CPU tests need no GPU library)."""
    coef = [0.000018566625444266, -0.000118469698701817, 0.000457318798253456, -0.001347840471412094, 0.003321838571445455,
            -0.007198422696929033, 0.014211106939802483, -0.026424776824073383, 0.048414810444971007, -0.096214669073304823,
            0.314881034738348550]
    t = np.zeros(43)
    for i, v in enumerate(coef):
        t[2 * i] = t[42 - 2 * i] = v
    t[21] = 0.5
    return t


HB_OPS = 26                         # the 24 products and sums of a half-band output, plus 2


def hb45_chain(x, nstage, u):
    """`nstage` half-band decimators in a row over the last axis of x.  Returns (y, B): B bounds, per part (packed), the error of the
    same chain evaluated with unit roundoff u:  B_0 = 0,  B_s = |h| (*)v2 B_(s-1) + 26 u (|h| (*)v2 |x_(s-1)|)."""
    h = hb45_taps()
    y = np.asarray(x).astype(np.complex128)
    B = np.zeros(y.shape, dtype=np.complex128)
    for _ in range(nstage):
        y, A = fir_decimate(y, h, 2)
        carried, _ = fir_decimate(B, np.abs(h), 2)
        B = carried + HB_OPS * u * A
    return y, B


def os_model(x, taps, d, dtype, phase0=0):
    """Overlap-save on 4096-point tiles with np.fft in the bank's own precision (1-D x, zero history), every d-th sample kept.  The mask is
    formed in float64 and rounded to the type.  Not a reference for values: see the module's head."""
    ct = ctype(dtype)
    taps = np.asarray(taps)
    nt = taps.size
    L = NFFT - (nt - 1)
    assert L >= 1
    hp = np.zeros(NFFT, dtype=np.complex128)
    hp[:nt] = taps
    mask = np.fft.fft(hp).astype(ct)
    x = np.asarray(x).astype(ct)
    n = x.size
    ntiles = (n + L - 1) // L
    xp = np.concatenate([np.zeros(nt - 1, dtype=ct), x, np.zeros(ntiles * L - n, dtype=ct)])
    full = np.empty(ntiles * L, dtype=ct)
    off = np.arange(NFFT)
    for t0 in range(0, ntiles, 256):
        t1 = min(t0 + 256, ntiles)
        tiles = xp[(np.arange(t0, t1) * L)[:, None] + off[None, :]]
        X = np.fft.fft(tiles, axis=-1)
        assert X.dtype == ct, "np.fft must stay in the bank's precision (numpy >= 2.0)"
        Y = np.fft.ifft(X * mask[None, :], axis=-1)
        assert Y.dtype == ct
        full[t0 * L:t1 * L] = Y[:, nt - 1:].reshape(-1)
    nout = (phase0 + n) // d
    return full[d - 1 - phase0:n:d][:nout]


# ---------------------------------------------------------------------------------------------------------------------------
# the worst sample of a comparison and where it sits
# ---------------------------------------------------------------------------------------------------------------------------
def _nearest(marks, idx):
    marks = np.asarray(marks, dtype=np.int64)
    if marks.size == 0:
        return None
    return int(np.min(np.abs(marks - idx)))


def worst_sample(got, want, bound, seams=(), calls=()):
    """got, want [nch, n]; bound: a scalar, or [nch, n] packed per part.  seams / calls: output indices where a tile (segment, block)
    and a call start.  Returns the sample with the largest error over bound."""
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape, (got.shape, want.shape)
    if got.size == 0:
        return {"ratio": 0.0, "channel": 0, "index": 0, "err": 0.0, "bound": 0.0, "to_seam": None, "to_call": None}
    g = got.astype(np.complex128)
    err = np.stack([np.abs(g.real - want.real), np.abs(g.imag - want.imag)])
    if np.ndim(bound) == 0:
        bnd = np.full(err.shape, float(bound))
    else:
        bound = np.asarray(bound)
        bnd = np.stack([bound.real, bound.imag]) if np.iscomplexobj(bound) else np.stack([bound, bound])
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = np.where(err == 0.0, 0.0, err / bnd)            # a zero bound allows only an exact result
    ratio = np.where(np.isfinite(g.real) & np.isfinite(g.imag), ratio, np.inf)
    part, ch, idx = np.unravel_index(int(np.argmax(ratio)), ratio.shape)
    return {"ratio": float(ratio[part, ch, idx]), "channel": int(ch), "index": int(idx), "part": "re" if part == 0 else "im",
            "err": float(err[part, ch, idx]), "bound": float(bnd[part, ch, idx]),
            "to_seam": _nearest(seams, idx), "to_call": _nearest(calls, idx)}


def assert_inside(name, got, want, bound, seams=(), calls=()):
    w = worst_sample(got, want, bound, seams, calls)
    assert w["ratio"] <= 1.0, (
        "%s: channel %d sample %d (%s): error %.3e over bound %.3e = %.3g; %s samples from the nearest tile/segment start, "
        "%s from the nearest call boundary" % (name, w["channel"], w["index"], w["part"], w["err"], w["bound"], w["ratio"],
                                                w["to_seam"], w["to_call"]))
    return w


def run_calls(bank, x, sizes, after=None):
    """Feed x [nch, n] to bank.process_host in calls of `sizes` samples.  Returns (y, starts): the outputs in one row per channel and the
    output index at which every call starts.  `after(call_index, out)` runs behind every call."""
    out, starts, pos, m = [], [], 0, 0
    for j, k in enumerate(sizes):
        y = bank.process_host(x[:, pos:pos + k])
        starts.append(m)
        out.append(y)
        pos += k
        m += y.shape[1]
        if after is not None:
            after(j, y)
    assert pos == x.shape[1], "the call sizes must use up the stream"
    return np.concatenate(out, axis=1), starts


# ---------------------------------------------------------------------------------------------------------------------------
# FirBank: geometry as Stage::init computes it, taps, inputs, call pattern, and the case record
# ---------------------------------------------------------------------------------------------------------------------------
def stage_geometry(ntaps, d):
    """(fold, pick, P, Lf, per_tile) as qh_stage.hpp Stage::init: P history samples, Lf folded outputs and per_tile final outputs a tile."""
    fold = 8 if d % 8 == 0 else 4 if d % 4 == 0 else 2 if d % 2 == 0 else 1
    pick = d // fold
    P = max(fold, (ntaps - 1 + fold - 1) // fold * fold)
    Lf = ((NFFT - P) // fold) // pick * pick
    return fold, pick, P, Lf, Lf // pick


def forced_taps(ntaps, seed, complex_taps=False):
    """Taps without a window: seeded normal values scaled by 1 / sqrt(ntaps) so that fp32 sums stay near unit size, the first and the
    last tap forced to +-1 -- a tile, a history row or a copy that is one sample off changes an output by the size of a sample."""
    rng = np.random.default_rng(seed)
    h = rng.standard_normal(ntaps) / np.sqrt(ntaps)
    if complex_taps:
        h = h + 1j * rng.standard_normal(ntaps) / np.sqrt(ntaps)
    h[0] = 1.0
    h[-1] = -1.0
    return h


def make_input(kind, nch, n, seed, dtype):
    """'noise': complex Gaussian; 'impulses': unit impulses every 977 samples on zeros, another offset and turn per channel.  In fp32 the
    values are complex64, and the references read exactly those."""
    if kind == "noise":
        rng = np.random.default_rng(seed)
        x = rng.standard_normal((nch, n)) + 1j * rng.standard_normal((nch, n))
    else:
        x = np.zeros((nch, n), dtype=np.complex128)
        for c in range(nch):
            pos = np.arange(7 + 13 * c, n, 977)
            x[c, pos] = 1j ** ((np.arange(pos.size) + c) % 4)
    return x.astype(ctype(dtype))


def fir_call_sizes(ntaps, d, short=False):
    """Calls that produce per_tile - 1, per_tile, per_tile + 1 and 2 per_tile + 1 outputs (each leaving another phase); calls of P - 1, P
    and P + 1 samples, either side of the switch between the kernel's own hist_next copy and hist_update_kernel; three single samples in a
    row; an empty call; one long remainder.  About 20 000 samples; `short`: about 600 beside the three calls of one delay line."""
    fold, pick, P, Lf, per_tile = stage_geometry(ntaps, d)
    sizes, phase = [], 0

    def add(n):
        nonlocal phase
        sizes.append(n)
        phase = (phase + n) % d

    for j, q in enumerate((per_tile - 1, per_tile, per_tile + 1, 2 * per_tile + 1)):
        add(max(q * d - phase + j % d, 0))              # (phase + n) // d == q
    for n in (P - 1, P, P + 1, 1, 1, 1, 0):
        add(n)
    target = sum(sizes) + 600 if short else 20000
    add(max(target - sum(sizes), (3 * d * per_tile + 7) if not short else 600))
    return sizes


def fir_seams(ntaps, d, sizes):
    """Output indices at which a call and a tile start, for the failure message."""
    per_tile = stage_geometry(ntaps, d)[4]
    calls, tiles, phase, m = [], [], 0, 0
    for n in sizes:
        k = (phase + n) // d
        calls.append(m)
        tiles.extend(range(m, m + k, per_tile))
        m += k
        phase = (phase + n) % d
    return np.array(calls), np.array(tiles)


def fir_case_id(case):
    ntaps, d, cplx = case
    return "%dtaps_d%d%s" % (ntaps, d, "_ctaps" if cplx else "")


@functools.lru_cache(maxsize=4)
def fir_case(case, kind, dtype, nch=3):
    """Everything a FirBank case needs, computed once: taps, input, call sizes, the float64 reference and, in fp32, E -- the largest
    per-sample error of os_model in complex64 against the reference on channel 0's stream (one channel keeps it quick; a maximum over
    fewer samples is smaller, never larger)."""
    ntaps, d, cplx = case
    fold, pick, P, Lf, per_tile = stage_geometry(ntaps, d)
    short = Lf <= 2                                             # the two extremes: a tile per output or two
    taps = forced_taps(ntaps, 1000 * ntaps + d, cplx)
    sizes = fir_call_sizes(ntaps, d, short)
    x = make_input(kind, nch, sum(sizes), 77 * ntaps + d, dtype)
    want, _ = fir_decimate(x, taps, d)
    r = rms(want)
    assert r > 0.0
    rec = {"taps": taps, "x": x, "sizes": sizes, "want": want, "rms": r, "geometry": (fold, pick, P, Lf, per_tile)}
    rec["calls"], rec["tiles"] = fir_seams(ntaps, d, sizes)
    if dtype == F32:
        model = os_model(x[0], taps, d, F32)
        rec["E"] = float(np.max(np.maximum(np.abs(model.real - want[0].real), np.abs(model.imag - want[0].imag))))
        rec["bound"] = 16.0 * rec["E"]
    else:
        rec["bound"] = TOL64 * r
    return rec


# ---------------------------------------------------------------------------------------------------------------------------
# RationalFir
# ---------------------------------------------------------------------------------------------------------------------------
def rat_case_id(case):
    U, D, ntaps = case
    return "%d_over_%d_%dtaps" % (U, D, ntaps)


def rat_call_sizes(U, D, ntaps):
    """The SPLITS pattern, calls shorter than the K - 1 samples of memory, and (for ratios that decimate by more than 3) runs of one-sample
    calls that produce nothing, so that the phase stays beyond a call's span over several calls."""
    K = (ntaps + U - 1) // U
    sizes = list(SPLITS) + [max(K - 2, 0), 1, max(K // 2, 0), K - 1 + 3]
    if D > 3 * U:
        sizes += [1] * (2 * ((D + U - 1) // U) + 3) + [2, 1, 1, 1]
    sizes += [K, 411]
    return sizes


def rat_calls(U, D, sizes):
    """Per call (outputs, phase left), and the output index at which every call starts."""
    phase, m, counts, starts = 0, 0, [], []
    for n in sizes:
        k, phase = rational_count(n, U, D, phase) if n > 0 else (0, phase)
        starts.append(m)
        counts.append((k, phase))
        m += k
    return counts, np.array(starts)


@functools.lru_cache(maxsize=4)
def rat_case(case, dtype, nch=3):
    U, D, ntaps = case
    K = (ntaps + U - 1) // U
    taps = forced_taps(ntaps, 31 * ntaps + 7 * U + D)
    sizes = rat_call_sizes(U, D, ntaps)
    x = make_input("noise", nch, sum(sizes), 5 * ntaps + U, dtype)
    want, S = rational(x, taps, U, D)
    counts, starts = rat_calls(U, D, sizes)
    assert sum(k for k, _ in counts) == want.shape[1]
    blocks = np.concatenate([np.arange(s, s + k, NT) for s, (k, _) in zip(starts, counts)] + [np.zeros(0, dtype=np.int64)])
    return {"taps": taps, "x": x, "sizes": sizes, "want": want, "K": K, "bound": (K + 4) * unit(dtype) * S, "counts": counts,
            "calls": starts, "blocks": blocks}


def polyphase_emulated(x, taps, U, D, T=np.float32):
    """The kernel's arithmetic on the CPU in type T: taps rounded to T, K products accumulated in order, one multiply by U."""
    CT = np.complex64 if T == np.float32 else np.complex128
    taps = np.asarray(taps, dtype=np.float64)
    K = (taps.size + U - 1) // U
    c = np.zeros(U * K, dtype=T)
    c[:taps.size] = taps.astype(T)
    x = np.asarray(x).astype(CT)
    xp = np.concatenate([np.zeros(x.shape[:-1] + (K - 1,), dtype=CT), x], axis=-1)
    nout, _ = rational_count(x.shape[-1], U, D, 0)
    p = D * np.arange(nout, dtype=np.int64)
    i, ph = p // U, p % U
    ar = np.zeros(x.shape[:-1] + (nout,), dtype=T)
    ai = np.zeros_like(ar)
    for k in range(K):
        ck = c[ph + k * U]
        v = xp[..., i - k + (K - 1)]
        ar = ar + v.real * ck
        ai = ai + v.imag * ck
    g = T(U)
    return (ar * g) + 1j * (ai * g)


# ---------------------------------------------------------------------------------------------------------------------------
# HalfBandCascade
# ---------------------------------------------------------------------------------------------------------------------------
def hbc_head(nstage):
    """Stages of a cascade's first launch (qh_hbcascade.hip: six and more stages run as 4 + the rest)."""
    return 4 if nstage >= 6 else nstage


def hbc_warm(nstage):
    """Input samples of history a launch keeps (qh_hbcascade.hip warm_of)."""
    return (42 * ((1 << hbc_head(nstage)) - 1) + 4095) // 4096 * 4096


def hbc_segment(nch, n_in, nstage):
    """Input samples per segment of the first launch, as qh_hbcascade.hip launch() picks them (2048-sample steps)."""
    step = 2048
    warm = (42 * ((1 << hbc_head(nstage)) - 1) + step - 1) // step * step     # HbGeom::WARM: the warm-up of a segment, whole steps
    seg = 64 * step
    while seg > 16 * step and nch * ((n_in + seg - 1) // seg) < 1024:
        seg >>= 1
    while seg > 4 * step and seg > 4 * warm and nch * ((n_in + seg - 1) // seg) < 512:
        seg >>= 1
    return seg


def hbc_seams(nch, sizes, nstage):
    calls, segs, m = [], [], 0
    for n in sizes:
        calls.append(m)
        if n > 0:
            seg = hbc_segment(nch, n, nstage)
            segs.extend(m + (s >> nstage) for s in range(0, n, seg))
        m += n >> nstage
    return np.array(calls), np.array(segs)


def hbc_ragged_sizes(nstage):
    """Ragged multiples of 2^nstage around the launch's history length (tests/test_gpu_hbcascade_parity.py
    test_calls_around_one_history_long)."""
    d, W = 1 << nstage, hbc_warm(nstage)
    return [W - d, W, d, W + d, 3 * d, W, W - d, 2 * W + 5 * d, d, W // 16 // d * d + d, W, 4 * W, W - d, W + d]


@functools.lru_cache(maxsize=4)
def hbc_case(nstage, dtype, ragged):
    if ragged:
        nch, sizes = 2, hbc_ragged_sizes(nstage)
    else:
        nch, sizes = 1, [5 * 8192 + 3 * (1 << nstage)]
    x = make_input("noise", nch, sum(sizes), 900 + 10 * nstage + (1 if ragged else 0), dtype)
    want, B = hb45_chain(x, nstage, unit(dtype))
    calls, segs = hbc_seams(nch, sizes, nstage)
    return {"x": x, "sizes": sizes, "want": want, "B": B, "rms": rms(want), "calls": calls, "segs": segs, "nch": nch}
