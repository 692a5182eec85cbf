"""The two 16-point butterflies of quisk_amd/csrc/qh_fft.hpp restated in numpy, operation by operation and in the kernels' order, and
an exact 16-point DFT in long double to hold them against.  numpy only.

    dft16_radix2   Dft<16, INV, double2>: the radix-2 decimation-in-frequency recursion with mul_wconst's literals.  Sums and
                   products round one by one, except the two FMAs of a full complex product (cmul), which the compiler contracts.
    dft16_lean     Dft16Lean<INV, double2>: two radix-4 layers, the eight constants W_16^m (m = 1, 2, 2, 3, 3, 6, 6, 9) as
                   s (1 + i t) with the scale s carried in the second layer's FMAs; 144 operations.

Both take x [..., 16] complex128 in natural order and return natural order; inv = True is the unnormalised inverse (conjugate
constants).  An FMA is one rounding: math.fma where Python has it (3.13), else the product and the sum in long double (64-bit
significand), rounded once to float64 -- the product of two float64 values carries 106 bits, so that form can differ from a true FMA
in the last place in rare cases; it is a model of the rounding ORDER, which is what the two forms differ in.

`fault` plants one error in dft16_lean for the tests: "constant" (tan(pi/8) with its 14th digit wrong) or "sign" (the imaginary part
of the m = 3 rotation with the wrong sign)."""
import math

import numpy as np

LD, CLD = np.longdouble, np.clongdouble
C1 = 0.92387953251128675613         # cos(pi/8)
C2 = 0.70710678118654752440         # cos(pi/4)
T1 = 0.41421356237309504880         # tan(pi/8)
COS32 = [1.0, 0.98078528040323044913, 0.92387953251128675613, 0.83146961230254523708, 0.70710678118654752440,
         0.55557023301960222474, 0.38268343236508977173, 0.19509032201612826785, 0.0]       # qh_fft.hpp cos32


def fma(a, b, c):
    a, b, c = np.broadcast_arrays(np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64), np.asarray(c, dtype=np.float64))
    if hasattr(math, "fma"):
        return np.array([math.fma(p, q, r) for p, q, r in zip(a.ravel(), b.ravel(), c.ravel())], dtype=np.float64).reshape(a.shape)
    return (a.astype(LD) * b.astype(LD) + c.astype(LD)).astype(np.float64)


# ---- complex values as (re, im) pairs of float64 arrays -------------------------------------------------------------------
def cadd(a, b):
    return (a[0] + b[0], a[1] + b[1])


def csub(a, b):
    return (a[0] - b[0], a[1] - b[1])


def mul_mi(a, inv):
    """a (-i) forward, a (+i) inverse: no arithmetic."""
    return (-a[1], a[0]) if inv else (a[1], -a[0])


def cmul(a, w):
    """qh_fft.hpp cmul under the compiler's contraction: one product, one FMA per part."""
    return (fma(a[0], w[0], -(a[1] * w[1])), fma(a[0], w[1], a[1] * w[0]))


# ---- Dft<16>: radix 2 -----------------------------------------------------------------------------------------------------
def mul_wconst(R, I, inv, a):
    A = I * (32 // R)
    if A == 0:
        return a
    if A == 8:
        return mul_mi(a, inv)
    s = 0.70710678118654752440
    if A == 4:
        return ((a[0] - a[1]) * s, (a[0] + a[1]) * s) if inv else ((a[0] + a[1]) * s, (a[1] - a[0]) * s)
    if A == 12:
        return (-(a[0] + a[1]) * s, (a[0] - a[1]) * s) if inv else ((a[1] - a[0]) * s, -(a[0] + a[1]) * s)
    c = COS32[A] if A <= 8 else -COS32[16 - A]
    sn = COS32[8 - A] if A <= 8 else COS32[A - 8]
    return cmul(a, (c, sn if inv else -sn))


def _radix2(x, inv):
    R = len(x)
    if R == 1:
        return x
    a = [cadd(x[i], x[i + R // 2]) for i in range(R // 2)]
    b = [mul_wconst(R, i, inv, csub(x[i], x[i + R // 2])) for i in range(R // 2)]
    a, b = _radix2(a, inv), _radix2(b, inv)
    out = [None] * R
    out[0::2], out[1::2] = a, b
    return out


# ---- Dft16Lean: radix 4 x 4 -----------------------------------------------------------------------------------------------
def _scale(m):
    return {1: C1, 3: C1, 2: C2, 6: -C2, 9: -C1}.get(m, 1.0)


def _rot(m, a, inv, t1, fault):
    """u with W_16^(+-m) a = _scale(m) u"""
    if m in (1, 9):
        t = -t1 if inv else t1
        return (fma(t, a[1], a[0]), fma(-t, a[0], a[1]))
    if m == 3:
        if inv:
            return (fma(t1, a[0], -a[1]), fma(t1, a[1], a[0]))
        im = fma(t1, a[1], a[0]) if fault == "sign" else fma(t1, a[1], -a[0])
        return (fma(t1, a[0], a[1]), im)
    if m == 4:
        return mul_mi(a, inv)
    if (m == 2) != inv:                     # a (1 - i)
        return (a[0] + a[1], a[1] - a[0])
    return (a[0] - a[1], a[0] + a[1])       # a (1 + i)


def _dft4(a0, a1, a2, a3, inv):
    y0, y1, y2, y3 = cadd(a0, a2), csub(a0, a2), cadd(a1, a3), mul_mi(csub(a1, a3), inv)
    return cadd(y0, y2), cadd(y1, y3), csub(y0, y2), csub(y1, y3)


def _column(k2, a0, a1, a2, a3, inv, t1, fault):
    s1, s2, s3 = _scale(k2), _scale(2 * k2), _scale(3 * k2)
    assert abs(s3) == abs(s1)
    u1, u2, u3 = _rot(k2, a1, inv, t1, fault), _rot(2 * k2, a2, inv, t1, fault), _rot(3 * k2, a3, inv, t1, fault)
    if s2 == 1.0:
        y0, y1 = cadd(a0, u2), csub(a0, u2)
    else:
        y0 = (fma(s2, u2[0], a0[0]), fma(s2, u2[1], a0[1]))
        y1 = (fma(-s2, u2[0], a0[0]), fma(-s2, u2[1], a0[1]))
    z2, z3 = (cadd(u1, u3), csub(u1, u3)) if s3 == s1 else (csub(u1, u3), cadd(u1, u3))
    sq = -s1 if inv else s1
    return ((fma(s1, z2[0], y0[0]), fma(s1, z2[1], y0[1])), (fma(sq, z3[1], y1[0]), fma(-sq, z3[0], y1[1])),
            (fma(-s1, z2[0], y0[0]), fma(-s1, z2[1], y0[1])), (fma(-sq, z3[1], y1[0]), fma(sq, z3[0], y1[1])))


def _lean(x, inv, fault):
    t1 = T1 + 1e-14 if fault == "constant" else T1
    x = list(x)
    for n1 in range(4):                     # x[n1 + 4 k2] = first-layer output (n1, k2)
        x[n1], x[n1 + 4], x[n1 + 8], x[n1 + 12] = _dft4(x[n1], x[n1 + 4], x[n1 + 8], x[n1 + 12], inv)
    x[0:4] = _dft4(x[0], x[1], x[2], x[3], inv)
    for k2 in (1, 2, 3):
        x[4 * k2:4 * k2 + 4] = _column(k2, *x[4 * k2:4 * k2 + 4], inv, t1, fault)
    return [x[4 * (k % 4) + k // 4] for k in range(16)]         # x[4 k2 + k1] holds bin 4 k1 + k2


def _run(form, x, inv, **kw):
    x = np.asarray(x, dtype=np.complex128)
    assert x.shape[-1] == 16
    parts = [(np.ascontiguousarray(x[..., r].real), np.ascontiguousarray(x[..., r].imag)) for r in range(16)]
    out = form(parts, inv, **kw)
    y = np.empty(x.shape, dtype=np.complex128)
    for r in range(16):
        y[..., r].real, y[..., r].imag = out[r]
    return y


def dft16_radix2(x, inv=False):
    return _run(_radix2, x, inv)


def dft16_lean(x, inv=False, fault=None):
    return _run(_lean, x, inv, fault=fault)


# ---- the exact transform ---------------------------------------------------------------------------------------------------
def dft16_exact(x, inv=False):
    """sum_n x[n] exp(-+2 pi i n k / 16) in long double; the 16 roots come from cos and sin of angles up to pi/4 only."""
    c = [LD(1), np.cos(np.arctan(LD(1)) / 2), np.sqrt(LD(0.5))]
    s = [LD(0), np.sin(np.arctan(LD(1)) / 2), np.sqrt(LD(0.5))]
    re = c + [s[1], s[0]]                   # cos(m pi / 8), m = 0 .. 4
    im = s + [c[1], c[0]]
    roots = np.empty(16, dtype=CLD)
    for m in range(16):
        q, r = divmod(m, 4)
        a, b = re[r], im[r]
        for _ in range(q):
            a, b = -b, a                    # times i
        roots.real[m], roots.imag[m] = a, (b if inv else -b)
    n = np.arange(16)
    W = roots[(n[:, None] * n[None, :]) % 16]
    return np.asarray(x).astype(CLD) @ W


def largest_error(y, want):
    y = np.asarray(y).astype(CLD)
    return float(max(np.max(np.abs(y.real - want.real)), np.max(np.abs(y.imag - want.imag))))


def inputs(seed=16):
    """{name: x [n, 16]}: the 16 unit vectors, the 16 single-bin inputs exp(2 pi i k n / 16), 1000 random vectors."""
    n = np.arange(16)
    rng = np.random.default_rng(seed)
    return {"unit vectors": np.eye(16, dtype=np.complex128),
            "single bins": np.exp(2j * np.pi * ((n[:, None] * n[None, :]) % 16) / 16.0),
            "random": rng.standard_normal((1000, 16)) + 1j * rng.standard_normal((1000, 16))}
