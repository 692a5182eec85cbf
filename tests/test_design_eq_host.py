"""qh::eq_impulse (quisk_amd/csrc/qh_design.cpp: plain C++, compiled here with g++) against the restatement of wdsp/eq.c:39-158 in
tests/wdsp_fmsq_ref.py: WDSP's piecewise-linear-in-dB frequency-sampling design, which the FM squelch's noise filter is made with.
CPU only."""
import ctypes as C
import math
import os
import shutil
import subprocess

import numpy as np
import pytest

from wdsp_fmsq_ref import eq_impulse, fmsq_impulse, pllpole

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHIM = r'''
#include <cstring>
#include <stdexcept>
#include "qh_design.hpp"
extern "C" int t_eq_impulse(int N, int nfreqs, const double *F, const double *G, double fs, double scale, int ctfmode, int wintype, double *out)
{
    try { auto h = qh::eq_impulse(N, nfreqs, F, G, fs, scale, ctfmode, wintype); std::memcpy(out, h.data(), h.size() * 16); return 0; }
    catch (const std::exception &) { return -1; }
}
extern "C" void t_fmsq_impulse(int nc, double fs, double scale, double *out)
{ auto h = qh::fmsq_impulse(nc, fs, scale); std::memcpy(out, h.data(), h.size() * 16); }
extern "C" void t_fmsq_mp(int nc, double fs, double scale, double *out)
{ auto h = qh::mp_imp(qh::fmsq_impulse(nc, fs, scale), 16, 0); std::memcpy(out, h.data(), h.size() * 16); }
extern "C" double t_pllpole(double zeta, double omegaN) { return qh::fm_pllpole(zeta, omegaN); }
'''


@pytest.fixture(scope="module")
def design(tmp_path_factory):
    if not shutil.which("g++"):
        pytest.skip("no g++")
    d = tmp_path_factory.mktemp("design_eq")
    (d / "shim.cpp").write_text(SHIM)
    so = d / "libdesigneq.so"
    csrc = os.path.join(ROOT, "quisk_amd", "csrc")
    subprocess.run(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-I", csrc, str(d / "shim.cpp"), os.path.join(csrc, "qh_design.cpp"), "-o", str(so)], check=True)
    lib = C.CDLL(str(so))
    lib.t_pllpole.restype = C.c_double
    lib.t_pllpole.argtypes = [C.c_double, C.c_double]
    return lib


def _taps(lib, N, F, G, fs, scale, ctfmode, wintype):
    out = np.zeros(N, dtype=np.complex128)
    Fa, Ga = (C.c_double * len(F))(*F), (C.c_double * len(G))(*G)
    rc = lib.t_eq_impulse(C.c_int(N), C.c_int(len(F) - 1), Fa, Ga, C.c_double(fs), C.c_double(scale), C.c_int(ctfmode), C.c_int(wintype),
                          out.ctypes.data_as(C.c_void_p))
    return rc, out


def _fmsq_points():
    pp = pllpole()
    return [0.0, 5000.0, pp, 20000.0], [0.0, 0.0, 3.0, 20.0 * math.log10(20000.0 / pp)]


@pytest.mark.parametrize("nc", [256, 2048, 4096])
@pytest.mark.parametrize("rate", [24000.0, 48000.0, 96000.0])
@pytest.mark.parametrize("wintype", [0, 1])
@pytest.mark.parametrize("ctfmode", [0, 1])
def test_eq_impulse_is_the_restated_design(design, nc, rate, wintype, ctfmode):
    """the squelch's design points (at 24 kHz the upper two clamp to Nyquist and tie: both sides keep the input order there)"""
    F, G = _fmsq_points()
    rc, out = _taps(design, nc, F, G, rate, 1.0 / 512, ctfmode, wintype)
    assert rc == 0 and np.all(out.imag == 0.0)
    want = eq_impulse(nc, 3, F, G, rate, 1.0 / 512, ctfmode, wintype)
    assert np.abs(out.real - want).max() <= 1e-12 * np.abs(want).max()


@pytest.mark.parametrize("ctfmode", [0, 1])
def test_unsorted_points_and_a_preamp(design, ctfmode):
    F = [0.0, 6000.0, 300.0, 12000.0, 1500.0, 3000.0]
    G = [-2.5, 4.0, -6.0, -12.0, 0.0, 3.0]
    rc, out = _taps(design, 2048, F, G, 48000.0, 1.0, ctfmode, 1)
    want = eq_impulse(2048, 5, F, G, 48000.0, 1.0, ctfmode, 1)
    assert rc == 0 and np.abs(out.real - want).max() <= 1e-12 * np.abs(want).max()
    order = np.argsort(F[1:])
    Fs, Gs = [0.0] + [F[1 + k] for k in order], [G[0]] + [G[1 + k] for k in order]
    rc, srt = _taps(design, 2048, Fs, Gs, 48000.0, 1.0, ctfmode, 1)
    assert rc == 0 and np.array_equal(out, srt)                # the sort is the design's own


def test_odd_n_throws(design):
    F, G = _fmsq_points()
    assert _taps(design, 2047, F, G, 48000.0, 1.0, 0, 0)[0] == -1


@pytest.mark.parametrize("nc,rate", [(2048, 48000.0), (4096, 96000.0), (256, 48000.0)])
def test_fmsq_filter_is_symmetric_and_passes_through_its_design_points(design, nc, rate):
    out = np.zeros(nc, dtype=np.complex128)
    design.t_fmsq_impulse(C.c_int(nc), C.c_double(rate), C.c_double(1.0), out.ctypes.data_as(C.c_void_p))
    h = out.real
    assert np.all(out.imag == 0.0) and np.abs(h - h[::-1]).max() <= 1e-18 + 1e-15 * np.abs(h).max()
    assert np.abs(h - fmsq_impulse(nc, rate, 0.5)).max() <= 1e-12 * np.abs(h).max()       # (size 0.5: scale 1 kept)
    assert design.t_pllpole(1.0, 20000.0) == pllpole() and abs(pllpole() - 7901.0) < 1.0
    if nc < 2048:
        return                                                 # 256 taps at 48 kHz: bins 187.5 Hz wide, the window smears the corners
    F, G = _fmsq_points()
    nfft = 16 * nc
    H = 20.0 * np.log10(np.maximum(np.abs(np.fft.fft(h, nfft)), 1e-300))
    for f, g in zip(F[1:], G[1:]):
        got = H[int(round(f / rate * nfft))]
        assert abs(got - g) < 0.5, (f, g, got)


@pytest.mark.parametrize("nc", [256, 2048, 4096])
def test_minimum_phase_taps_real_parts_give_the_reference_noise(design, nc):
    """The engine runs the squelch's noise filter as a real filter and so keeps the real parts of mp_imp's taps (deviations of
    xfmsq).  The reference filters the signal (t, t) with the complex taps yr + j yi: n0 = yr - yi, n1 = yr + yi, noise = sqrt(2 (yr^2 +
    yi^2)).  With the real parts alone it is sqrt(2) |yr|: the two differ by yi^2 / (2 yr^2) relative, second order in a residue that is
    itself rounding beside a real minimum-phase design -- held here to 1e-12 of the noise's RMS on a white trigger."""
    out = np.zeros(nc, dtype=np.complex128)
    design.t_fmsq_mp(C.c_int(nc), C.c_double(48000.0), C.c_double(1.0), out.ctypes.data_as(C.c_void_p))
    assert np.abs(out.imag).max() <= 1e-6 * np.abs(out.real).max()
    assert np.abs(out[:nc // 8]).max() == np.abs(out).max()                # minimum phase: the weight sits at the front
    x = np.random.default_rng(nc).standard_normal(20000)
    y, yr = np.convolve(x, out, mode="valid"), np.convolve(x, out.real, mode="valid")
    z = (1.0 + 1.0j) * y
    ref, got = np.sqrt(z.real * z.real + z.imag * z.imag), np.sqrt(yr * yr + yr * yr)
    assert np.abs(ref - got).max() <= 1e-12 * np.sqrt(np.mean(ref * ref))
