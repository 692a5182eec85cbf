"""The host design of the fixed-ratio resampler bank, compiled here with g++ (quisk_amd/csrc/qh_design.cpp): qh::design_resampler with
its fc_low, qh::design_resampler_fv, qh::resampler_phase_major and qh::resampler_sizes against the restatement's calc_resample and
create_resampleF (tests/wdsp_resample_ref.py, whose prototype is the oracle's fir_bandpass).  CPU only."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

from wdsp_resample_ref import calc_resample, calc_resample_f

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHIM = r'''
#include <cstring>
#include "qh_design.hpp"
static int put(const qh::ResamplerDesign &d, double *nat, double *pm, int cap, int *LM)
{
    LM[0] = d.L; LM[1] = d.M; LM[2] = d.ncoef; LM[3] = d.cpp;
    if (d.ncoef <= cap) {
        std::memcpy(nat, d.h.data(), (size_t)d.ncoef * 8);
        const std::vector<double> h = qh::resampler_phase_major(d);
        std::memcpy(pm, h.data(), (size_t)d.ncoef * 8);
    }
    return d.ncoef;
}
extern "C" int t_old(int in_rate, int out_rate, double fc, int ncoef, double gain, double *nat, double *pm, int cap, int *LM)
{ return put(qh::design_resampler(in_rate, out_rate, fc, ncoef, gain), nat, pm, cap, LM); }
extern "C" int t_new(int in_rate, int out_rate, double fc, int ncoef, double gain, double fc_low, double *nat, double *pm, int cap, int *LM)
{ return put(qh::design_resampler(in_rate, out_rate, fc, ncoef, gain, fc_low), nat, pm, cap, LM); }
extern "C" int t_fv(int in_rate, int out_rate, double *nat, double *pm, int cap, int *LM)
{ return put(qh::design_resampler_fv(in_rate, out_rate), nat, pm, cap, LM); }
extern "C" long long t_sizes(int in_rate, int out_rate, int ncoef, int fv, int *LM)
{ long long n; qh::resampler_sizes(in_rate, out_rate, ncoef, fv != 0, &LM[0], &LM[1], &n); return n; }
'''
CAP = 1 << 18
PAIRS = [(48000, 44100), (44100, 48000), (96000, 48000), (48000, 96000), (48000, 48000), (384000, 48000)]


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    if not shutil.which("g++"):
        pytest.skip("no g++")
    d = tmp_path_factory.mktemp("design_resample")
    (d / "shim.cpp").write_text(SHIM)
    so = d / "libdesignresample.so"
    csrc = os.path.join(ROOT, "quisk_amd", "csrc")
    subprocess.run(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-I", csrc, str(d / "shim.cpp"), os.path.join(csrc, "qh_design.cpp"), "-o", str(so)], check=True)
    lib = C.CDLL(str(so))
    vp, ip = C.c_void_p, C.POINTER(C.c_int)
    lib.t_old.argtypes = [C.c_int, C.c_int, C.c_double, C.c_int, C.c_double, vp, vp, C.c_int, ip]
    lib.t_new.argtypes = [C.c_int, C.c_int, C.c_double, C.c_int, C.c_double, C.c_double, vp, vp, C.c_int, ip]
    lib.t_fv.argtypes = [C.c_int, C.c_int, vp, vp, C.c_int, ip]
    lib.t_sizes.argtypes = [C.c_int, C.c_int, C.c_int, C.c_int, ip]
    lib.t_sizes.restype = C.c_longlong
    return lib


def _call(fn, *args):
    nat, pm, lm = np.zeros(CAP), np.zeros(CAP), (C.c_int * 4)()
    n = fn(*args, nat.ctypes.data, pm.ctypes.data, CAP, lm)
    assert n <= CAP
    return tuple(lm), nat[:n], pm[:n]


@pytest.mark.parametrize("design", [p + (0.0, 0, 1.0) for p in PAIRS] + [(48000, 44100, 9000.0, 5000, 0.5), (192000, 48000, 0.0, 0, 1.0)])
@pytest.mark.parametrize("fc_low", [-1.0, -0.25, -7000.0])
def test_a_negative_fc_low_gives_the_old_taps_bit_for_bit(host, design, fc_low):
    lm0, nat0, pm0 = _call(host.t_old, *design)
    lm1, nat1, pm1 = _call(host.t_new, *design, fc_low)
    assert lm0 == lm1 and np.array_equal(nat0, nat1) and np.array_equal(pm0, pm1)
    L, M, ncoef, cpp = lm0
    assert np.array_equal(pm0.reshape(L, cpp), nat0.reshape(cpp, L).T)  # resample.c:69-72


@pytest.mark.parametrize("design", [(48000, 44100, 9000.0, 0, 1.0, 300.0), (44100, 48000, 0.0, 0, 1.0, 0.0), (96000, 48000, 12000.0, 999, 2.0, 150.0),
                                    (48000, 96000, 0.0, 0, 1.0, 2500.0)])
def test_fc_low_is_calc_resample(oracle, host, design):
    in_rate, out_rate, fc, ncoef, gain, fc_low = design
    L, M, nc, cpp, h = calc_resample(in_rate, out_rate, fc, ncoef, gain, fc_low)
    lm, nat, pm = _call(host.t_new, *design)
    assert lm == (L, M, nc, cpp)
    worst = float(np.max(np.abs(pm - h))) / float(np.max(np.abs(h)))
    print("resample design %s: worst %.3e of the largest tap" % (design, worst))
    assert worst <= 4e-16


@pytest.mark.parametrize("pair", PAIRS)
def test_the_float_design_is_create_resampleF(oracle, host, pair):
    L, M, nc, cpp, h = calc_resample_f(*pair)
    lm, nat, pm = _call(host.t_fv, *pair)
    assert lm == (L, M, nc, cpp)
    worst = float(np.max(np.abs(pm - h))) / float(np.max(np.abs(h)))
    print("resampleF design %s: cpp %d, worst %.3e of the largest tap" % (pair, cpp, worst))
    assert worst <= 4e-16


def test_sizes_in_64_bits(oracle, host):
    lm = (C.c_int * 2)()
    for pair in PAIRS:
        assert host.t_sizes(*pair, 0, 0, lm) == calc_resample(*pair)[2] and tuple(lm) == calc_resample(*pair)[:2]
        assert host.t_sizes(*pair, 0, 1, lm) == calc_resample_f(*pair)[2]
    # what the bank refuses: the reference's ints would not hold these
    assert host.t_sizes(48000, 44101, 0, 0, lm) == (int(140.0 * 48000.0 * 44101 / 44101) // 44101 + 1) * 44101 and tuple(lm) == (44101, 48000)
    assert host.t_sizes(1, 2000000000, 2147483647, 0, lm) > 2 ** 31
