"""The host side of the variable-ratio resampler bank, compiled here with g++: qh::design_varsamp (quisk_amd/csrc/qh_design.cpp)
against the restatement's calc_varsamp, whose h is the oracle's fir_bandpass, and the host build of qh::varsamp_walk
(quisk_amd/csrc/qh_varsamp.hpp, the function the bank's walk kernel runs one lane per channel) against the restatement's xvarsamp: the
counts, every output's input index and h_offset, and the state behind every call, bit for bit.  CPU only."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

from wdsp_varsamp_ref import Varsamp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHIM = r'''
#include "qh_design.hpp"
#include "qh_varsamp.hpp"
extern "C" int t_varsamp_design(int in_rate, int out_rate, int R, double fc, double fc_low, double gain, double *nom_ratio, int *rsize, double *h, int room)
{
    const qh::VarsampDesign d = qh::design_varsamp(in_rate, out_rate, R, fc, fc_low, gain);
    *nom_ratio = d.nom_ratio; *rsize = d.rsize;
    for (int i = 0; i < d.ncoef && i < room; i++) h[i] = d.h[i];
    return d.ncoef;
}
extern "C" int t_varsamp_walk(double *state, int n, double var, double nom_ratio, int varmode, int run, int *rec_i, double *rec_h, int room)
{
    qh::VarsampState s{state[0], state[1], state[2], state[3]};
    const int c = qh::varsamp_walk(s, n, var, nom_ratio, varmode, run, [&](int m, int i, double h) { if (m < room) { rec_i[m] = i; rec_h[m] = h; } });
    state[0] = s.inv_cvar; state[1] = s.h_offset; state[2] = s.isamps; state[3] = s.var;
    return c;
}
'''
PAIRS = [(48000, 48000, 1024), (48000, 96000, 64), (96000, 48000, 64)]
VARS = (0.96, 0.97, 1.0, 1.0003, 1.01, 1.04)


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    if not shutil.which("g++"):
        pytest.skip("no g++")
    d = tmp_path_factory.mktemp("design_varsamp")
    (d / "shim.cpp").write_text(SHIM)
    so = d / "libdesignvarsamp.so"
    csrc = os.path.join(ROOT, "quisk_amd", "csrc")
    subprocess.run(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-I", csrc, str(d / "shim.cpp"), os.path.join(csrc, "qh_design.cpp"), "-o", str(so)], check=True)
    lib = C.CDLL(str(so))
    dp, ip = C.POINTER(C.c_double), C.POINTER(C.c_int)
    lib.t_varsamp_design.argtypes = [C.c_int, C.c_int, C.c_int, C.c_double, C.c_double, C.c_double, dp, ip, dp, C.c_int]
    lib.t_varsamp_walk.argtypes = [dp, C.c_int, C.c_double, C.c_double, C.c_int, C.c_int, ip, dp, C.c_int]
    return lib


def _design(lib, in_rate, out_rate, R, fc=0.0, fc_low=-1.0, gain=1.0):
    nom, rsize = C.c_double(0), C.c_int(0)
    room = 2240 * R + 1
    h = np.zeros(room)
    ncoef = lib.t_varsamp_design(in_rate, out_rate, R, fc, fc_low, gain, C.byref(nom), C.byref(rsize), h.ctypes.data_as(C.POINTER(C.c_double)), room)
    return nom.value, rsize.value, ncoef, h[:ncoef]


@pytest.mark.parametrize("design", [p + (0.0, -1.0, 1.0) for p in PAIRS] + [(48000, 44100, 256, 0.0, -1.0, 1.0), (48000, 48000, 64, 9000.0, 300.0, 0.5),
                                                                          (384000, 48000, 64, 0.0, -1.0, 1.0)])
def test_the_design_is_calc_varsamp(oracle, host, design):
    in_rate, out_rate, R, fc, fc_low, gain = design
    ref = Varsamp(in_rate, out_rate, R, fc=fc, fc_low=fc_low, gain=gain)
    nom, rsize, ncoef, h = _design(host, *design)
    assert (nom, rsize, ncoef) == (ref.nom_ratio, ref.rsize, ref.ncoef)
    worst = float(np.max(np.abs(h - ref.h))) / float(np.max(np.abs(ref.h)))
    print("varsamp design %s: rsize %d, ncoef %d, %d coefficients differ, worst %.3e of max|h|" % (design, rsize, ncoef, np.count_nonzero(h != ref.h), worst))
    if not np.array_equal(h, ref.h):
        assert worst <= 1e-15


@pytest.mark.parametrize("varmode", [0, 1])
@pytest.mark.parametrize("pair", PAIRS)
def test_the_walk_is_xvarsamp_bit_for_bit(oracle, host, pair, varmode):
    in_rate, out_rate, R = pair
    rng = np.random.default_rng(in_rate // 1000 + varmode)
    cuts = [0, 1, 2, 300, 301, 440, 440, 700, 1400]                      # one-sample calls, an empty call, ragged ones
    var = [VARS[k] for k in rng.permutation(len(VARS))] + [1.0003, 0.96, 1.04]
    ref = Varsamp(in_rate, out_rate, R, var=1.0, varmode=varmode)
    x = rng.standard_normal(cuts[-1]) + 0j
    state = np.array([ref.inv_cvar, ref.h_offset, ref.isamps, ref.var])
    room = 4096
    ri, rh = np.zeros(room, dtype=np.int32), np.zeros(room)
    total = 0
    for k, (a, b) in enumerate(zip(cuts[:-1], cuts[1:])):
        y, _ = ref.process(x[a:b], var[k])
        c = host.t_varsamp_walk(state.ctypes.data_as(C.POINTER(C.c_double)), b - a, var[k], ref.nom_ratio, varmode, 1,
                                ri.ctypes.data_as(C.POINTER(C.c_int)), rh.ctypes.data_as(C.POINTER(C.c_double)), room)
        assert c == len(y) and c <= room, (k, c, len(y))
        assert np.array_equal(ri[:c], np.array(ref.rec_i, dtype=np.int32)), k
        assert np.array_equal(rh[:c], np.array(ref.rec_h, dtype=np.float64)), k         # bit for bit
        assert tuple(state) == (ref.inv_cvar, ref.h_offset, ref.isamps, ref.var), k
        total += c
    print("varsamp walk %s varmode %d: %d outputs of %d inputs" % (pair, varmode, total, cuts[-1]))
    assert total > 0


def test_a_channel_that_does_not_run_still_follows_var(oracle, host):
    ref = Varsamp(48000, 48000, 64, varmode=0, run=0)
    state = np.array([ref.inv_cvar, ref.h_offset, ref.isamps, ref.var])
    y, _ = ref.process(np.ones(9, dtype=np.complex128), 1.02)
    c = host.t_varsamp_walk(state.ctypes.data_as(C.POINTER(C.c_double)), 9, 1.02, ref.nom_ratio, 0, 0, None, None, 0)
    assert c == 9 == len(y) and tuple(state) == (ref.inv_cvar, 0.0, 0.0, 1.02)
