"""qh::sweep_walk (quisk_amd/csrc/qh_design.cpp: plain C++, compiled here with g++) against the restatement's count of the reference's own
addition chain (tests/wdsp_gen_ref.py sweep_period, wdsp/gen.c:253-258): the period P the engine's sweep resets by, the table of the
chain's (phs, dphs) the kernel starts its quadratics from, and the closed-form count beyond the walk's cap.  CPU only."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

from wdsp_gen_ref import TWOPI, Gen, sweep_period

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHIM = r'''
#include "qh_design.hpp"
extern "C" long long t_sweep_walk(double rate, double f1, double f2, double sweeprate, long long max_walk, int ck_step, double *full, int *walked,
                                  double *ck, int ck_room, int *nck)
{
    const qh::SweepWalk w = qh::sweep_walk(rate, f1, f2, sweeprate, max_walk, ck_step);
    *full = w.full; *walked = w.walked ? 1 : 0; *nck = (int)w.ck.size();
    for (int i = 0; i < (int)w.ck.size() && i < ck_room; i++) { ck[2 * i] = w.ck[i].first; ck[2 * i + 1] = w.ck[i].second; }
    return w.P;
}
'''
RATE = 48000.0
STEP = 16384
CASES = [(-2000.0, 2000.0, 400000.0), (-1000.0, 3000.0, 250000.0), (-2000.0, 2001.7, 400000.0), (-20000.0, 20000.0, 4000.0),
         (0.0, 1000.0, -5000.0),            # a negative rate: it never resets
         (1000.0, 0.0, 5000.0)]             # f2 < f1: every sample resets


@pytest.fixture(scope="module")
def design(tmp_path_factory):
    if not shutil.which("g++"):
        pytest.skip("no g++")
    d = tmp_path_factory.mktemp("design_gen")
    (d / "shim.cpp").write_text(SHIM)
    so = d / "libdesigngen.so"
    csrc = os.path.join(ROOT, "quisk_amd", "csrc")
    subprocess.run(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-I", csrc, str(d / "shim.cpp"), os.path.join(csrc, "qh_design.cpp"), "-o", str(so)], check=True)
    lib = C.CDLL(str(so))
    lib.t_sweep_walk.restype = C.c_longlong
    return lib


def _walk(lib, f1, f2, rate, max_walk=1 << 27, room=64):
    full, walked, nck = C.c_double(0), C.c_int(0), C.c_int(0)
    ck = np.zeros(2 * room)
    P = lib.t_sweep_walk(C.c_double(RATE), C.c_double(f1), C.c_double(f2), C.c_double(rate), C.c_longlong(max_walk), C.c_int(STEP), C.byref(full),
                         C.byref(walked), ck.ctypes.data_as(C.POINTER(C.c_double)), C.c_int(room), C.byref(nck))
    return P, full.value, walked.value, ck[:2 * nck.value].reshape(-1, 2)


@pytest.mark.parametrize("f1,f2,rate", CASES)
def test_the_walk_counts_what_the_reference_chain_counts(design, f1, f2, rate):
    P, full, walked, ck = _walk(design, f1, f2, rate)
    want = sweep_period(RATE, f1, f2, rate)
    print("f1 %g f2 %g rate %g: P %d (restatement %d), %d table entries" % (f1, f2, rate, P, want, len(ck)))
    assert walked == 1 and P == want
    assert len(ck) == (P + STEP - 1) // STEP


def test_the_defaults_are_the_tie_a_closed_form_gets_wrong(design):
    P, _, _, _ = _walk(design, -20000.0, 20000.0, 4000.0)
    assert P == 480000                                          # exact arithmetic and a strict `>` would give 480001


def test_the_table_is_the_literal_chain(design):
    """(phs, dphs) of the literal xgen every 16384 samples of the default sweep's first period, bit for bit, and phs at the period's end"""
    P, full, _, ck = _walk(design, -20000.0, 20000.0, 4000.0)
    g = Gen(RATE, STEP, run=1, mode=3)
    for j in range(len(ck)):
        assert (g.sweep_phs, g.sweep_dphs) == (ck[j][0], ck[j][1]), j
        g.size = min(STEP, P - j * STEP)
        g.block()
    assert g.sweep_phs == full and g.sweep_dphs == TWOPI * -20000.0 / RATE


def test_beyond_the_cap_the_count_is_the_closed_forms(design):
    """with the cap at 1000 additions the default sweep is not walked: floor((dphsmax - dphs) / d2phs) + 1 = 480001 here, one more than
    the chain's own count (the deviation DESIGN.md b20 states for periods beyond 2^27 samples)"""
    P, full, walked, ck = _walk(design, -20000.0, 20000.0, 4000.0, max_walk=1000)
    assert walked == 0 and len(ck) == 0
    assert P in (480000, 480001)
    assert 0.0 <= abs(full) < TWOPI
