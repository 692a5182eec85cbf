"""qh::eq_impulse and qh::mp_imp (quisk_amd/csrc/qh_design.cpp: plain C++, compiled here with g++) at the shapes the equalizer's setters
produce, against the restatement of wdsp/eq.c:39-158 (tests/wdsp_fmsq_ref.py) and the oracle's mp_imp.  CPU only.

The bound on eq_impulse is the one tests/test_design_eq_host.py uses: 1e-12 of the largest tap."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

from wdsp_eqp_ref import DEFAULT_F, GRPH_F, mp_imp
from wdsp_fmsq_ref import eq_impulse

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHIM = r'''
#include <cstring>
#include <stdexcept>
#include "qh_design.hpp"
extern "C" int t_eq_impulse(int N, int nfreqs, const double *F, const double *G, double fs, double scale, int ctfmode, int wintype, int mp, double *out)
{
    try {
        auto h = qh::eq_impulse(N, nfreqs, F, G, fs, scale, ctfmode, wintype);
        if (mp) h = qh::mp_imp(h, 16, 0);
        std::memcpy(out, h.data(), h.size() * 16);
        return 0;
    } catch (const std::exception &) { return -1; }
}
'''
G10 = [3.0, -12.0, 12.0, -6.0, 9.0, 0.0, -12.0, 12.0, 4.0, -9.0, 7.0]
PROFILES = {
    "grph": (GRPH_F, [2.0, -6.0, -6.0, 8.0, -11.0]),                               # SetRXAGrphEQ: nfreqs 4, G[1] = G[2]
    "grph10": (DEFAULT_F, G10),                                                    # SetRXAGrphEQ10 / the default frequencies
    "unsorted": ([0.0, 5000.0, 200.0, 9000.0, 1200.0], [-1.5, 6.0, -9.0, -3.0, 4.0]),
    "above_nyquist": ([0.0, 300.0, 2500.0, 40000.0], [0.0, -4.0, 5.0, -8.0]),      # one clamp to 1.0 at both rates
}


@pytest.fixture(scope="module")
def design(tmp_path_factory):
    if not shutil.which("g++"):
        pytest.skip("no g++")
    d = tmp_path_factory.mktemp("design_eqp")
    (d / "shim.cpp").write_text(SHIM)
    so = d / "libdesigneqp.so"
    csrc = os.path.join(ROOT, "quisk_amd", "csrc")
    subprocess.run(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-I", csrc, str(d / "shim.cpp"), os.path.join(csrc, "qh_design.cpp"), "-o", str(so)], check=True)
    return C.CDLL(str(so))


def _taps(lib, N, F, G, fs, scale, ctfmode, wintype, mp=0):
    out = np.zeros(N, dtype=np.complex128)
    Fa, Ga = (C.c_double * len(F))(*F), (C.c_double * len(G))(*G)
    rc = lib.t_eq_impulse(C.c_int(N), C.c_int(len(F) - 1), Fa, Ga, C.c_double(fs), C.c_double(scale), C.c_int(ctfmode), C.c_int(wintype), C.c_int(mp),
                          out.ctypes.data_as(C.c_void_p))
    assert rc == 0
    return out


@pytest.mark.parametrize("rate", [48000.0, 12000.0])
@pytest.mark.parametrize("nc", [256, 2048, 4096])
@pytest.mark.parametrize("wintype", [0, 1])
@pytest.mark.parametrize("ctfmode", [0, 1])
@pytest.mark.parametrize("profile", sorted(PROFILES))
def test_eq_impulse_is_the_restated_design(design, profile, ctfmode, wintype, nc, rate):
    """(at 12 kHz the default frequencies 8000 and 16000 Hz both clamp to Nyquist; the profiles that tie there have equal gains only
    where the engine accepts them, and both sides keep the input order otherwise, as tests/test_design_eq_host.py notes)"""
    F, G = PROFILES[profile]
    out = _taps(design, nc, F, G, rate, 1.0 / 512, ctfmode, wintype)
    assert np.all(out.imag == 0.0)
    want = eq_impulse(nc, len(F) - 1, F, G, rate, 1.0 / 512, ctfmode, wintype)
    err = np.abs(out.real - want).max() / np.abs(want).max()
    print("%s ctfmode %d wintype %d nc %d rate %.0f: %.3g of the largest tap" % (profile, ctfmode, wintype, nc, rate, err))
    assert err <= 1e-12


# qh::mp_imp against the oracle's mp_imp, largest tap difference over the largest tap, worst case per nc as first measured; the bound is ten
# times that
MP_MEASURED = {256: 0.22, 2048: 0.0427, 4096: 0.0357}


@pytest.mark.parametrize("rate", [48000.0, 12000.0])
@pytest.mark.parametrize("nc", [256, 2048, 4096])
@pytest.mark.parametrize("wintype", [0, 1])
@pytest.mark.parametrize("profile", sorted(PROFILES))
def test_minimum_phase_taps_at_ctfmode_1_are_the_oracles(design, profile, wintype, nc, rate):
    """qh::mp_imp against the oracle's mp_imp on the same design at ctfmode 1, complex taps kept.  Measured: at most 0.22 (nc 256), 0.0427
    (nc 2048), 0.0357 (nc 4096) of the largest tap; bound: ten times that, 2.2 / 0.427 / 0.357.

    These figures are large because ctfmode 1 does not make mp_imp well conditioned: an even-length linear-phase design has a zero at
    Nyquist whatever its skirts, so one bin of mp_imp's 16 nc-point spectrum holds the transform's rounding (1e-17 of the peak) or an exact
    0 (taken as 1e-300), and its logarithm -- hundreds of nepers apart between two FFT implementations -- turns the phase of the bins
    around it.  Where both transforms give an exact 0 there (grph10, wintype 0, nc 2048, 48 kHz) the two sets of taps agree to 1.9e-15.
    So, as at ctfmode 0, signal tests with mp 1 take the library's own taps (debug_eqp)."""
    F, G = PROFILES[profile]
    got = _taps(design, nc, F, G, rate, 1.0 / 512, 1, wintype, mp=1)
    want = mp_imp(eq_impulse(nc, len(F) - 1, F, G, rate, 1.0 / 512, 1, wintype).astype(np.complex128))
    err = np.abs(got - want).max() / np.abs(want).max()
    print("mp %s wintype %d nc %d rate %.0f: %.3g of the largest tap" % (profile, wintype, nc, rate, err))
    assert np.abs(got[:nc // 4]).max() == np.abs(got).max()                     # minimum phase: the weight sits at the front
    assert err <= 10.0 * MP_MEASURED[nc]
    if (profile, wintype, nc, rate) == ("grph10", 0, 2048, 48000.0):
        # both transforms give an exact 0 at the Nyquist bin here (taken as 1e-300 on both sides): nothing is left to rounding, and
        # qh::mp_imp with its complex taps kept is the oracle's to the design's own bound (1.9e-15 measured)
        assert err <= 1e-12, err
