"""The eight SetRXAPreGen* names bound as a WDSP caller binds them (wdsp/gen.c:384-450), through OpenChannel and fexchange0.  -m gpu.

The channels run with in rate = dsp rate and the shift off, so the whole-chain reference (tests/rxa_chain_ref.py) fed the restatement's
signal (tests/wdsp_gen_ref.py) is what the channel must put out, behind the channel's own latency of whole output buffers
(wdsp/iobuffs.c), which is read off the leading all-zero buffers and must be at most two.  fexchange0 is fed zeros: a channel whose
generator runs needs no input.  Bounds: 1e-9 relative RMS for the filter-only chain, 1e-6 for the seeded walk (the setter walks' gate)."""
import ctypes as C

import numpy as np
import pytest

from conftest import rel_rms
from rxa_chain_ref import RxaChainRef
from wdsp_gen_ref import Gen, default_seed, noise

pytestmark = pytest.mark.gpu
D = C.c_double
RATE, SIZE = 48000, 256


def _open(lib, ch, mode=1, passband=(300.0, 3000.0)):
    lib.OpenChannel(ch, SIZE, SIZE, RATE, RATE, RATE, 0, 1, D(0.010), D(0.025), D(0.0), D(0.010), 1)
    assert lib.qh_wdsp_status() == 0, lib.qh_last_error()
    lib.SetRXAShiftRun(ch, 0); lib.RXANBPSetRun(ch, 1)
    lib.SetRXAMode(ch, mode); lib.RXASetPassband(ch, D(passband[0]), D(passband[1]))
    lib.SetRXAAGCMode(ch, 0); lib.SetRXAAGCFixed(ch, D(0.0))
    assert lib.qh_wdsp_status() == 0, lib.qh_last_error()


def _ref(mode=1, passband=(300.0, 3000.0)):
    r = RxaChainRef(in_size=SIZE, dsp_size=SIZE, in_rate=RATE, dsp_rate=RATE, out_rate=RATE)
    r.SetRXAShiftRun(0); r.RXANBPSetRun(1)
    r.SetRXAMode(mode); r.RXASetPassband(*passband)
    r.SetRXAAGCMode(0); r.SetRXAAGCFixed(0.0)
    return r


def _blocks(lib, ch, nb, expect_ok=True):
    out = np.zeros(nb * SIZE, dtype=np.complex128)
    zeros = np.zeros(SIZE, dtype=np.complex128)
    err = C.c_int(0)
    for b in range(nb):
        lib.fexchange0(ch, zeros.ctypes.data_as(C.c_void_p), out[b * SIZE:].ctypes.data_as(C.c_void_p), C.byref(err))
        if expect_ok:
            assert err.value == 0 and lib.qh_wdsp_status() == 0, lib.qh_last_error()
    return out


def _latency(y):
    d = 0
    while d < 3 and not np.any(y[d * SIZE:(d + 1) * SIZE]):
        d += 1
    assert d <= 2, "the channel's latency is at most two output buffers"
    return d * SIZE


def test_a_tone_through_the_names(qh):
    lib = qh.load()
    _open(lib, 0)
    r = _ref()
    g = Gen(RATE, SIZE, run=0, mode=2)
    try:
        lib.SetRXAPreGenRun(0, 1); lib.SetRXAPreGenMode(0, 0); lib.SetRXAPreGenToneMag(0, D(0.5)); lib.SetRXAPreGenToneFreq(0, D(1234.5))
        g.SetRun(1); g.SetMode(0); g.SetToneMag(0.5); g.SetToneFreq(1234.5)
        y = _blocks(lib, 0, 40)
        ref = r.xrxa(g.blocks(40))
        lat = _latency(y)
        err = rel_rms(y[lat:], ref[:ref.size - lat])
        print("tone through the WDSP names: latency %d samples, rel rms %.3g" % (lat, err))
        assert np.abs(ref).max() > 0.1 and err < 1e-9
    finally:
        lib.CloseChannel(0); r.close()


def test_modes_4_and_5_are_refused_and_the_default_mode_runs(qh):
    """a fresh channel's generator is in mode 2, noise (RXA.c:60-66): it runs.  SetRXAPreGenMode 4 / 5: fexchange0 reports the refusal
    in qh_wdsp_status() and leaves the output buffer as the caller filled it."""
    lib = qh.load()
    _open(lib, 0)
    try:
        lib.SetRXAPreGenNoiseMag(0, D(0.1)); lib.SetRXAPreGenRun(0, 1)
        y = _blocks(lib, 0, 12)
        assert np.abs(y).max() > 1e-3 and np.all(np.isfinite(y.view(np.float64)))
        for m in (4, 5):
            lib.SetRXAPreGenMode(0, m)
            assert lib.qh_wdsp_status() == 0                    # the setter stores a field
            out = np.full(SIZE, 7.0 + 3.0j, dtype=np.complex128)
            err = C.c_int(0)
            lib.fexchange0(0, np.zeros(SIZE, dtype=np.complex128).ctypes.data_as(C.c_void_p), out.ctypes.data_as(C.c_void_p), C.byref(err))
            assert lib.qh_wdsp_status() != 0 and err.value != 0
            assert np.all(out == 7.0 + 3.0j)
        lib.SetRXAPreGenMode(0, 2)
        assert np.abs(_blocks(lib, 0, 4)).max() > 1e-3
    finally:
        lib.CloseChannel(0)


MODES = {0: (-3000.0, -300.0), 1: (300.0, 3000.0), 4: (300.0, 3000.0), 6: (-4000.0, 4000.0)}       # LSB, USB, CWU, AM


@pytest.mark.parametrize("seed", [3, 11])
def test_a_seeded_walk_over_the_names(qh, seed):
    """the eight names mixed with SetRXAMode / RXASetPassband, a few blocks between settings; the reference: the generator's restatement
    (the project's noise generator in mode 2, zeros while the generator is off) into the whole-chain reference"""
    lib = qh.load()
    rng = np.random.default_rng(seed)
    _open(lib, 1)
    r = _ref()
    g = Gen(RATE, SIZE, run=0, mode=2)
    drawn = 0                                                   # noise samples drawn so far
    ys, refs = [], []
    try:
        lib.SetRXAPreGenNoiseMag(1, D(0.05)); g.SetNoiseMag(0.05)
        for step in range(36):
            k = int(rng.integers(0, 10))
            if step == 0:
                lib.SetRXAPreGenRun(1, 1); g.SetRun(1)
            elif k == 0:
                run = int(rng.integers(0, 2))
                lib.SetRXAPreGenRun(1, run); g.SetRun(run)
            elif k == 1:
                m = int(rng.choice([0, 1, 2, 3, 6, 99, 0, 3]))
                lib.SetRXAPreGenMode(1, m); g.SetMode(m)
            elif k == 2:
                v = float(rng.uniform(0.05, 0.8))
                lib.SetRXAPreGenToneMag(1, D(v)); g.SetToneMag(v)
            elif k == 3:
                v = float(rng.uniform(-3500.0, 3500.0))
                lib.SetRXAPreGenToneFreq(1, D(v)); g.SetToneFreq(v)
            elif k == 4:
                v = float(rng.uniform(0.01, 0.2))
                lib.SetRXAPreGenNoiseMag(1, D(v)); g.SetNoiseMag(v)
            elif k == 5:
                v = float(rng.uniform(0.05, 0.8))
                lib.SetRXAPreGenSweepMag(1, D(v)); g.SetSweepMag(v)
            elif k == 6:
                f1 = float(rng.uniform(-4000.0, 0.0)); f2 = f1 + float(rng.uniform(500.0, 6000.0))
                lib.SetRXAPreGenSweepFreq(1, D(f1), D(f2)); g.SetSweepFreq(f1, f2)
            elif k == 7:
                v = float(rng.uniform(50000.0, 900000.0))
                lib.SetRXAPreGenSweepRate(1, D(v)); g.SetSweepRate(v)
            elif k == 8:
                m = int(rng.choice(list(MODES)))
                lib.SetRXAMode(1, m); r.SetRXAMode(m)
                lib.RXASetPassband(1, D(MODES[m][0]), D(MODES[m][1])); r.RXASetPassband(*MODES[m])
            else:
                lo = float(rng.uniform(200.0, 600.0)); hi = lo + float(rng.uniform(1500.0, 3000.0))
                lib.RXASetPassband(1, D(lo), D(hi)); r.RXASetPassband(lo, hi)
            assert lib.qh_wdsp_status() == 0, lib.qh_last_error()
            nb = int(rng.choice([1, 3, 5, 7]))
            ys.append(_blocks(lib, 1, nb))
            if not g.run:
                x = np.zeros(nb * SIZE, dtype=np.complex128)
            elif g.mode == 2:
                x = noise(default_seed(0), 0, drawn, nb * SIZE, g.noise_mag)
                drawn += nb * SIZE
            else:
                x = g.blocks(nb)
            refs.append(r.xrxa(x))
        y, ref = np.concatenate(ys), np.concatenate(refs)
        lat = _latency(y)
        err = rel_rms(y[lat:], ref[:ref.size - lat])
        print("seed %d: %d samples, latency %d, rel rms %.3g, peak %.3g" % (seed, y.size, lat, err, np.abs(ref).max()))
        assert np.abs(ref).max() > 1e-2 and err < 1e-6
    finally:
        lib.CloseChannel(1); r.close()
