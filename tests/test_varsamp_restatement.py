"""tests/wdsp_varsamp_ref.py, the restatement the GPU tests of qh_varsamp_* lean on, pinned on wdsp/varsamp.c's own properties: the sizes
calc_varsamp gives, the reach of hshift into h, the independence of a constant-ratio stream from its cuts, what flush keeps, the cleared
16 bits, both wrap directions of h_offset, and the output counts of one ragged stream.  CPU only."""
import numpy as np
import pytest

from wdsp_varsamp_ref import Varsamp, clear16, run_cuts

PAIRS = [(48000, 48000, 1024), (48000, 96000, 64), (96000, 48000, 64)]


def _x(n, seed=1):
    rng = np.random.default_rng(seed)
    t = np.arange(n)
    return 0.3 * (rng.standard_normal(n) + 1j * rng.standard_normal(n)) + np.exp(2j * np.pi * 0.031 * t)


@pytest.mark.parametrize("in_rate,out_rate,R,rsize", [(48000, 48000, 1024, 140), (48000, 96000, 64, 140), (96000, 48000, 64, 280)])
def test_sizes_and_the_reach_into_h(oracle, in_rate, out_rate, R, rsize):
    v = Varsamp(in_rate, out_rate, R)
    assert v.rsize == rsize and v.ncoef == rsize * R + 1 and len(v.h) == v.ncoef
    assert v.idx_in == rsize - 1 and v.inv_cvar == 1.0 / (float(out_rate) / float(in_rate))
    # h_offset just below 1: hidx = R - 1, and k = hidx + 1 + (rsize - 1) R = ncoef - 1, the last coefficient
    v.h_offset = 1.0 - 2.0 ** -53
    hs = v.hshift()
    assert v.max_k == v.ncoef - 1 and len(hs) == rsize
    v.process(_x(400), 0.97)
    v.process(_x(400), 1.04)
    assert 0 < v.max_k <= v.ncoef - 1
    assert abs(np.sum(v.h) / R - 1.0) < 1e-3                       # unity gain at DC: R * gain over R phases


def test_varmode_0_ragged_cuts_give_the_bits_of_one_call(oracle):
    x = _x(700)
    for var in (1.0003, 0.97):
        a, b = Varsamp(48000, 48000, 64, varmode=0), Varsamp(48000, 48000, 64, varmode=0)
        cuts = [0, 1, 300, 301, 302, 700]
        ya, _, ca = run_cuts(a, x, cuts, [var] * 5)
        yb, _, cb = run_cuts(b, x, [0, 700], [var])
        assert sum(ca) == cb[0] and np.array_equal(ya, yb)
        assert a.state() == b.state()


def test_flush_returns_the_created_state_but_for_inv_cvar(oracle):
    v, fresh = Varsamp(48000, 96000, 64), Varsamp(48000, 96000, 64)
    v.process(_x(333), 1.02)
    inv = v.inv_cvar
    assert inv != fresh.inv_cvar and v.h_offset != 0.0
    v.flush()
    assert (v.h_offset, v.isamps, v.idx_in) == (0.0, 0.0, v.rsize - 1) and not np.any(v.ring)
    assert v.inv_cvar == inv
    # ... and from there the stream is that of a new resampler that starts from this inv_cvar
    fresh.inv_cvar = inv
    x = _x(200, seed=4)
    ya, _ = v.process(x, 1.01)
    yb, _ = fresh.process(x, 1.01)
    assert np.array_equal(ya, yb)


def test_the_low_16_bits_are_cleared_after_every_step(oracle):
    assert np.array([clear16(1.0 / 1.0003)]).view(np.uint64)[0] & np.uint64(0xffff) == 0
    assert clear16(1.0) == 1.0 and 0.0 <= 1.0 / 1.0003 - clear16(1.0 / 1.0003) < 2.0 ** -36
    for varmode in (0, 1):
        v = Varsamp(48000, 48000, 64, varmode=varmode)
        for k, var in enumerate((1.0003, 0.99, 1.01)):
            for i in range(5):                          # one-sample calls: the state after every step
                v.process(_x(1, seed=i), var)
                assert np.array([v.inv_cvar]).view(np.uint64)[0] & np.uint64(0xffff) == 0
                assert v.delta == 1.0 - v.inv_cvar


def test_h_offset_wraps_both_ways(oracle):
    up, down = Varsamp(48000, 48000, 64, varmode=0), Varsamp(48000, 48000, 64, varmode=0)
    up.process(_x(300), 1.04)               # inv_cvar < 1: delta > 0, h_offset climbs through 1
    down.process(_x(300), 0.96)             # inv_cvar > 1: delta < 0, the first step leaves 0 downwards
    hu, hd = np.array(up.rec_h), np.array(down.rec_h)
    assert np.all((hu >= 0.0) & (hu < 1.0)) and np.all((hd >= 0.0) & (hd < 1.0))
    assert np.count_nonzero(np.diff(hu) < 0) >= 5 and np.count_nonzero(np.diff(hd) > 0) >= 5
    assert hu[1] > hu[0] == 0.0 and hd[1] > 0.9


@pytest.mark.parametrize("pair,want", list(zip(PAIRS, [[1, 301, 1, 393], [2, 601, 2, 786], [1, 150, 1, 196]])))
def test_counts_of_a_ragged_stream(oracle, pair, want):
    v = Varsamp(*pair, var=1.0, varmode=1)
    _, _, counts = run_cuts(v, _x(700), [0, 1, 300, 301, 700], [1.0, 1.01, 0.97, 1.0003])
    print("varsamp counts %s: %s" % (pair, counts))
    assert counts == want
