"""The fused meters' partials (one per row of 16 lanes) and finish weights (tests/meter_partials_ref.py, a numpy restatement of the kernels'
arithmetic) against a sample-by-sample xmeter: both recurrences are linear, so the factorisation is exact up to rounding.  No GPU."""
import numpy as np
import pytest

import meter_partials_ref as mref

RATE = 48000.0
M = float(np.exp(-1.0 / (RATE * 0.100)))        # create_meter: tau 0.1 s for the average and the peak (wdsp/RXA.c:69-82)
TILES = [(884, 140), (2048, 2048)]              # (new samples, pre-roll): the front tile's 1024-point inverse, the band tile


def _signal(n, seed):
    rng = np.random.default_rng(seed)
    z = rng.standard_normal(n) + 1j * rng.standard_normal(n)
    z *= 1.0 + 0.9 * np.sin(np.arange(n) * 2.0 * np.pi / 1777.0)     # a level that moves across tiles
    return np.abs(z) ** 2


def _close(got, want):
    return abs(got - want) <= 1e-12 * abs(want)


@pytest.mark.parametrize("lout,j0", TILES)
@pytest.mark.parametrize("size", [64, 256, 1024])
@pytest.mark.parametrize("nblk", [1, 3, 9])
def test_partials_match_xmeter_with_carried_state(size, lout, j0, nblk):
    """Calls of one block, of a few and of many (ends inside the first tile, inside a later one), the second and third call from
    the state the one before left."""
    avg = peak = ravg = rpeak = 0.0
    for call in range(3):
        n = nblk * size
        mag2 = _signal(n, 100 * call + nblk)
        part = mref.tile_partials(mag2, size, M, M, lout, j0)
        assert part.shape == ((n + lout - 1) // lout, 16, 2)
        avg, peak = mref.finish(part, n, size, M, M, lout, avg, peak)
        ravg, rpeak = mref.xmeter(mag2, size, M, M, ravg, rpeak)
        assert _close(avg, ravg) and _close(peak, rpeak), (call, avg, ravg, peak, rpeak)


@pytest.mark.parametrize("lout,j0", TILES)
@pytest.mark.parametrize("size", [64, 256, 1024])
def test_a_burst_decays_across_tile_seams(size, lout, j0):
    """One loud sample -- first block, last sample of a call, either side of a tile seam -- then quiet: the peak read at the end is
    the burst's block maximum decayed block by block."""
    n = 8 * 1024
    for at in (3, n - 1, lout - 1, lout, 2 * lout + 1):
        mag2 = np.full(n, 1e-6)
        mag2[at] = 4.0
        part = mref.tile_partials(mag2, size, M, M, lout, j0)
        avg, peak = mref.finish(part, n, size, M, M, lout)
        ravg, rpeak = mref.xmeter(mag2, size, M, M)
        assert _close(avg, ravg) and _close(peak, rpeak), (at, avg, ravg, peak, rpeak)
        assert _close(rpeak, 4.0 * M ** float(size * (n // size - 1 - at // size)))
        quiet = np.full(2 * size, 1e-6)
        avg, peak = mref.finish(mref.tile_partials(quiet, size, M, M, lout, j0), len(quiet), size, M, M, lout, avg, peak)
        ravg, rpeak = mref.xmeter(quiet, size, M, M, ravg, rpeak)
        assert _close(avg, ravg) and _close(peak, rpeak)


def test_wider_tiles_and_another_peak_decay():
    """384 lanes on a 6144-point tile (4096 new samples), and a peak decay unlike the average's."""
    size, n = 256, 5 * 4096 + 3 * 256
    mag2 = _signal(n, 7)
    mp = float(np.exp(-1.0 / (RATE * 0.020)))
    part = mref.tile_partials(mag2, size, M, mp, 4096, 2048, nts=384)
    assert part.shape == (6, 24, 2)
    avg, peak = mref.finish(part, n, size, M, mp, 4096, 0.25, 9.0)
    ravg, rpeak = mref.xmeter(mag2, size, M, mp, 0.25, 9.0)
    assert _close(avg, ravg) and _close(peak, rpeak)
