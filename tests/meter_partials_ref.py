"""The fused meters' partial scheme (quisk_amd/csrc/qh_osfir.hpp "fused meters", qh_demod.hpp meter_finish_kernel) restated in
numpy, lane by lane, and xmeter (wdsp/meter.c:75-108) sample by sample to hold it against.

A tile of `lout` new samples is held by `nts` lanes with `regs` registers each: lane t, register i holds sample
rel = t + nts i - j0 of the tile (j0 the pre-roll; j0 + lout = nts regs, the transform's length).  Every row of 16 lanes
leaves one (sum, max) per tile; the finish carries them to the call's end and joins them with the carried state."""
import numpy as np


def xmeter(mag2, size, m, mp, avg=0.0, peak=0.0):
    """The running average and the decaying block peak after the blocks of `size` samples in mag2 (|z|^2), one sample at a time."""
    assert len(mag2) % size == 0
    for b in range(len(mag2) // size):
        blk_max = 0.0
        for v in mag2[b * size:(b + 1) * size]:
            avg = avg * m + (1.0 - m) * v
            blk_max = max(blk_max, v)
        peak = max(peak * mp ** size, blk_max)
    return avg, peak


def tile_partials(mag2, size, m, mp, lout, j0, nts=256):
    """[tile][row of 16 lanes] (sum, max) of a call's squared magnitudes."""
    n = len(mag2)
    span = j0 + lout
    assert span % nts == 0 and nts % 64 == 0
    regs = span // nts
    ntiles = (n + lout - 1) // lout
    t = np.arange(nts)
    wlane = (1.0 - m) * m ** (nts - 1.0 - t)                # the last register's sample lies nts - 1 - t short of the tile's end
    mnt = m ** nts
    pk = mp ** (size * np.arange(lout // size + 2.0))       # the host's table
    out = np.zeros((ntiles, nts // 16, 2))
    for T in range(ntiles):
        bT = ((T + 1) * lout - 1) // size
        h = np.zeros(nts)
        mx = np.zeros(nts)
        first = j0 // nts                                   # the first register that can hold a valid sample
        for i in range(first, regs):
            rel = t + nts * i - j0
            g = T * lout + rel
            ok = (rel >= 0) & (rel < lout) & (g < n)
            v = np.where(ok, mag2[np.clip(g, 0, n - 1)], 0.0)
            h = h * mnt + v
            k = bT - np.clip(g, 0, None) // size
            mx = np.maximum(mx, v * pk[np.where(ok, k, 0)])
        out[T, :, 0] = (h * wlane).reshape(-1, 16).sum(axis=1)
        out[T, :, 1] = mx.reshape(-1, 16).max(axis=1)
    return out


def finish(part, n, size, m, mp, lout, avg=0.0, peak=0.0):
    """The meters at the call's end from a call's partials and the state carried in."""
    nblocks = n // size
    a, p = 0.0, 0.0
    for T in range(part.shape[0]):
        end = (T + 1) * lout                                # negative exponents for a last tile the call's end cuts short
        wa = m ** float(n - end)
        wp = mp ** float(size * (nblocks - 1 - (end - 1) // size))
        a += wa * part[T, :, 0].sum()
        p = max(p, wp * part[T, :, 1].max())
    return avg * m ** float(n) + a, max(peak * mp ** float(n), p)
