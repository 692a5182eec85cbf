"""tests/rxa_fm_filters_ref.py pinned on the CPU (no GPU): the composition that stands in for an xfmd with other filters reproduces the
oracle's own xfmd at the six defaults, the library's fc_impulse is the restated one, and the restated CTCSS notch behaves as a filter
with four state words does."""
import numpy as np
import pytest

import rxa_fm_filters_ref as R
from oracle import pyoracle


@pytest.mark.parametrize("ctcss", [1, 0])
def test_identity_at_the_defaults(oracle, ctcss):
    """32 blocks of 64 samples at 48 kHz, a 1 kHz tone at 3 kHz deviation: the replaced buf equals what the oracle's xfmd left there,
    to 1e-12 of the peak.  Pins the restated fc_impulse, the restated xsnotch and the hook plumbing at once."""
    size, nblk, rate = 64, 32, 48000
    x = R.fm_tone(size * nblk, rate)
    seen = {"own": [], "mine": []}
    o = pyoracle.WdspChannel(size, size, rate, rate, rate)
    o.SetRXAMode(R.FM)
    o.SetRXACTCSSRun(ctcss)
    fm = R.FmFilters(rate, size, ctcss_run=ctcss)

    def hook(where, z, aux):
        seen["own"].append(z.copy())
        z[:] = fm.process(aux)
        seen["mine"].append(z.copy())
    o.set_stage_hook(hook, sites=(pyoracle.WdspChannel.HOOK_FMSQ,))
    o.xrxa(x)
    o.close()
    own, mine = np.concatenate(seen["own"]), np.concatenate(seen["mine"])
    peak = np.max(np.abs(own))
    worst = np.max(np.abs(own - mine)) / peak
    print("ctcss %d: peak %.3e, replaced buf off the oracle's by %.3e of the peak" % (ctcss, peak, worst))
    assert peak > 1e-3
    assert worst <= 1e-12


def test_library_fc_impulse_is_the_restated_one():
    worst = 0.0
    for lo, hi, nc, rate in R.GPU_DESIGNS:
        if 1.1 * hi >= rate / 2:
            continue
        for size in (64, 128):
            args = (nc, lo, hi, +20.0 * np.log10(hi / lo), 0.0, 1, float(rate), 1.0 / (2.0 * size), 0, 0)
            a, b = R.library_fc_impulse(*args), R.fc_impulse(*args)
            d = np.max(np.abs(a - b)) / np.max(np.abs(b))
            worst = max(worst, d)
            assert d <= 1e-12, (lo, hi, nc, rate, size, d)
    print("fc_impulse: library against restatement, worst %.3e of the largest tap over %d designs" % (worst, len(R.GPU_DESIGNS)))


def test_restated_xsnotch_is_block_size_independent_and_flush_zeroes_it():
    r = np.random.default_rng(5)
    z = r.standard_normal(1024) + 1j * r.standard_normal(1024)
    a, b = R.Snotch(1, 48000, 254.1, 0.0002), R.Snotch(1, 48000, 254.1, 0.0002)
    whole = a.process(z)
    parts = np.concatenate([b.process(z[i:i + n]) for i, n in ((0, 64), (64, 1), (65, 447), (512, 512))])
    assert np.array_equal(whole, parts)
    assert np.array_equal(whole.imag, z.imag) and not np.array_equal(whole.real, z.real)
    assert (a.x1, a.x2, a.y1, a.y2) != (0.0, 0.0, 0.0, 0.0)
    a.flush()
    assert (a.x1, a.x2, a.y1, a.y2) == (0.0, 0.0, 0.0, 0.0)
    fresh = R.Snotch(1, 48000, 254.1, 0.0002)
    assert np.array_equal(a.process(z[:64]), fresh.process(z[:64]))
    off = R.Snotch(0, 48000, 254.1, 0.0002)
    assert np.array_equal(off.process(z), z)


def test_a_kept_line_is_the_line():
    """_Line.set_impulse(keep=True) with the SAME impulse changes nothing that follows: the replayed inputs rebuild the delay line"""
    size, rate = 64, 48000
    r = np.random.default_rng(9)
    x = r.standard_normal(size * 80)
    a, b = R.FmFilters(rate, size), R.FmFilters(rate, size)
    ya = np.concatenate([a.process(x[i:i + size]) for i in range(0, x.size, size)])
    yb = []
    for i in range(0, x.size, size):
        if i == size * 50:
            b._design("de", True)
            b._design("aud", True)
        yb.append(b.process(x[i:i + size]))
    yb = np.concatenate(yb)
    d = np.max(np.abs(ya - yb)) / np.max(np.abs(ya))
    print("kept line: %.3e of the peak" % d)
    assert d <= 1e-12
