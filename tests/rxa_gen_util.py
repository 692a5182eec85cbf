"""What the GPU tests of the RXA engine's gen0 share: "the bare chain" (USB with nbp0 and bp1 off, the AGC a fixed gain of 0 dB, the
panel passing I and Q, out rate = dsp rate), on which a channel's output row is its generator's row times the panel's gain1 = 4 -- a
power of two, so dividing it out is exact -- and the comparison against the restatement (tests/wdsp_gen_ref.py).

The bound is the project's fp64 gate, 1e-6 relative RMS, with the largest sample error held to 1e-6 of the largest sample beside it: a
generator that is one sample late is off by sin(delta), 0.09 of a 700 Hz tone at 48 kHz, which an RMS over a long run with one late stretch
could hide and the sample-wise maximum cannot."""
import numpy as np

from conftest import rel_rms
from wdsp_gen_ref import Gen

RATE = 48000
PANEL_GAIN = 4.0            # create_panel's gain1 (RXA.c:464-474)
GATE = 1e-6


def bare(qh, nch, dsp_size=64, in_rate=RATE):
    e = qh.RxaEngine(nch, dsp_size=dsp_size, in_rate=in_rate, dsp_rate=RATE, out_rate=RATE)
    e.SetRXAMode(-1, 1)
    e.RXANBPSetRun(-1, 0)
    e.SetRXAAGCMode(-1, 0); e.SetRXAAGCFixed(-1, 0.0)
    return e


def run(e, nblk, x=None):
    """the generators' rows over one call of nblk blocks (zeros in unless x is given)"""
    if x is None:
        x = np.zeros((e.nch, nblk * e.dsp_insize), dtype=np.complex128)
    return e.process_host(x) / PANEL_GAIN


def runs(e, calls):
    return np.concatenate([run(e, nb) for nb in calls], axis=1)


def ref(dsp_size, mode, setup=None):
    g = Gen(RATE, dsp_size, run=1, mode=mode)
    if setup:
        setup(g)
    return g


def hold(got, want, what):
    """1e-6 relative RMS and 1e-6 of the largest sample, both printed"""
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    r = rel_rms(got, want)
    peak = np.abs(want).max()
    m = np.abs(got - want).max() / peak if peak > 0.0 else np.abs(got).max()
    print("%s: rel rms %.3g, largest sample error %.3g of the peak" % (what, r, m))
    assert r <= GATE and m <= GATE, (what, r, m, int(np.abs(got - want).argmax()))
    return r, m
