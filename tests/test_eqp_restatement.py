"""The equalizer's yardstick checked on the CPU alone, oracle against oracle (no GPU, none of the engine's code).

tests/wdsp_eqp_ref.py restates xeqp as a convolution over a kept delay line.  Held here at 1e-12 relative RMS:
  * against the oracle's fircore (oracle.pyoracle.Fircore) with the same taps from a zero line, block by block;
  * a new design on the kept line: from the block of the change on, the output is that of a fircore which had the new taps all along
    (both see the same input history; setImpulse_fircore leaves the stored spectra alone);
  * a new nc zeroes the line, Run 0 copies and keeps it, flush zeroes it;
  * the identity the GPU tests lean on: with the shift off, equal rates and an SSB chain with a fixed gain, everything in xrxa is linear
    and time-invariant at the dsp rate, so oracle(EQ x) = EQ(oracle x) -- the pre-filter identity read one way, the post-filter identity
    read the other."""
import numpy as np
import pytest

from conftest import rel_rms
from wdsp_eqp_ref import Eqp

TOL = 1e-12
G10 = [3, -12, 12, -6, 9, 0, -12, 12, 4, -9, 7]


def _noise(n, seed=5):
    r = np.random.default_rng(seed)
    return (r.standard_normal(n) + 1j * r.standard_normal(n)) * 0.1


@pytest.mark.parametrize("size,nc,mp", [(256, 2048, 0), (256, 256, 0), (64, 256, 0), (256, 4096, 0), (256, 1024, 1)])
def test_the_convolution_is_the_oracles_fircore(oracle, size, nc, mp):
    e = Eqp(48000, size=size, run=1, nc=nc, mp=mp)
    e.SetRXAGrphEQ10(G10)
    if mp:
        e.SetRXAEQCtfmode(1)
    x = _noise(40 * size)
    want = e.fircore()(x)
    got = np.concatenate([e.process(x[a:b]) for a, b in ((0, size), (size, 4 * size), (4 * size, 13 * size), (13 * size, 40 * size))])
    err = rel_rms(got, want)
    print("size %d nc %d mp %d: %.3g" % (size, nc, mp, err))
    assert err < TOL


def test_a_new_design_acts_on_the_kept_line(oracle):
    e = Eqp(48000, run=1)
    x = _noise(60 * 256, seed=6)
    y0 = e.process(x[:20 * 256])
    e.SetRXAEQProfile(3, [0.0, 400.0, 1500.0, 5000.0], [-2.0, 6.0, -9.0, 3.0])
    y1 = e.process(x[20 * 256:])
    assert rel_rms(y0, Eqp(48000, run=1).fircore()(x[:20 * 256])) < TOL
    assert rel_rms(y1, e.fircore()(x)[20 * 256:]) < TOL


def test_nc_zeroes_the_line_run_0_keeps_it_and_flush_zeroes_it(oracle):
    e = Eqp(48000, run=1)
    e.SetRXAGrphEQ([0, -6, 5, 9])
    x = _noise(50 * 256, seed=7)
    e.process(x[:10 * 256])
    e.SetRXAEQNC(1024)
    assert rel_rms(e.process(x[10 * 256:20 * 256]), e.fircore()(x[10 * 256:20 * 256])) < TOL      # as from a zero line
    e.SetRXAEQRun(0)
    assert np.array_equal(e.process(x[20 * 256:30 * 256]), x[20 * 256:30 * 256])
    e.SetRXAEQRun(1)
    # the line still ends at sample 20 * 256: the output is that of the stream with the skipped blocks cut out
    cut = np.concatenate([x[10 * 256:20 * 256], x[30 * 256:40 * 256]])
    assert rel_rms(e.process(x[30 * 256:40 * 256]), e.fircore()(cut)[10 * 256:]) < TOL
    e.flush()
    assert rel_rms(e.process(x[40 * 256:]), e.fircore()(x[40 * 256:])) < TOL


@pytest.mark.parametrize("bp1", [0, 1])
def test_the_equalizer_commutes_with_the_linear_chain(oracle, bp1):
    """oracle(EQ x) against EQ(oracle x): USB, shift off, 48 kHz throughout, fixed gain, with and without bp1 behind the equalizer's spot"""
    n = 400 * 256
    x = _noise(n, seed=8)

    def chain():
        w = oracle.WdspChannel(256, 256, 48000, 48000, 48000)
        w.SetRXAMode(1); w.SetRXAShiftRun(0); w.RXANBPSetRun(1); w.RXASetPassband(150.0, 4000.0)
        w.SetRXAAGCMode(0); w.SetRXAAGCFixed(10.0); w.SetRXABandpassRun(bp1)
        return w

    def eq():
        e = Eqp(48000, run=1)
        e.SetRXAGrphEQ10(G10)
        return e

    a, b = chain(), chain()
    pre = a.xrxa(eq().process(x))
    post = eq().process(b.xrxa(x))
    a.close(); b.close()
    err = rel_rms(pre, post)
    print("oracle(EQ x) against EQ(oracle x), bp1 %d: %.3g" % (bp1, err))
    assert err < TOL
