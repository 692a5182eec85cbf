"""SetRXAPanelPan and SetRXAPanelBinaural (wdsp/patchpanel.c:158-192) against the setters whose fields they write, SetRXAPanelGain2 and
SetRXAPanelCopy: 3 channels, dsp_size 64, 48 kHz at all three rates, five ragged calls (6400 samples).  Pan 0 and 0.5 give the gains 1, 0
and 1, 1 exactly, so those are bit-equal; at 0.25 and 0.8 the gain is sin(pan PI) and numpy's sine is the reference: the outputs agree to
1e-15 relative per part (the two sines may differ in their last place, 1.1e-16, and the output is that gain times a sample).  -m gpu."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu
RATE, SIZE, NCH = 48000, 64, 3
BLOCKS = (1, 40, 7, 33, 19)
N = sum(BLOCKS) * SIZE
PI = 3.1415926535897932                 # wdsp/comm.h:146


def signal():
    rng = np.random.default_rng(11)
    t = np.arange(N) / float(RATE)
    x = 0.1 * (rng.standard_normal((NCH, N)) + 1j * rng.standard_normal((NCH, N)))
    for c in range(NCH):
        x[c] += np.exp(-2j * np.pi * (900.0 + 300.0 * c) * t)
    return x


def run(qh, setup, between=None):
    """a fresh engine (USB, fixed AGC gain), `setup(e)` ahead of the first call, `between(e)` ahead of the third"""
    e = qh.RxaEngine(NCH, dsp_size=SIZE, in_rate=RATE, dsp_rate=RATE, out_rate=RATE)
    try:
        e.SetRXAShiftRun(-1, 0)
        e.SetRXAMode(-1, 1)
        e.RXASetPassband(-1, 300.0, 3000.0)
        e.SetRXAAGCMode(-1, 0)
        e.SetRXAAGCFixed(-1, 6.0)
        setup(e)
        x, out, pos = signal(), [], 0
        for j, nb in enumerate(BLOCKS):
            if j == 2 and between:
                between(e)
            out.append(e.process_host(np.ascontiguousarray(x[:, pos:pos + nb * SIZE])))
            pos += nb * SIZE
        return np.concatenate(out, axis=1)
    finally:
        e.close()


@pytest.mark.parametrize("pan, gains", [(0.0, (1.0, 0.0)), (0.5, (1.0, 1.0))])
def test_pan_at_the_ends_is_gain2_bit_for_bit(qh, pan, gains):
    a = run(qh, lambda e: e.SetRXAPanelPan(-1, pan))
    b = run(qh, lambda e: e.SetRXAPanelGain2(-1, *gains))
    assert np.abs(b.real).max() > 0.5
    assert np.array_equal(a, b)


@pytest.mark.parametrize("pan", [0.25, 0.8])
def test_pan_follows_the_sine_law(qh, pan):
    s = float(np.sin(pan * PI))
    gains = (1.0, s) if pan <= 0.5 else (s, 1.0)
    a = run(qh, lambda e: e.SetRXAPanelPan(-1, pan))
    b = run(qh, lambda e: e.SetRXAPanelGain2(-1, *gains))
    plain = run(qh, lambda e: None)
    assert np.abs(b.real).max() > 0.5 and np.abs(b.imag).max() > 0.5
    for part in ("real", "imag"):
        pa, pb = getattr(a, part), getattr(b, part)
        worst = float(np.max(np.abs(pa - pb) / np.maximum(np.abs(pb), 1e-300)))
        print("pan %g %s: worst relative %.3e" % (pan, part, worst))
        assert np.all(np.abs(pa - pb) <= 1e-15 * np.abs(pb))
    # the panned side is quieter than the unpanned chain's, the other side is its own
    quiet, full = ("imag", "real") if pan <= 0.5 else ("real", "imag")
    assert np.array_equal(getattr(a, full), getattr(plain, full))
    assert np.allclose(getattr(a, quiet), s * getattr(plain, quiet), rtol=1e-14, atol=0.0)


def test_pan_of_one_channel_leaves_the_others(qh):
    a = run(qh, lambda e: e.SetRXAPanelPan(1, 0.8))
    plain = run(qh, lambda e: None)
    assert np.array_equal(a[0], plain[0]) and np.array_equal(a[2], plain[2])
    assert not np.array_equal(a[1], plain[1])


@pytest.mark.parametrize("bin_, copy", [(0, 1), (1, 0)])
def test_binaural_is_copy(qh, bin_, copy):
    a = run(qh, lambda e: e.SetRXAPanelBinaural(-1, bin_))
    b = run(qh, lambda e: e.SetRXAPanelCopy(-1, copy))
    assert np.abs(b).max() > 0.5
    assert np.array_equal(a, b)
    if copy == 1:
        assert np.array_equal(a.real, a.imag)           # copy 1: I to both sides


def test_the_last_writer_wins(qh):
    """pan and Gain2 write the same two fields, binaural and copy the same one: set one ahead of the first call and the other between the
    calls, either way round"""
    ends = sum(BLOCKS[:2]) * SIZE
    pan = run(qh, lambda e: e.SetRXAPanelPan(-1, 0.8))
    g2 = run(qh, lambda e: e.SetRXAPanelGain2(-1, 0.3, 0.9))
    a = run(qh, lambda e: e.SetRXAPanelGain2(-1, 0.3, 0.9), lambda e: e.SetRXAPanelPan(-1, 0.8))
    assert np.array_equal(a[:, :ends], g2[:, :ends]) and np.array_equal(a[:, ends:], pan[:, ends:])
    b = run(qh, lambda e: e.SetRXAPanelPan(-1, 0.8), lambda e: e.SetRXAPanelGain2(-1, 0.3, 0.9))
    assert np.array_equal(b[:, :ends], pan[:, :ends]) and np.array_equal(b[:, ends:], g2[:, ends:])
    # both set ahead of a call: only the later one shows
    c = run(qh, lambda e: (e.SetRXAPanelGain2(-1, 0.3, 0.9), e.SetRXAPanelPan(-1, 0.8)))
    assert np.array_equal(c, pan)
    d = run(qh, lambda e: (e.SetRXAPanelBinaural(-1, 0), e.SetRXAPanelCopy(-1, 0)))
    assert np.array_equal(d, run(qh, lambda e: None))
