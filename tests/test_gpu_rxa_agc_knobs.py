"""SetRXAAGCThresh, SetRXAAGCHangLevel and SetRXAAGCMaxInputLevel (wdsp/wcpAGC.c:449-466,499-511,550-557) on the engine's AGC: mode 3 on a
two-tone input with fades, 2 to 3 channels, dsp_size 64, 48 kHz at all three rates, five ragged calls of 3 to 40 blocks (10240 samples: the
calls cross the 4097-sample seams of the 8192-point tiles twice).

    Thresh          against an engine given SetRXAAGCTop(20 log10 g), g from the Python formula (tests/wdsp_agc_knobs_ref.py): 1e-6 relative RMS
    HangLevel       the level solved in Python from hang_thresh = k / 100, against an engine given SetRXAAGCHangThreshold(k): 1e-6, once the
                    reference alone (oracle/wcpagc_oracle's wo_agc) has shown that hang_thresh one ulp apart moves its output by less than 1e-9
    MaxInputLevel   against wo_agc, max_input set in its field, run on the same pre-AGC samples (the engine's own, AGC at a fixed gain of 1
                    and a unit panel): 1e-9, the bound tests/test_gpu_wcpagc_batch.py holds the engine's AGC to against the oracle
    refusals        a refused value leaves the next call bit-equal to an engine that never saw it
"""
import math

import numpy as np
import pytest

import wdsp_agc_knobs_ref as K
from conftest import rel_rms

gpu = pytest.mark.gpu
RATE, SIZE = 48000, 64
BLOCKS = (3, 40, 37, 40, 40)
N = sum(BLOCKS) * SIZE
BAND = (300.0, 3000.0)
HANG_MS = 20


def two_tone(c):
    """two tones inside the USB band (fir_bandpass's flow .. fhigh passes exp(-2 pi i f t)) under a slow fade, with a dip longer than the
    hang time and a step up.  The fade rises for the first 3800 samples or more and the second tone is weak: when the level first falls,
    the detector's fast average has come up far enough that the fall is no `pop` (wcpAGC.c:225), so the hang decision is taken -- on a
    louder beat the machine would move between attack and fast decay alone and no hang threshold would show."""
    t = np.arange(N) / float(RATE)
    env = 0.2 * (1.0 + 0.1 * np.sin(2.0 * np.pi * (2.5 + 0.3 * c) * t))
    env[8200:8200 + 900] *= 0.05                        # a dip, nearly as long as the hang time
    env[9500:] *= 2.0                                   # a step up
    x = env * (np.exp(-2j * np.pi * (700.0 + 40.0 * c) * t) + 0.15 * np.exp(-2j * np.pi * (1900.0 - 55.0 * c) * t))
    rng = np.random.default_rng(70 + c)
    return x + 1e-5 * (rng.standard_normal(N) + 1j * rng.standard_normal(N))


def engine(qh, nch, agc=True):
    e = qh.RxaEngine(nch, dsp_size=SIZE, in_rate=RATE, dsp_rate=RATE, out_rate=RATE)
    e.SetRXAShiftRun(-1, 0)
    e.SetRXAMode(-1, 1)
    e.RXASetPassband(-1, *BAND)
    if agc:
        e.SetRXAAGCMode(-1, 3)
        e.SetRXAAGCHang(-1, HANG_MS)
    else:                                               # the samples ahead of xwcpagc: a fixed gain of 1 and a unit panel behind them
        e.SetRXAAGCMode(-1, 0)
        e.SetRXAAGCFixed(-1, 0.0)
    e.SetRXAPanelGain1(-1, 1.0)
    return e


def run(e, x):
    out, pos = [], 0
    for nb in BLOCKS:
        out.append(e.process_host(np.ascontiguousarray(x[:, pos:pos + nb * SIZE])))
        pos += nb * SIZE
    return np.concatenate(out, axis=1)


def pre_agc_cpu(oracle, c):
    """the pre-AGC samples of channel c from the oracle's channel (AGC at a fixed gain of 1, unit panel): for the CPU-only check"""
    o = oracle.WdspChannel(SIZE, SIZE, RATE, RATE, RATE)
    o.SetRXAShiftRun(0); o.SetRXAMode(1); o.RXASetPassband(*BAND); o.SetRXAAGCMode(0); o.SetRXAAGCFixed(0.0); o.SetRXAPanelGain1(1.0)
    y = o.xrxa(two_tone(c))
    o.close()
    return y


@pytest.mark.parametrize("k", [55, 80])
def test_the_input_is_not_on_a_knife_edge_of_the_hang_threshold(oracle, k):
    """the reference alone: two runs of wo_agc with hang_thresh one ulp apart agree to 1e-9 (the level SetRXAAGCHangLevel is given comes
    back as a hang_thresh a few ulps from k / 100; if a decision of the state machine hung on that, the comparison below would test
    the input, not the setter)"""
    for c in range(2):
        pre = pre_agc_cpu(oracle, c)
        outs = []
        for ht in (k / 100.0, np.nextafter(k / 100.0, 1.0), np.nextafter(k / 100.0, 0.0)):
            a = K.RxaAgc(oracle, RATE, 3)
            a.set(hangtime=HANG_MS / 1000.0, hang_thresh=float(ht))
            outs.append(a(pre, SIZE))
            a.close()
        assert np.abs(outs[0]).max() > 0.1
        assert rel_rms(outs[1], outs[0]) < 1e-9 and rel_rms(outs[2], outs[0]) < 1e-9
        # and the threshold matters on this input: another k gives another output
        a = K.RxaAgc(oracle, RATE, 3)
        a.set(hangtime=HANG_MS / 1000.0, hang_thresh=1.0)
        assert rel_rms(a(pre, SIZE), outs[0]) > 1e-3
        a.close()


@gpu
@pytest.mark.parametrize("thresh", [-95.0, -120.0])
def test_thresh_is_top_at_the_formulas_gain(qh, thresh):
    nch = 3
    x = np.stack([two_tone(c) for c in range(nch)])
    size, rate = 4096.0, 192000.0
    a, b = engine(qh, nch), engine(qh, nch)
    a.SetRXAAGCThresh(-1, thresh, size, rate)
    g = K.thresh_to_max_gain(thresh, size, rate, band=BAND)
    b.SetRXAAGCTop(-1, 20.0 * math.log10(g))
    ya, yb = run(a, x), run(b, x)
    ref = run(engine(qh, nch), x)                       # create_rxa's max_gain: the knob is seen in the output
    for c in range(nch):
        assert np.abs(yb[c]).max() > 0.1
        print("thresh %g ch %d: rel rms %.3e (moved %.3e)" % (thresh, c, rel_rms(ya[c], yb[c]), rel_rms(ya[c], ref[c])))
        assert rel_rms(ya[c], yb[c]) < 1e-6
        assert rel_rms(ya[c], ref[c]) > 1e-3
    # set between calls: the new gain acts from the next call on, on both engines alike
    a, b = engine(qh, nch), engine(qh, nch)
    n0 = BLOCKS[0] * SIZE + BLOCKS[1] * SIZE
    ya0, yb0 = a.process_host(np.ascontiguousarray(x[:, :n0])), b.process_host(np.ascontiguousarray(x[:, :n0]))
    assert np.array_equal(ya0, yb0)
    a.SetRXAAGCThresh(1, thresh, size, rate)
    b.SetRXAAGCTop(1, 20.0 * math.log10(g))
    ya1, yb1 = a.process_host(np.ascontiguousarray(x[:, n0:])), b.process_host(np.ascontiguousarray(x[:, n0:]))
    for c in range(nch):
        assert rel_rms(ya1[c], yb1[c]) < 1e-6
    assert np.array_equal(ya1[0], yb1[0]) and np.array_equal(ya1[2], yb1[2])


@gpu
@pytest.mark.parametrize("k", [55, 80])
def test_hang_level_is_hang_threshold_at_the_solved_level(qh, k):
    nch = 2
    x = np.stack([two_tone(c) for c in range(nch)])
    a, b = engine(qh, nch), engine(qh, nch)
    level = K.solve_hang_level(k / 100.0)
    assert abs(K.hang_level_to_thresh(level) - k / 100.0) < 1e-14
    a.SetRXAAGCHangLevel(-1, level)
    b.SetRXAAGCHangThreshold(-1, k)
    assert a.GetRXAAGCHangLevel(0) == pytest.approx(b.GetRXAAGCHangLevel(0), abs=1e-12)
    ya, yb = run(a, x), run(b, x)
    ref = run(engine(qh, nch), x)                       # mode 3's hang_thresh of 1
    for c in range(nch):
        print("hang k %d ch %d: rel rms %.3e (moved %.3e)" % (k, c, rel_rms(ya[c], yb[c]), rel_rms(yb[c], ref[c])))
        assert rel_rms(ya[c], yb[c]) < 1e-6
        assert rel_rms(yb[c], ref[c]) > 1e-3


@gpu
@pytest.mark.parametrize("level", [0.05, 0.5])
def test_max_input_level_follows_the_oracles_agc(qh, oracle, level):
    nch = 2
    x = np.stack([two_tone(c) for c in range(nch)])
    pre = run(engine(qh, nch, agc=False), x)
    e = engine(qh, nch)
    e.SetRXAAGCMaxInputLevel(-1, level)
    y = run(e, x)
    plain = run(engine(qh, nch), x)
    for c in range(nch):
        a = K.RxaAgc(oracle, RATE, 3)
        a.set(hangtime=HANG_MS / 1000.0, max_input=level)
        ref = a(pre[c], SIZE)
        a.close()
        assert np.abs(ref).max() > 0.05
        print("max_input %g ch %d: rel rms %.3e (moved %.3e)" % (level, c, rel_rms(y[c], ref), rel_rms(y[c], plain[c])))
        assert rel_rms(y[c], ref) < 1e-9
        assert rel_rms(y[c], plain[c]) > 1e-3


@gpu
def test_a_refused_value_leaves_the_next_call_as_it_was(qh):
    nch = 2
    x = np.stack([two_tone(c) for c in range(nch)])
    a, b = engine(qh, nch), engine(qh, nch)
    for e in (a, b):
        e.SetRXAAGCThresh(-1, -100.0, 4096.0, 192000.0)
        e.SetRXAAGCHangLevel(-1, -30.0)
        e.SetRXAAGCMaxInputLevel(-1, 0.8)
    n0 = (BLOCKS[0] + BLOCKS[1]) * SIZE
    ya, yb = [a.process_host(np.ascontiguousarray(x[:, :n0]))], [b.process_host(np.ascontiguousarray(x[:, :n0]))]
    nan = float("nan")
    for name, args in (("SetRXAAGCThresh", (nan, 4096.0, 192000.0)), ("SetRXAAGCThresh", (-90.0, 0.0, 192000.0)),
                       ("SetRXAAGCThresh", (-90.0, 4096.0, -1.0)), ("SetRXAAGCHangLevel", (nan,)), ("SetRXAAGCMaxInputLevel", (0.0,)),
                       ("SetRXAAGCMaxInputLevel", (-2.0,)), ("SetRXAPanelPan", (nan,))):
        with pytest.raises(qh.QuiskHipError):
            getattr(a, name)(-1, *args)
    ya.append(a.process_host(np.ascontiguousarray(x[:, n0:])))
    yb.append(b.process_host(np.ascontiguousarray(x[:, n0:])))
    assert np.array_equal(np.concatenate(ya, axis=1), np.concatenate(yb, axis=1))
    assert np.abs(ya[1]).max() > 0.1
