"""The AGC's display-side setters and getters (wdsp/wcpAGC.c:440-557) against their formulas written out in Python
(tests/wdsp_agc_knobs_ref.py), on the host's mirror of loadWcpAGC alone: no block is processed.  An engine exists only on a device, so
the file is marked gpu all the same.  -m gpu."""
import math

import pytest

import wdsp_agc_knobs_ref as K

pytestmark = pytest.mark.gpu

SIZE, RATE = 4096.0, 192000.0           # a client's display FFT size and rate


@pytest.fixture()
def eng(qh):
    e = qh.RxaEngine(2, dsp_size=64, in_rate=48000, dsp_rate=48000, out_rate=48000)
    yield e
    e.close()


def test_the_getters_give_create_rxas_values(eng):
    for c in range(2):
        assert eng.GetRXAAGCTop(c) == 20.0 * math.log10(K.MAX_GAIN)
        assert eng.GetRXAAGCHangThreshold(c) == int(100.0 * K.HANG_THRESH)
        assert eng.GetRXAAGCHangLevel(c) == pytest.approx(K.thresh_to_hang_level(K.HANG_THRESH), abs=1e-12)
        assert eng.GetRXAAGCThresh(c, SIZE, RATE) == pytest.approx(K.max_gain_to_thresh(K.MAX_GAIN, SIZE, RATE), abs=1e-12)


@pytest.mark.parametrize("thresh", [-140.0, -100.0, -63.5, 0.0])
def test_thresh_sets_max_gain_by_the_formula_and_comes_back(eng, thresh):
    eng.RXANBPSetFreqs(0, 200.0, 2900.0)
    eng.SetRXAAGCSlope(0, 35)
    var_gain = 10.0 ** (35 / 20.0 / 10.0)
    eng.SetRXAAGCThresh(0, thresh, SIZE, RATE)
    g = K.thresh_to_max_gain(thresh, SIZE, RATE, band=(200.0, 2900.0), var_gain=var_gain)
    assert eng.GetRXAAGCTop(0) == pytest.approx(20.0 * math.log10(g), abs=1e-12)
    assert eng.GetRXAAGCThresh(0, SIZE, RATE) == pytest.approx(thresh, abs=1e-12)
    # the other channel was not touched
    assert eng.GetRXAAGCTop(1) == 20.0 * math.log10(K.MAX_GAIN)


def test_a_later_passband_leaves_max_gain(eng):
    """the reference reads nbp0's edges in SetRXAAGCThresh and does not follow a later RXANBPSetFreqs: max_gain stays, and GetRXAAGCThresh,
    which reads the edges again, moves by the change of the noise offset"""
    eng.RXANBPSetFreqs(-1, 300.0, 3000.0)
    eng.SetRXAAGCThresh(-1, -110.0, SIZE, RATE)
    top = [eng.GetRXAAGCTop(c) for c in range(2)]
    assert top[0] == top[1] == pytest.approx(20.0 * math.log10(K.thresh_to_max_gain(-110.0, SIZE, RATE, band=(300.0, 3000.0))), abs=1e-12)
    eng.RXANBPSetFreqs(0, 300.0, 1650.0)
    eng.RXASetPassband(1, 300.0, 1650.0)
    for c in range(2):
        assert eng.GetRXAAGCTop(c) == top[c]
        assert eng.GetRXAAGCThresh(c, SIZE, RATE) == pytest.approx(-110.0 + 10.0 * math.log10(2.0), abs=1e-12)


@pytest.mark.parametrize("level", [-3.0, -20.0, -47.25, -80.0])
def test_hang_level_first_branch_and_round_trip(eng, level):
    """max_input (1.0) above min_volts: hang_thresh by the logarithm, and GetRXAAGCHangLevel gives the level back"""
    eng.SetRXAAGCTop(0, 90.0)
    mg = 10.0 ** (90.0 / 20.0)
    eng.SetRXAAGCHangLevel(0, level)
    ht = K.hang_level_to_thresh(level, max_gain=mg)
    assert eng.GetRXAAGCHangThreshold(0) == int(100.0 * ht)
    assert eng.GetRXAAGCHangLevel(0) == pytest.approx(K.thresh_to_hang_level(ht, max_gain=mg), abs=1e-12)
    assert eng.GetRXAAGCHangLevel(0) == pytest.approx(level, abs=1e-12)


def test_hang_level_is_clamped_at_1e_minus_8(eng):
    """a level below min_volts: the reference's max(1e-8, ...) gives hang_thresh = 1 + 0.125 log10(1e-8) = 0"""
    eng.SetRXAAGCHangLevel(0, -200.0)
    assert K.hang_level_to_thresh(-200.0) == 0.0
    assert eng.GetRXAAGCHangThreshold(0) == 0
    assert eng.GetRXAAGCHangLevel(0) == pytest.approx(K.thresh_to_hang_level(0.0), abs=1e-12)


def test_hang_level_second_branch(eng):
    """max_input not above min_volts: hang_thresh = 1, whatever the level"""
    mv = K.min_volts()
    eng.SetRXAAGCMaxInputLevel(0, 0.5 * mv)
    eng.SetRXAAGCHangLevel(0, -30.0)
    assert K.hang_level_to_thresh(-30.0, max_input=0.5 * mv) == 1.0
    assert eng.GetRXAAGCHangThreshold(0) == 100
    assert eng.GetRXAAGCHangLevel(0) == pytest.approx(K.thresh_to_hang_level(1.0, max_input=0.5 * mv), abs=1e-12)
    # exactly min_volts is still the second branch (`>`)
    eng.SetRXAAGCHangThreshold(0, 40)
    eng.SetRXAAGCMaxInputLevel(0, mv)
    eng.SetRXAAGCHangLevel(0, -30.0)
    assert eng.GetRXAAGCHangThreshold(0) == 100


def test_the_percent_setter_and_the_level_setter_write_one_field(eng):
    eng.SetRXAAGCHangLevel(0, -12.0)
    eng.SetRXAAGCHangThreshold(0, 37)
    assert eng.GetRXAAGCHangThreshold(0) == 37
    assert eng.GetRXAAGCHangLevel(0) == pytest.approx(K.thresh_to_hang_level(0.37), abs=1e-12)
    eng.SetRXAAGCHangLevel(0, -12.0)
    assert eng.GetRXAAGCHangLevel(0) == pytest.approx(-12.0, abs=1e-12)


def test_max_input_moves_the_hang_level(eng):
    eng.SetRXAAGCMaxInputLevel(-1, 0.25)
    for c in range(2):
        assert eng.GetRXAAGCHangLevel(c) == pytest.approx(K.thresh_to_hang_level(K.HANG_THRESH, max_input=0.25), abs=1e-12)


def test_refused_values_change_nothing(qh, eng):
    eng.SetRXAAGCThresh(-1, -95.0, SIZE, RATE)
    eng.SetRXAAGCHangLevel(-1, -25.0)
    eng.SetRXAAGCMaxInputLevel(-1, 0.75)
    before = [(eng.GetRXAAGCTop(c), eng.GetRXAAGCHangLevel(c), eng.GetRXAAGCHangThreshold(c), eng.GetRXAAGCThresh(c, SIZE, RATE)) for c in range(2)]
    nan, inf = float("nan"), float("inf")
    bad = [("SetRXAAGCThresh", (nan, SIZE, RATE)), ("SetRXAAGCThresh", (-90.0, inf, RATE)), ("SetRXAAGCThresh", (-90.0, SIZE, nan)),
           ("SetRXAAGCThresh", (-90.0, 0.0, RATE)), ("SetRXAAGCThresh", (-90.0, SIZE, 0.0)), ("SetRXAAGCThresh", (-90.0, -4096.0, RATE)),
           ("SetRXAAGCThresh", (-90.0, SIZE, -48000.0)), ("SetRXAAGCHangLevel", (nan,)), ("SetRXAAGCHangLevel", (-inf,)),
           ("SetRXAAGCMaxInputLevel", (0.0,)), ("SetRXAAGCMaxInputLevel", (-1.0,)), ("SetRXAAGCMaxInputLevel", (inf,)),
           ("SetRXAAGCMaxInputLevel", (nan,)), ("SetRXAPanelPan", (nan,)), ("SetRXAPanelPan", (inf,))]
    for name, args in bad:
        for ch in (0, -1):
            with pytest.raises(qh.QuiskHipError):
                getattr(eng, name)(ch, *args)
    for args in ((0.0, RATE), (SIZE, -1.0), (nan, RATE)):
        with pytest.raises(qh.QuiskHipError):
            eng.GetRXAAGCThresh(0, *args)
    after = [(eng.GetRXAAGCTop(c), eng.GetRXAAGCHangLevel(c), eng.GetRXAAGCHangThreshold(c), eng.GetRXAAGCThresh(c, SIZE, RATE)) for c in range(2)]
    assert after == before
    # an nbp0 band that is not wider than 0: the reference would take the log of it.  With -1, one such channel refuses the call for all.
    eng.RXANBPSetFreqs(1, 3000.0, 3000.0)
    for ch in (1, -1):
        with pytest.raises(qh.QuiskHipError):
            eng.SetRXAAGCThresh(ch, -90.0, SIZE, RATE)
    with pytest.raises(qh.QuiskHipError):
        eng.GetRXAAGCThresh(1, SIZE, RATE)
    eng.RXANBPSetFreqs(1, 3000.0, 300.0)
    with pytest.raises(qh.QuiskHipError):
        eng.SetRXAAGCThresh(1, -90.0, SIZE, RATE)
    assert [eng.GetRXAAGCTop(c) for c in range(2)] == [b[0] for b in before]
    eng.SetRXAAGCThresh(0, -90.0, SIZE, RATE)           # the channel with a band takes it
    assert eng.GetRXAAGCTop(0) != before[0][0]
    # a getter wants one channel
    with pytest.raises(qh.QuiskHipError):
        eng.GetRXAAGCTop(-1)
    with pytest.raises(qh.QuiskHipError):
        eng.GetRXAAGCHangLevel(2)
