"""gen0 in front of the whole chain, by an identity: in an engine with in rate = dsp rate and the shift off, xshift and xresample copy, so
the GPU chain with gen0 running and ANY input must equal the whole-chain reference (tests/rxa_chain_ref.py, which has no gen0) fed the
restatement's signal (tests/wdsp_gen_ref.py) as its input.  Every stage behind the generator -- the adc meter, nbp0, the S meter, the
detectors, the squelch, the AGC -- then reads the generated signal or the identity fails.  -m gpu.

Bounds, those of the stages' own tests: 1e-9 relative RMS for the filter-only chains (test_gpu_rxa_parity.py), 1e-6 for the FM detector
behind its settling time, the AM squelch and the AGC's state machine (the setter walks' gate), 0.002 dB for the meters."""
import numpy as np
import pytest

from conftest import rel_rms
from rxa_chain_ref import RxaChainRef
from rxa_gen_util import RATE
from wdsp_gen_ref import Gen, default_seed, noise

pytestmark = pytest.mark.gpu
USB, FM, AM = 1, 5, 6
SIZE = 256
CALLS = (1, 3, 5, 7, 9, 11, 4)              # 40 blocks


def _setup(obj, pre, mode, passband):
    obj.SetRXAShiftRun(*pre, 0)
    obj.RXANBPSetRun(*pre, 1)
    obj.SetRXAMode(*pre, mode)
    obj.RXASetPassband(*pre, *passband)
    obj.SetRXAAGCMode(*pre, 0); obj.SetRXAAGCFixed(*pre, 0.0)


def _pair(qh, mode, passband, in_rate=RATE):
    e = qh.RxaEngine(2, dsp_size=SIZE, in_rate=in_rate, dsp_rate=RATE, out_rate=RATE)
    r = RxaChainRef(in_size=SIZE, dsp_size=SIZE, in_rate=RATE, dsp_rate=RATE, out_rate=RATE)
    _setup(e, (-1,), mode, passband)
    _setup(r, (), mode, passband)
    return e, r


def _any_input(e, nblk, seed):
    rng = np.random.default_rng(seed)
    return (rng.standard_normal((e.nch, nblk * e.dsp_insize)) + 1j * rng.standard_normal((e.nch, nblk * e.dsp_insize))) * 0.3


def _walk(e, calls, seed=1):
    return np.concatenate([e.process_host(_any_input(e, nb, seed + k)) for k, nb in enumerate(calls)], axis=1)


def test_tone_into_usb_with_the_meters(qh):
    """700 Hz at 0.5 through nbp0 and bp1 (SetRXABandpassRun), adc / S / agc meters against the reference's"""
    e, r = _pair(qh, USB, (300.0, 3000.0))
    g = Gen(RATE, SIZE, run=1, mode=0)
    try:
        e.SetRXABandpassRun(-1, 1); r.SetRXABandpassRun(1)
        e.enable_meters(True)
        e.SetRXAPreGenMode(0, 0); e.SetRXAPreGenToneMag(0, 0.5); e.SetRXAPreGenToneFreq(0, 700.0); e.SetRXAPreGenRun(0, 1)
        g.SetToneMag(0.5); g.SetToneFreq(700.0)
        y = _walk(e, CALLS)
        ref = r.xrxa(g.blocks(sum(CALLS)))
        err = rel_rms(y[0], ref)
        print("tone into USB: rel rms %.3g" % err)
        assert np.abs(ref).max() > 0.1 and err < 1e-9
        for mt in (0, 1, 2, 3, 5, 6):
            d = abs(e.GetRXAMeter(0, mt) - r.GetRXAMeter(mt))
            print("meter %d: %.3g dB off" % (mt, d))
            assert d < 0.002, mt
    finally:
        e.close(); r.close()


def test_pulse_into_am_with_the_am_squelch(qh):
    """the keyed 1 kHz tone is a carrier to the AM detector and the squelch opens on it: 561 blocks of the first OFF run in one call, then
    the rising edge and ON over ragged calls"""
    e, r = _pair(qh, AM, (-4000.0, 4000.0))
    g = Gen(RATE, SIZE, run=1, mode=6)
    try:
        e.SetRXAAMSQRun(-1, 1); r.SetRXAAMSQRun(1)
        e.SetRXAPreGenMode(0, 6); e.SetRXAPreGenRun(0, 1)
        calls = (561, 1, 3, 5, 7, 9, 11, 24)
        y = _walk(e, calls)[0]
        ref = r.xrxa(g.blocks(sum(calls)))
        err = rel_rms(y, ref)
        print("pulse into AM + AMSQ: rel rms %.3g, peak %.3g" % (err, np.abs(ref).max()))
        assert np.abs(ref).max() > 1e-3 and err < 1e-6
    finally:
        e.close(); r.close()


def test_sweep_into_fm(qh):
    """-3 kHz to +3 kHz at 30 kHz/s (a period of 9600 samples) inside the FM channel's passband; compared behind the detector's settling
    time as its own tests do"""
    e, r = _pair(qh, FM, (-8000.0, 8000.0))
    g = Gen(RATE, SIZE, run=1, mode=3)
    try:
        e.SetRXAPreGenMode(0, 3); e.SetRXAPreGenSweepMag(0, 0.3); e.SetRXAPreGenSweepFreq(0, -3000.0, 3000.0); e.SetRXAPreGenSweepRate(0, 30000.0)
        e.SetRXAPreGenRun(0, 1)
        g.SetSweepMag(0.3); g.SetSweepFreq(-3000.0, 3000.0); g.SetSweepRate(30000.0)
        calls = (1, 3, 5, 150, 41)
        y = _walk(e, calls)[0]
        ref = r.xrxa(g.blocks(sum(calls)))
        lo = 150 * SIZE
        err = rel_rms(y[lo:], ref[lo:])
        print("sweep into FM: rel rms %.3g behind %d blocks" % (err, 150))
        assert np.abs(ref[lo:]).max() > 1e-3 and err < 1e-6
    finally:
        e.close(); r.close()


def test_noise_into_usb_with_the_agc_running(qh):
    """this project's generator restated on the host is the reference's input; AGC mode 3 (medium)"""
    e, r = _pair(qh, USB, (300.0, 3000.0))
    try:
        e.SetRXAAGCMode(-1, 3); r.SetRXAAGCMode(3)
        e.SetRXAPreGenNoiseMag(1, 0.05); e.SetRXAPreGenRun(1, 1)          # mode 2 is the default
        y = _walk(e, CALLS)[1]
        ref = r.xrxa(noise(default_seed(1), 1, 0, sum(CALLS) * SIZE, 0.05))
        err = rel_rms(y, ref)
        print("noise into USB with AGC 3: rel rms %.3g" % err)
        assert np.abs(ref).max() > 1e-3 and err < 1e-6
    finally:
        e.close(); r.close()


def test_an_engine_at_192k_gives_the_equal_rate_engines_output(qh):
    """the chain behind gen0 is the same in both.  Bound: the largest difference DESIGN.md records between two forms of one tile path,
    1.9e-14 of the peak, times five: 1e-13 (measured: printed)."""
    outs = []
    for in_rate in (RATE, 192000):
        e = qh.RxaEngine(2, dsp_size=SIZE, in_rate=in_rate, dsp_rate=RATE, out_rate=RATE)
        try:
            _setup(e, (-1,), USB, (300.0, 3000.0))
            e.SetRXAShiftRun(-1, 1); e.SetRXAShiftFreq(-1, 11000.0)
            e.SetRXAPreGenMode(-1, 1); e.SetRXAPreGenRun(-1, 1)
            outs.append(_walk(e, CALLS))
        finally:
            e.close()
    d = np.abs(outs[0] - outs[1]).max() / np.abs(outs[0]).max()
    print("192k engine against the equal-rate engine: %.3g of the peak" % d)
    assert np.abs(outs[0]).max() > 0.1 and d <= 1e-13


def test_the_input_does_not_reach_the_output_and_the_front_stage_keeps_running(qh, oracle):
    """gen0 running: zeros, random samples and NaN / Inf in give the same bits.  Switched off again, the channel continues from the
    front stage's state as the reference's would -- xshift and xresample ran all along (RXA.c:563-565) -- so the engine's output behind
    the switch is the oracle's over the whole input, generator and all."""
    modes_in = 192000
    nb_gen, nb_after = 6, 12
    rng = np.random.default_rng(7)
    n_in = (nb_gen + nb_after) * 4 * SIZE
    t = np.arange(n_in) / modes_in
    x = 0.2 * np.exp(-2j * np.pi * (((11000.0 + 1000.0) * t) % 1.0)) + 0.01 * (rng.standard_normal(n_in) + 1j * rng.standard_normal(n_in))
    cut = nb_gen * 4 * SIZE
    outs = []
    for kind in ("signal", "zeros", "nan"):
        e = qh.RxaEngine(2, dsp_size=SIZE, in_rate=modes_in, dsp_rate=RATE, out_rate=RATE)
        try:
            _setup(e, (-1,), USB, (300.0, 3000.0))
            e.SetRXAShiftRun(-1, 1); e.SetRXAShiftFreq(-1, 11000.0)
            e.SetRXAPreGenMode(0, 0); e.SetRXAPreGenRun(0, 1)
            head = np.stack([x[:cut], x[:cut]])
            if kind == "zeros":
                head[0] = 0.0
            elif kind == "nan":
                head[0, ::7] = np.nan; head[0, 3::11] = np.inf; head[0, 5::13] = -np.inf
            y = [e.process_host(head)]
            if kind == "signal":
                e.SetRXAPreGenRun(0, 0)
                y.append(e.process_host(np.stack([x[cut:], x[cut:]])))
            outs.append(np.concatenate(y, 1))
        finally:
            e.close()
    n_gen = nb_gen * SIZE
    assert np.all(np.isfinite(outs[2][0]))
    assert np.array_equal(outs[0][0, :n_gen], outs[1][0]) and np.array_equal(outs[0][0, :n_gen], outs[2][0])
    assert np.array_equal(outs[0][1, :n_gen], outs[1][1])                   # the channel beside it read its own input
    o = oracle.WdspChannel(4 * SIZE, SIZE, modes_in, RATE, RATE)
    try:
        _setup(o, (), USB, (300.0, 3000.0))
        o.SetRXAShiftRun(1); o.SetRXAShiftFreq(11000.0)
        ref = o.xrxa(x)
    finally:
        o.close()
    err1 = rel_rms(outs[0][1], ref)
    # channel 0 behind the switch: nbp0's delay line still holds the tone (2047 samples), the front stage's holds the input
    lo = n_gen + 2048
    err0 = rel_rms(outs[0][0, lo:], ref[lo:])
    print("channel 1 against the oracle %.3g; channel 0 behind the switch and nbp0's delay line %.3g" % (err1, err0))
    assert np.abs(ref[lo:]).max() > 0.1 and err1 < 1e-9 and err0 < 1e-9
