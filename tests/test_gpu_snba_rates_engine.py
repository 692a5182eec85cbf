"""The engine around xsnba at DSP rates above 48 kHz (the three-pass form of qh_snba.hpp): no channel's blanker reaches another channel,
graph replay, qh_rxa_set_dsp_rate 48 k -> 96 k with the blanker running, what is still refused, and the WDSP names (OpenChannel at
96000 / 256, SetRXASNBARun, fexchange0).  Inputs: snba_rate_cases.py; the two that are compared against the oracle are vetted by
test_snba_rate_inputs.py.  -m gpu."""
import ctypes as C

import numpy as np
import pytest
import torch

from conftest import rel_rms
from quisk_amd import synth
from snba_rate_cases import AFTER_RATE_CHANGE, AM, LSB, NAMES_CASE, USB, Case

pytestmark = pytest.mark.gpu
D = C.c_double


def _same_bits(a, b):
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


def test_a_channel_without_snb_has_the_bits_it_has_with_no_blanker_in_the_engine(qh):
    c = Case((96000, 96000, 96000, 256), (USB, LSB, AM, USB), seconds=0.2)
    x = c.inputs()
    ys = []
    for on in (0, 1):
        e = c.engine(qh, snba=0)
        e.SetRXASNBARun(1, on); e.SetRXASNBARun(3, on)
        ys.append(c.through(e, x))
        e.close()
    assert np.all(np.isfinite(ys[1])) and np.abs(ys[0]).max() > 1e-3
    for ch in (0, 2):
        assert _same_bits(ys[0][ch], ys[1][ch]), ch
    for ch in (1, 3):
        assert rel_rms(ys[1][ch], ys[0][ch]) > 1e-3         # ... while the blanker is really in the other channels' paths


def test_replayed_calls_at_96k_equal_plain_launches(qh):
    c = Case((96000, 96000, 96000, 256), (USB, AM), seconds=0.2)
    x = c.inputs()
    dev = torch.device("cuda:0")
    nb = 60
    ys, launches = [], []
    for replay in (False, True):
        e = c.engine(qh)
        e.set_graph_replay(replay)
        d_in = torch.zeros((c.nch, c.insize), dtype=torch.complex128, device=dev)
        d_out = torch.zeros((c.nch, c.outsize), dtype=torch.complex128, device=dev)
        y = np.zeros((c.nch, nb * c.outsize), dtype=np.complex128)
        for b in range(nb):
            d_in.copy_(torch.from_numpy(x[:, b * c.insize:(b + 1) * c.insize]))
            torch.cuda.synchronize()
            e.process_ptr(d_in.data_ptr(), c.insize, d_out.data_ptr(), c.outsize, 1)
            e.synchronize()
            y[:, b * c.outsize:(b + 1) * c.outsize] = d_out.cpu().numpy()
        ys.append(y); launches.append(e.graph_launches())
        e.close()
    assert launches[0] == 0 and launches[1] >= nb - 5
    assert np.all(np.isfinite(ys[0])) and np.abs(ys[0]).max() > 1e-3
    assert _same_bits(ys[0], ys[1])


def test_a_new_dsp_rate_with_snb_running_is_accepted_and_equals_a_fresh_channel(qh, oracle):
    """48 k -> 96 k on a live engine: both resamplers, the accumulators and the indices are made anew at the new ratio (calc_snba), the
    frame memory stays.  Signal, the change, 0.3 s of silence (448 blocks of 64: a whole number of the blanker's
    frames of 64 samples at 12 kHz, eight blocks each, so that the frames behind it begin where a fresh channel's do), then 0.5 s of
    signal against a fresh oracle channel at 96 k."""
    after = AFTER_RATE_CHANGE
    before = Case((96000, 48000, 48000, 64), (USB,), chans=after.chans, seconds=0.3, shift=False)
    e = before.engine(qh)
    y0 = before.through(e, before.inputs())
    assert np.abs(y0).max() > 1e-3
    e.set_dsp_rate(96000)
    assert (e.in_rate, e.dsp_rate, e.out_rate, e.dsp_size) == after.rates and e.dsp_insize == after.insize
    silence = 448
    assert abs(silence * 64 / 96000.0 - 0.3) < 0.002 and (silence * 64 // 8) % 64 == 0
    e.process_host(np.zeros((1, silence * after.insize), dtype=np.complex128))
    x = after.inputs()
    y = after.through(e, x)
    e.close()
    ref, plain = after.reference(oracle, x), after.reference(oracle, x, snba=0)
    assert rel_rms(ref[0], plain[0]) > 1e-3
    err = rel_rms(y[0], ref[0])
    print("dsp_rate 48000 -> 96000 with SNB running: rel RMS against a fresh channel %.3e" % err)
    assert err < 1e-6, err


def _refused(e, call, *args):
    with pytest.raises(Exception) as info:
        call(*args)
    assert "384000" in str(info.value) and "4096" in str(info.value), str(info.value)       # the message names the accepted set


@pytest.mark.parametrize("rate", [96000, 384000])
def test_what_is_still_refused_changes_nothing(qh, rate):
    """a dsp_rate that is not 12000 x 2^k (k = 0 .. 5), a dsp_size the ratio does not divide or above 4096: calc_snba's integer divisions
    (snb.c:33-36) give them no consistent isize.  (All three rates move together, so that the blanker's check is the one that refuses.)"""
    c = Case((rate, rate, rate, 1024), (USB, AM), seconds=0.12)         # (the blanker alone delays the signal by some 45 ms)
    x = c.inputs()
    half = c.nblk // 2 * c.insize
    a, b = c.engine(qh), c.engine(qh)
    ya, yb = [a.process_host(x[:, :half])], [b.process_host(x[:, :half])]
    state, nbytes = (a.in_rate, a.dsp_rate, a.out_rate, a.dsp_size), a.device_bytes()
    for r in (36000, 768000, 8000):
        _refused(a, a.set_rates, r, r, r)
    if rate == 384000:
        _refused(a, a.set_dsp_size, 16)     # the ratio 32 does not divide it
    with pytest.raises(qh.QuiskHipError):
        a.set_dsp_size(8192)                # (above nc = 2048 as well, and refused for that first: wdsp/nbp.c:308)
    assert (a.in_rate, a.dsp_rate, a.out_rate, a.dsp_size) == state and a.device_bytes() == nbytes
    ya.append(a.process_host(x[:, half:])); yb.append(b.process_host(x[:, half:]))
    a.close(); b.close()
    ya, yb = np.concatenate(ya, axis=1), np.concatenate(yb, axis=1)
    assert np.all(np.isfinite(ya)) and np.abs(ya).max() > 1e-3
    assert _same_bits(ya, yb)


def test_a_dsp_size_above_4096_is_refused_by_the_blanker_itself(qh):
    """with nc = 8192 the filters would take a block of 8192 (wdsp/nbp.c:308), so the refusal and its message are the blanker's"""
    c = Case((96000, 96000, 96000, 1024), (USB,), seconds=0.12)
    x = c.inputs()
    half = c.nblk // 2 * c.insize
    a, b = c.engine(qh), c.engine(qh)
    a.RXASetNC(0, 8192); b.RXASetNC(0, 8192)
    ya, yb = [a.process_host(x[:, :half])], [b.process_host(x[:, :half])]
    state, nbytes = (a.in_rate, a.dsp_rate, a.out_rate, a.dsp_size), a.device_bytes()
    _refused(a, a.set_dsp_size, 8192)
    assert (a.in_rate, a.dsp_rate, a.out_rate, a.dsp_size) == state and a.device_bytes() == nbytes
    ya.append(a.process_host(x[:, half:])); yb.append(b.process_host(x[:, half:]))
    a.close(); b.close()
    ya, yb = np.concatenate(ya, axis=1), np.concatenate(yb, axis=1)
    assert np.all(np.isfinite(ya)) and np.abs(ya).max() > 1e-3
    assert _same_bits(ya, yb)


@pytest.mark.parametrize("size,form", [(256, 0), (256, 1), (2048, 0)])
def test_snb_at_creation_is_refused_where_the_ratio_is_not_a_power_of_two(qh, size, form):
    """... and with SNB switched off again the engine runs on as one that was never asked: an all-SSB engine then takes the linear path,
    which keeps the channel lists of the refused call (form 1 and dsp_size 2048 are where the three passes' rows would be sized)"""
    c = Case((36000, 36000, 36000, size), (USB,), seconds=0.25)
    x = c.inputs()
    e, plain = c.engine(qh, snba=0), c.engine(qh, snba=0)
    e.set_snba_form(form)
    e.SetRXASNBARun(0, 1)
    _refused(e, e.process_host, x[:, :c.insize])
    e.SetRXASNBARun(0, 0)
    y, ref = e.process_host(x), plain.process_host(x)
    e.close(); plain.close()
    assert np.all(np.isfinite(y)) and np.abs(ref).max() > 1e-3
    assert _same_bits(y, ref)


def test_the_wdsp_names_at_96000(qh, oracle):
    """OpenChannel at dsp_rate 96000 / 256, SetRXASNBARun(ch, 1), fexchange0: against the oracle's fexchange0 (latency and slew included)"""
    c = NAMES_CASE
    lib = qh.load()
    x = c.inputs()[0]
    ch = 4
    lib.OpenChannel(ch, c.insize, c.size, c.in_rate, c.dsp_rate, c.out_rate, 0, 1, D(0.010), D(0.025), D(0.0), D(0.010), 1)
    assert lib.qh_wdsp_status() == 0, lib.qh_last_error()
    try:
        lib.SetRXAShiftRun(ch, 1); lib.SetRXAShiftFreq(ch, D(synth.shift_freq(c.chans[0]))); lib.RXANBPSetRun(ch, 1)
        lib.SetRXAMode(ch, USB); lib.RXASetPassband(ch, D(300.0), D(3000.0))
        lib.SetRXAAGCMode(ch, 0); lib.SetRXAAGCFixed(ch, D(6.0))
        lib.SetRXASNBARun(ch, 1)
        assert lib.qh_wdsp_status() == 0, lib.qh_last_error()
        y = np.zeros(c.nblk * c.outsize, dtype=np.complex128)
        err = C.c_int(0)
        for b in range(c.nblk):
            blk = np.ascontiguousarray(x[b * c.insize:(b + 1) * c.insize])
            lib.fexchange0(ch, blk.ctypes.data_as(C.c_void_p), y[b * c.outsize:].ctypes.data_as(C.c_void_p), C.byref(err))
            assert err.value == 0 and lib.qh_wdsp_status() == 0, lib.qh_last_error()
    finally:
        lib.CloseChannel(ch)
    o, p = c.oracle_channel(oracle, 0), c.oracle_channel(oracle, 0, snba=0)
    ref, errs = o.fexchange0(x)
    plain, _ = p.fexchange0(x)
    assert errs == 0 and rel_rms(ref, plain) > 1e-3
    err = rel_rms(y, ref)
    print("the WDSP names at 96000 / 256 with SNB: rel RMS %.3e" % err)
    assert err < 1e-6, err
