"""channel.c's run-time setters under their WDSP names (wdsp/channel.c:158-258,301-347), driven through fexchange0 with host pointers and
through qh_wdsp_fexchange0_device, against the oracle: a fresh wo_open + wo_fexchange0 where the reference starts the channel's DSP from
zero (SetDSPSamplerate, SetDSPBuffsize after silence: the up-slew is armed again), and wdsp_iobuffs_ref.Iobuffs made anew at the change
around the oracle composition that goes on (tests/test_gpu_rxa_rates.py) where it does not (SetInputSamplerate, SetOutputSamplerate,
SetInputBuffsize, SetAllRates with the DSP rate unchanged: nothing is armed).  Gate: relative RMS <= 1e-6.  -m gpu.

The device entry point is Quisk's hand-off (quisk_wdsp.c:24-69): it re-blocks through the shim's in_size, scales by 1 / CLIP32 and back and
returns as many samples as it took, so it is driven where out_size = in_size and the shim is given the channel's in_size."""
import ctypes as C

import numpy as np
import pytest
import torch

from conftest import rel_rms
from wdsp_iobuffs_ref import Iobuffs

pytestmark = pytest.mark.gpu
D = C.c_double
GATE, CLIP32 = 1e-6, 2147483647.0
SLEWS = dict(tdelayup=0.002, tslewup=0.005, tdelaydown=0.0, tslewdown=0.003)
CH = 6


def signal(n, seed, fs=48000.0):
    t = np.arange(n) / fs
    g = np.random.default_rng(seed).standard_normal((n, 2))
    return 0.1 * np.exp(-2j * np.pi * 1000.0 * t) + 0.01 * (g[:, 0] + 1j * g[:, 1])


def settle(t, ch=None):
    lead = [] if ch is None else [ch]
    t.SetRXAMode(*lead, 1)
    t.RXASetPassband(*lead, D(300.0) if ch is not None else 300.0, D(3000.0) if ch is not None else 3000.0)
    t.SetRXAAGCMode(*lead, 3)


def open_channel(lib, in_size, dsp_size, rates, state=1, slews=SLEWS):
    lib.OpenChannel(CH, in_size, dsp_size, rates[0], rates[1], rates[2], 0, state, D(slews["tdelayup"]), D(slews["tslewup"]), D(slews["tdelaydown"]),
                    D(slews["tslewdown"]), 1)
    assert lib.qh_wdsp_status() == 0, lib.qh_last_error()
    settle(lib, CH)
    assert lib.qh_wdsp_status() == 0, lib.qh_last_error()


class Host:
    def __init__(self, lib, in_size):
        self.lib = lib

    def resize(self, in_size):
        pass

    def __call__(self, blk, out_size):
        """one fexchange0: the out_size samples it wrote, or None when it wrote nothing; 8 more samples must stay untouched"""
        out = np.full(out_size + 8, np.nan + 0j, dtype=np.complex128)
        err = C.c_int(0)
        blk = np.ascontiguousarray(blk)
        self.lib.fexchange0(CH, blk.ctypes.data_as(C.c_void_p), out.ctypes.data_as(C.c_void_p), C.byref(err))
        assert err.value == 0 and np.all(np.isnan(out[out_size:])), "fexchange0 wrote more than out_size samples"
        return None if np.all(np.isnan(out[:out_size])) else out[:out_size].copy()

    def close(self):
        pass


class Dev:
    def __init__(self, lib, in_size):
        self.lib, self.dev, self.stream = lib, torch.device("cuda:0"), torch.cuda.Stream()
        lib.qh_wdsp_set_parameter(CH, in_size, 1)

    def resize(self, in_size):
        self.lib.qh_wdsp_set_parameter(CH, in_size, 1)

    def __call__(self, blk, out_size):
        assert out_size == blk.size
        with torch.cuda.stream(self.stream):
            work = torch.zeros(3 * blk.size, dtype=torch.complex128, device=self.dev)
            work[:blk.size] = torch.from_numpy(blk * CLIP32).to(self.dev)
            n = self.lib.qh_wdsp_fexchange0_device(CH, C.c_void_p(work.data_ptr()), blk.size, C.c_void_p(self.stream.cuda_stream))
            assert self.lib.qh_wdsp_status() == 0, self.lib.qh_last_error()
            out = work[:n].cpu()
        self.stream.synchronize()
        assert n == blk.size
        return out.numpy() / CLIP32

    def close(self):
        self.lib.qh_wdsp_set_parameter(CH, 0, 0)


def feed(drive, x, in_size, out_size):
    return np.concatenate([drive(x[b * in_size:(b + 1) * in_size], out_size) for b in range(x.size // in_size)])


@pytest.mark.parametrize("drive_t", [Host, Dev], ids=["host", "device"])
@pytest.mark.parametrize("what", ["dsp_rate", "dsp_size"])
def test_dsp_rate_and_size_after_silence_start_the_channel_afresh_with_its_up_slew(qh, oracle, what, drive_t):
    lib = qh.load()
    x1, x2 = signal(64 * 40, 1), signal(64 * 90, 2)
    open_channel(lib, 64, 64, (48000, 48000, 48000))
    drive = drive_t(lib, 64)
    try:
        feed(drive, x1, 64, 64)
        feed(drive, np.zeros(64 * 40, dtype=np.complex128), 64, 64)        # nc = 2048 samples and the slack of the rings
        if what == "dsp_rate":
            lib.SetDSPSamplerate(CH, 96000)
        else:
            lib.SetDSPBuffsize(CH, 128)
        assert lib.qh_wdsp_status() == 0, lib.qh_last_error()
        y = feed(drive, x2, 64, 64)
    finally:
        drive.close()
        lib.CloseChannel(CH)
    o = oracle.WdspChannel(64, 128 if what == "dsp_size" else 64, 48000, 96000 if what == "dsp_rate" else 48000, 48000, **SLEWS)
    settle(o)
    ref, errs = o.fexchange0(x2)
    err = rel_rms(y, ref)
    print("%s %s after silence: rel RMS %.3e" % (drive_t.__name__, what, err))
    assert errs == 0 and err <= GATE
    assert np.all(y[:128 + 96] == 0.0) and np.abs(y).max() > 1e-3       # the latency and the up-slew's delay, as a channel just opened


CHANGES = {     # name: (call, in_size, rates) after (64, (48000, 48000, 48000))
    "SetInputSamplerate": (lambda lib: lib.SetInputSamplerate(CH, 96000), 64, (96000, 48000, 48000)),
    "SetOutputSamplerate": (lambda lib: lib.SetOutputSamplerate(CH, 96000), 64, (48000, 48000, 96000)),
    "SetInputBuffsize": (lambda lib: lib.SetInputBuffsize(CH, 128), 128, (48000, 48000, 48000)),
    "SetAllRates": (lambda lib: lib.SetAllRates(CH, 96000, 48000, 96000), 64, (96000, 48000, 96000)),
}


@pytest.mark.parametrize("name,drive_t", [(n, Host) for n in CHANGES] + [("SetInputBuffsize", Dev), ("SetAllRates", Dev)],
                         ids=lambda v: v if isinstance(v, str) else v.__name__)
def test_in_and_out_changes_rebuild_the_iobuffs_and_leave_the_dsp_running(qh, oracle, name, drive_t):
    lib = qh.load()
    call, in2, rates2 = CHANGES[name]
    out2 = in2 // (rates2[0] // rates2[2]) if rates2[0] >= rates2[2] else in2 * (rates2[2] // rates2[0])      # channel.c:49-52
    x1, x2 = signal(64 * 60, 3), signal(in2 * 60 * 64 // in2 * rates2[0] // 48000, 4, float(rates2[0]))
    open_channel(lib, 64, 64, (48000, 48000, 48000))
    drive = drive_t(lib, 64)
    try:
        y1 = feed(drive, x1, 64, 64)
        call(lib)
        assert lib.qh_wdsp_status() == 0, lib.qh_last_error()
        drive.resize(in2)
        y2 = feed(drive, x2, in2, out2)
    finally:
        drive.close()
        lib.CloseChannel(CH)
    # the oracle channel at in = dsp = out goes on; the iobuffs and the resamplers around it are made anew, nothing armed
    o = oracle.WdspChannel(64, 64, 48000, 48000, 48000)
    settle(o)
    r1, n1 = Iobuffs(o.xrxa, 64, 64, 48000, 48000, 48000, **SLEWS).run(x1)
    rs_in = oracle.Resample(rates2[0], 48000) if rates2[0] != 48000 else (lambda v: v)
    rs_out = oracle.Resample(48000, rates2[2]) if rates2[2] != 48000 else (lambda v: v)
    io = Iobuffs(lambda v: rs_out(o.xrxa(rs_in(v))), in2, 64, rates2[0], 48000, rates2[2], **SLEWS)
    io.upflag = 0               # post_main_build sets `exchange` alone (channel.c:60-66)
    assert io.out_size == out2
    r2, n2 = io.run(x2)
    e1, e2 = rel_rms(y1, r1), rel_rms(y2, r2)
    print("%s %s: rel RMS %.3e before, %.3e behind" % (drive_t.__name__, name, e1, e2))
    assert n1 == 0 and n2 == 0 and e1 <= GATE and e2 <= GATE


@pytest.mark.parametrize("drive_t", [Host, Dev], ids=["host", "device"])
def test_the_slew_setters_ahead_of_the_first_sample_equal_open_channel_with_those_values(qh, oracle, drive_t):
    lib = qh.load()
    x = signal(64 * 70, 5)
    x[:29] = 0.0
    open_channel(lib, 64, 64, (48000, 48000, 48000), state=0, slews=dict(tdelayup=0.010, tslewup=0.025, tdelaydown=0.001, tslewdown=0.010))
    drive = drive_t(lib, 64)
    try:
        lib.SetChannelTDelayUp(CH, D(SLEWS["tdelayup"])); lib.SetChannelTSlewUp(CH, D(SLEWS["tslewup"]))
        lib.SetChannelTDelayDown(CH, D(SLEWS["tdelaydown"])); lib.SetChannelTSlewDown(CH, D(SLEWS["tslewdown"]))
        assert lib.qh_wdsp_status() == 0, lib.qh_last_error()
        assert lib.SetChannelState(CH, 1, 0) == 0
        y = feed(drive, x, 64, 64)
    finally:
        drive.close()
        lib.CloseChannel(CH)
    o = oracle.WdspChannel(64, 64, 48000, 48000, 48000, **SLEWS)
    settle(o)
    ref, _ = o.fexchange0(x)
    err = rel_rms(y, ref)
    print("%s slew setters: rel RMS %.3e" % (drive_t.__name__, err))
    assert err <= GATE


def test_the_delay_setter_in_mid_ramp_flushes_the_slews_and_the_down_setters_shape_the_way_down(qh, oracle):
    lib = qh.load()
    x = signal(64 * 60, 6)
    open_channel(lib, 64, 64, (48000, 48000, 48000))
    o = oracle.WdspChannel(64, 64, 48000, 48000, 48000)
    settle(o)
    io = Iobuffs(o.xrxa, 64, 64, 48000, 48000, 48000, **SLEWS)
    drive = Host(lib, 64)
    ys, rs = [], []
    try:
        for b in range(60):
            if b == 3:          # 192 samples in: the ramp (96 delay + 240 ramp samples) is under way
                assert io.upflag and io.ustate != 0
                lib.SetChannelTDelayUp(CH, D(0.004)); io.SetChannelTDelayUp(0.004)
            if b == 30:
                lib.SetChannelTSlewDown(CH, D(0.002)); io.SetChannelTSlewDown(0.002)
                lib.SetChannelTDelayDown(CH, D(0.001)); io.SetChannelTDelayDown(0.001)
                assert lib.SetChannelState(CH, 0, 0) == 1
                io.downflag = 1                 # channel.c:273
            blk = x[b * 64:(b + 1) * 64]
            y, (r, _) = drive(blk, 64), io.fexchange0(blk)
            assert (y is None) == (r is None), b
            if y is not None:
                ys.append(y); rs.append(r)
        assert lib.qh_wdsp_status() == 0, lib.qh_last_error()
    finally:
        lib.CloseChannel(CH)
    assert 33 <= len(ys) < 40 and io.exchange == 0      # the way down: 49 samples pass, 97 ramp, 65 zeros, the rest of that call
    err = rel_rms(np.concatenate(ys), np.concatenate(rs))
    print("slew setters in mid-stream: rel RMS %.3e over %d calls" % (err, len(ys)))
    assert err <= GATE


def test_a_bad_channel_and_a_refused_rate_set_the_status_and_change_nothing(qh, oracle):
    lib = qh.load()
    x = signal(64 * 50, 7)
    for f in (lib.SetInputBuffsize, lib.SetDSPBuffsize, lib.SetInputSamplerate, lib.SetDSPSamplerate, lib.SetOutputSamplerate, lib.SetType):
        f(31, 48000)
        assert lib.qh_wdsp_status() != 0            # not open
        f(77, 48000)
        assert lib.qh_wdsp_status() != 0            # no such channel
    lib.SetAllRates(31, 48000, 48000, 48000)
    assert lib.qh_wdsp_status() != 0
    for f in (lib.SetChannelTDelayUp, lib.SetChannelTSlewUp, lib.SetChannelTDelayDown, lib.SetChannelTSlewDown):
        f(31, D(0.01))
        assert lib.qh_wdsp_status() != 0
    open_channel(lib, 64, 64, (96000, 48000, 48000))
    drive = Host(lib, 64)
    try:
        y1 = feed(drive, x[:64 * 25], 64, 32)
        lib.SetDSPSamplerate(CH, 64000)             # 96 k / 64 k is whole in neither direction
        assert lib.qh_wdsp_status() != 0
        lib.SetDSPBuffsize(CH, 4096)                # above nc
        assert lib.qh_wdsp_status() != 0
        lib.SetOutputSamplerate(CH, 36000)
        assert lib.qh_wdsp_status() != 0
        lib.SetInputBuffsize(CH, 0)
        assert lib.qh_wdsp_status() != 0
        lib.SetType(CH, 1)
        assert lib.qh_wdsp_status() != 0
        lib.SetType(CH, 0)
        assert lib.qh_wdsp_status() == 0
        lib.SetAllRates(CH, 96000, 48000, 48000); lib.SetInputBuffsize(CH, 64); lib.SetDSPBuffsize(CH, 64)      # nothing changes: nothing is done
        assert lib.qh_wdsp_status() == 0
        y2 = feed(drive, x[64 * 25:], 64, 32)
    finally:
        lib.CloseChannel(CH)
    o = oracle.WdspChannel(64, 64, 96000, 48000, 48000, **SLEWS)
    settle(o)
    ref, _ = o.fexchange0(x)
    assert rel_rms(np.concatenate([y1, y2]), ref) <= GATE
