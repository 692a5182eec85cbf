"""wdsp_iobuffs_ref.Iobuffs around wo_xrxa_block of one oracle channel equals wo_fexchange0 of a second, identically set channel, sample
for sample: over ragged in_size / dsp_insize pairs and through the up-slew (no GPU).  The restatement also carries what the oracle leaves
out -- the down-slew, the four slew setters -- whose state machines are checked against iobuffs.c's counts here."""
import numpy as np
import pytest

from wdsp_iobuffs_ref import Iobuffs

# (in_size, in_rate): dsp_size 64 at 48 kHz, so dsp_insize is 64 or 256.  in_size 96 against dsp_insize 64 is no case: see
# test_sizes_that_do_not_divide_run_past_the_reference_s_ring
PAIRS = [(64, 48000), (64, 192000), (256, 48000), (256, 192000), (128, 192000)]


def channel(oracle, in_size, in_rate, **slews):
    o = oracle.WdspChannel(in_size, 64, in_rate, 48000, 48000, **slews)
    o.SetRXAMode(1)
    o.RXASetPassband(300.0, 3000.0)
    o.SetRXAAGCMode(3)
    return o


def noise(n, seed):
    g = np.random.default_rng(seed).standard_normal((n, 2))
    x = 0.1 * (g[:, 0] + 1j * g[:, 1])
    x[:37] = 0.0                # the up-slew starts at the first sample that is not zero
    return x


@pytest.mark.parametrize("in_size,in_rate", PAIRS)
def test_the_restatement_around_xrxa_equals_fexchange0(oracle, in_size, in_rate):
    slews = dict(tdelayup=0.002, tslewup=0.005, tdelaydown=0.0, tslewdown=0.010)
    a, b = channel(oracle, in_size, in_rate, **slews), channel(oracle, in_size, in_rate, **slews)
    io = Iobuffs(a.xrxa, in_size, 64, in_rate, 48000, 48000, **slews)
    assert (io.dsp_insize, io.dsp_outsize, io.out_size) == (b.dsp_insize, b.dsp_outsize, b.out_size)
    nblk = 6 * max(1, io.dsp_insize // in_size) + 2400 * (in_rate // 48000) // in_size     # through the delay and the ramp, and beyond
    x = noise(nblk * in_size, 5)
    ref, ref_errs = b.fexchange0(x)
    y, errs = io.run(x)
    assert errs == ref_errs
    assert np.array_equal(y, ref)
    assert not io.upflag and np.abs(y).max() > 1e-3


def test_sizes_that_do_not_divide_run_past_the_reference_s_ring():
    """in_size 96 with dsp_insize = dsp_outsize 64: r2 holds 2 x 96 samples and dexchange's index goes 96 -> 160 -> 224, never equal to 192
    (iobuffs.c:592-594), so the reference's memcpy writes past r2 on the second DSP block.  The restatement refuses where that happens; an
    oracle channel with these sizes corrupts its heap, so none is made."""
    io = Iobuffs(lambda x: x, 96, 64, 48000, 48000, 48000)
    assert (io.r2_active, io.r2_inidx, io.r2_insize) == (192, 96, 64)
    with pytest.raises(ValueError):
        io.run(np.ones(96 * 4, dtype=np.complex128))


def test_the_slew_counts_are_the_references():
    io = Iobuffs(lambda x: x, 64, 64, 48000, 48000, 48000, tdelayup=0.001, tslewup=0.002, tdelaydown=0.0005, tslewdown=0.001)
    assert (io.ndelup, io.ntup, io.ndeldown, io.ntdown) == (48, 96, 24, 48)
    x = np.ones(64 * 8, dtype=np.complex128)
    y, errs = io.run(x)
    assert errs == 0
    # the identity block comes out two DSP blocks late (iobuffs.c:409-411): muted trigger sample, ndelup + 1 zeros, the ramp over ntup + 1 samples
    got = y[128:].real
    lead = 1 + 48 + 1
    assert np.all(got[:lead] == 0.0)
    assert np.allclose(got[lead:lead + 97], 0.5 * (1.0 - np.cos(np.pi * np.arange(97) / 96)), atol=1e-15)
    assert np.all(got[lead + 97:] == 1.0)
    # SetChannelTDelayUp in mid-ramp: flush_slews drops the flag, the input passes as it is from the next call on (iobuffs.c:88-96,475-478)
    io = Iobuffs(lambda x: x, 64, 64, 48000, 48000, 48000, tdelayup=0.001, tslewup=0.002)
    y1, _ = io.run(x[:128])
    assert io.upflag and io.ustate != 0
    io.SetChannelTDelayUp(0.003)
    assert (io.ndelup, io.upflag, io.ustate) == (144, 0, 0)
    y2, _ = io.run(x[:256])
    assert np.all(y2[128:] == 1.0)
    # the ramps' setters make the slews anew (channel.c:313-323,337-347)
    io.SetChannelTSlewUp(0.001)
    io.SetChannelTSlewDown(0.002)
    assert (io.ntup, io.cup.size, io.ntdown, io.cdown.size) == (48, 49, 96, 97)
    # the down-slew: ndeldown + 1 samples pass, the ramp, out_size + 1 zeros, then the exchange goes off at a call's end (iobuffs.c:226-300,496-503)
    io = Iobuffs(lambda x: x, 64, 64, 48000, 48000, 48000, tdelayup=0.0, tslewup=0.0, tdelaydown=0.0, tslewdown=0.001)
    io.run(x[:256])
    io.downflag = 1             # SetChannelState(channel, 0, 0), channel.c:273
    y, _ = io.run(x[:192])
    assert np.all(y[:1] == 1.0) and np.allclose(y[1:50].real, 0.5 * (1.0 + np.cos(np.pi * np.arange(49) / 48)), atol=1e-15) and np.all(y[50:] == 0.0)
    assert io.exchange == 0 and io.fexchange0(x[:64]) == (None, 0)
