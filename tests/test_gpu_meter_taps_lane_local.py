"""The fused meters' lane-local taps (quisk_amd/csrc/qh_osfir.hpp "fused meters", meter_finish_kernel; the arithmetic restated in
tests/meter_partials_ref.py): every row of 16 lanes of a band tile leaves one (sum, max) per tap, carried to the tile's end, and the finish
joins them over the call.  Held against the oracle's sample-by-sample xmeter where that scheme can go wrong -- a peak that decays
across tile seams and calls, calls that end inside a tile or on a seam, every front fold and ingest form ahead of the taps, the
stages that write between the front's store and nbp0's load, the wider band tiles -- and the audio's bits, which a tap must not
touch.  -m gpu."""
import numpy as np
import pytest
import torch

from conftest import rel_rms
from oracle import ingest_oracle as io
from quisk_amd import synth
from wdsp_gen_ref import Gen

pytestmark = pytest.mark.gpu

# mlog10 truncates the mantissa to 11 bits (wdsp/meterlog10.c): one step is 10*log10(2)/2048 dB
STEP_DB = 10.0 * np.log10(2.0) / 2048.0
NCH = 3
METERS = (0, 1, 2, 3, 5, 6)
DSP_RATE = 48000


def _setup(o, pre, ch, shift=True):
    o.SetRXAShiftRun(*pre, 1 if shift else 0)
    if shift:
        o.SetRXAShiftFreq(*pre, synth.shift_freq(ch))
    o.RXANBPSetRun(*pre, 1)
    o.SetRXAMode(*pre, 1)
    o.RXASetPassband(*pre, 300.0, 3000.0)
    o.SetRXAAGCMode(*pre, 0)
    o.SetRXAAGCFixed(*pre, 6.0 + ch)


def _engine(qh, dsp_size, in_rate=192000, meters=True, shift=True):
    e = qh.RxaEngine(NCH, dsp_size=dsp_size, in_rate=in_rate, dsp_rate=DSP_RATE, out_rate=DSP_RATE)
    for ch in range(NCH):
        _setup(e, (ch,), ch, shift)
    e.enable_meters(meters)
    return e


def _refs(oracle, dsp_size, in_rate=192000, shift=True):
    refs = []
    for ch in range(NCH):
        o = oracle.WdspChannel(dsp_size * (in_rate // DSP_RATE), dsp_size, in_rate, DSP_RATE, DSP_RATE)
        _setup(o, (), ch, shift)
        refs.append(o)
    return refs


def _hold_meters(e, refs, what):
    for ch in range(NCH):
        for mt in METERS:
            got, ref = e.GetRXAMeter(ch, mt), refs[ch].GetRXAMeter(mt)
            assert abs(got - ref) < 1.01 * STEP_DB, (what, ch, mt, got, ref)


def _walk(e, refs, x, calls, feed=None):
    """the engine and the oracles through the calls (in blocks): every meter after every call, the audio over the whole run (a first
    call of one block is the filters' start-up, 1e-11 of the signal, and rounding beside it)"""
    pos, ys, wants = 0, [], []
    for k, nb in enumerate(calls):
        seg = np.ascontiguousarray(x[:, pos:pos + nb * e.dsp_insize])
        pos += nb * e.dsp_insize
        ys.append(feed(seg, nb) if feed else e.process_host(seg))
        wants.append(np.stack([refs[ch].xrxa(seg[ch]) for ch in range(NCH)]))
        _hold_meters(e, refs, (k, nb))
    assert pos == x.shape[1]
    y, want = np.concatenate(ys, axis=1), np.concatenate(wants, axis=1)
    for ch in range(NCH):
        assert rel_rms(y[ch], want[ch]) < 1e-9, ch


def _quiet(n, in_rate=192000):
    """noise 60 dB under the bursts below, so that a decayed peak stays the largest thing the peak meters have seen"""
    return 1e-3 * synth.make_input_numpy(NCH, n, fs=float(in_rate))


def _burst(x, at, length, in_rate=192000):
    """a tone beside synth.channel_tones' first, inside each channel's passband behind its shift, over input samples [at, at + length)"""
    t = np.arange(at, at + length)
    for ch in range(NCH):
        x[ch, at:at + length] += np.exp(2j * np.pi * (((-1500.0 - synth.shift_freq(ch)) / in_rate * t) % 1.0))


@pytest.mark.parametrize("where", ["first block", "last sample"])
def test_a_burst_decays_across_tiles_and_calls(qh, oracle, where):
    """8 blocks of 256 fill one 2048-sample band tile exactly and two and a third 884-sample front tiles; the quiet calls behind read
    the burst's peak decayed over tile seams and call ends."""
    calls = [8, 3, 9, 1, 4]
    x = _quiet(sum(calls) * 1024)
    if where == "first block":
        _burst(x, 100, 600)
    else:
        x[:, 8 * 1024 - 1] += 40.0              # the call's last input sample: the filters' answer to it arrives in the next call
    e, refs = _engine(qh, 256), _refs(oracle, 256)
    _walk(e, refs, x, calls)
    peak, avg = e.GetRXAMeter(0, 0), e.GetRXAMeter(0, 1)
    assert peak > avg + 3.0, (peak, avg)        # the peak still is the burst's, not the noise's
    e.close()


@pytest.mark.parametrize("dsp_size,calls", [(256, [1, 3, 4, 9, 8, 1]), (64, [1, 31, 1, 31])])
def test_calls_that_end_inside_a_tile_or_on_a_seam(qh, oracle, dsp_size, calls):
    x = synth.make_input_numpy(NCH, sum(calls) * 4 * dsp_size)
    _burst(x, 4 * dsp_size // 2, 3 * dsp_size)
    e, refs = _engine(qh, dsp_size), _refs(oracle, dsp_size)
    _walk(e, refs, x, calls)
    e.close()


@pytest.mark.parametrize("in_rate", [96000, 192000, 384000])
def test_every_front_fold(qh, oracle, in_rate):
    dsp_size, calls = 256, [3, 9, 1]
    x = synth.make_input_numpy(NCH, sum(calls) * dsp_size * (in_rate // DSP_RATE), fs=float(in_rate))
    _burst(x, 50, 2000, in_rate)
    e, refs = _engine(qh, dsp_size, in_rate), _refs(oracle, dsp_size, in_rate)
    _walk(e, refs, x, calls)
    e.close()


def test_packed_24_bit_ingest(qh, oracle):
    dsp_size, calls = 256, [3, 9, 1]
    n = sum(calls) * 1024
    x = 0.25 * synth.make_input_numpy(NCH, n)
    _burst(x, 50, 2000)
    x *= 0.4 / np.abs(x).max()
    raws, xs = [], []
    for ch in range(NCH):
        q = np.round(np.stack([x[ch].real, x[ch].imag], axis=1) * 2 ** 23).astype("<i4")        # 24-bit ADC codes
        raws.append(q.view(np.uint8).reshape(n, 2, 4)[:, :, :3].tobytes())
        xs.append(io.read_rx_udp_le(raws[-1], 3, 1.0 / 2 ** 31))
    fmt = qh.IqFormat.le24(1.0 / 2 ** 31)
    e, refs = _engine(qh, dsp_size), _refs(oracle, dsp_size)
    at = [0]

    def feed(seg, nb):
        lo, hi = 6 * at[0], 6 * (at[0] + nb * 1024)
        at[0] += nb * 1024
        return e.process_packed_host(b"".join(r[lo:hi] for r in raws), fmt, hi - lo, nb)
    _walk(e, refs, np.stack(xs), calls, feed)
    e.close()


def test_a_front_that_is_not_overlap_save(qh, oracle):
    """in rate = dsp rate: the front stage is the oscillator alone"""
    dsp_size, calls = 256, [3, 9, 1]
    x = synth.make_input_numpy(NCH, sum(calls) * dsp_size, fs=float(DSP_RATE))
    e, refs = _engine(qh, dsp_size, DSP_RATE), _refs(oracle, dsp_size, DSP_RATE)
    _walk(e, refs, x, calls)
    e.close()


def test_a_channel_with_gen0_on(qh, oracle):
    """gen0 writes channel 2's row between the front's store and nbp0's load (RXA.c:565): its adc meter reads the generator"""
    dsp_size, calls = 256, [3, 9, 1]
    x = synth.make_input_numpy(NCH, sum(calls) * 1024)
    e, refs = _engine(qh, dsp_size), _refs(oracle, dsp_size)
    e.SetRXAPreGenMode(2, 0); e.SetRXAPreGenToneMag(2, 0.5); e.SetRXAPreGenToneFreq(2, 700.0); e.SetRXAPreGenRun(2, 1)
    g = Gen(DSP_RATE, dsp_size, run=1, mode=0)
    g.SetToneMag(0.5); g.SetToneFreq(700.0)
    refs[2] = oracle.WdspChannel(dsp_size, dsp_size, DSP_RATE, DSP_RATE, DSP_RATE)          # behind the front stage: the generator's row in
    _setup(refs[2], (), 2, shift=False)
    gen_row = g.blocks(sum(calls))              # at the dsp rate
    pos, ys, wants = 0, [], []
    for k, nb in enumerate(calls):
        seg = np.ascontiguousarray(x[:, pos * 1024:(pos + nb) * 1024])
        ys.append(e.process_host(seg))
        wants.append(np.stack([refs[ch].xrxa(gen_row[pos * 256:(pos + nb) * 256] if ch == 2 else seg[ch]) for ch in range(NCH)]))
        pos += nb
        _hold_meters(e, refs, (k, nb))
    y, want = np.concatenate(ys, axis=1), np.concatenate(wants, axis=1)
    for ch in range(NCH):
        assert rel_rms(y[ch], want[ch]) < 1e-9, ch
    e.close()


@pytest.mark.parametrize("tile", [6144, 8192])
def test_the_wider_band_tiles(qh, oracle, tile):
    """384 lanes and a 4096-sample tile; two groups of 256 lanes whose registers hold a 6144-sample tile in two runs"""
    dsp_size, calls = 256, [8, 1, 30, 17]
    x = _quiet(sum(calls) * 1024)
    _burst(x, 100, 600)
    _burst(x, 20 * 1024, 3000)
    e, refs = _engine(qh, dsp_size), _refs(oracle, dsp_size)
    e.set_band_tile(tile)
    _walk(e, refs, x, calls)
    assert e.band_tile() == tile
    e.close()


def _front_alone(qh, meters):
    e = qh.RxaEngine(NCH, dsp_size=256)
    for ch in range(NCH):
        e.SetRXAShiftRun(ch, 1); e.SetRXAShiftFreq(ch, synth.shift_freq(ch))
        e.RXANBPSetRun(ch, 0); e.SetRXAMode(ch, 1)
        e.SetRXAAGCMode(ch, 0); e.SetRXAAGCFixed(ch, 0.0)
    e.enable_meters(meters)
    return e


def test_front_output_is_the_same_bits_with_meters_on_and_off(qh):
    """a chain that is the front stage alone: what the front kernel stores must not depend on the meters"""
    x = synth.make_input_numpy(NCH, 12 * 1024)
    on, off = _front_alone(qh, True), _front_alone(qh, False)
    for lo, hi in ((0, 3), (3, 12)):
        seg = np.ascontiguousarray(x[:, lo * 1024:hi * 1024])
        assert np.array_equal(on.process_host(seg), off.process_host(seg))
    on.close(); off.close()


def test_audio_bits_across_engines_and_graph_replay(qh):
    """the nbp0 chain with meters on: two engines agree to the bit, and replayed launches with plain ones, audio and meters"""
    nb = 12
    x = synth.make_input_numpy(NCH, nb * 1024)
    dev = torch.device("cuda:0")
    outs, meters = [], []
    for replay in (False, False, True):
        e = _engine(qh, 256)
        e.set_graph_replay(replay)
        d_in = torch.zeros((NCH, 1024), dtype=torch.complex128, device=dev)
        d_out = torch.zeros((NCH, 256), dtype=torch.complex128, device=dev)
        y = np.zeros((NCH, nb * 256), dtype=np.complex128)
        for b in range(nb):
            d_in.copy_(torch.from_numpy(x[:, b * 1024:(b + 1) * 1024]))
            torch.cuda.synchronize()
            e.process_ptr(d_in.data_ptr(), 1024, d_out.data_ptr(), 256, 1)
            e.synchronize()
            y[:, b * 256:(b + 1) * 256] = d_out.cpu().numpy()
        assert (e.graph_launches() > 0) == replay
        outs.append(y)
        meters.append([[e.GetRXAMeter(ch, mt) for mt in METERS] for ch in range(NCH)])
        e.close()
    assert np.abs(outs[0]).max() > 1e-3
    assert np.array_equal(outs[0], outs[1]) and np.array_equal(outs[0], outs[2])
    assert meters[0] == meters[1] and meters[0] == meters[2]
