"""The long form of ANF / ANR (lms_long_kernel, quisk_amd/csrc/qh_demod.hpp): taps 1..2048 and delay 0..2047, the whole range of
wdsp/anf.c and anr.c, against the CPU oracle.  -m gpu.

Every case is a script of setter and run steps played to an engine and, channel by channel, to the oracle (`_play`).  The cases are
built as tests/test_gpu_rxa_parity.py::test_lms_notch_and_noise_reduction builds its own: 3 channels, shift and nbp0 on, USB / LSB / AM,
a fixed gain of 12 dB on channel 0 and a working AGC on the other two, so that a position-1 filter sits behind a live AGC; 60 DSP
blocks of 256.  The gate is that test's, relative RMS < 1e-6 per channel.

An LMS loop feeds its own rounding back, and its step-size logic compares nearly equal numbers.  So every case first shows on the
CPU that its input does not amplify: the oracle runs the script on x and on x (1 + 1e-13 g), g seeded unit noise, and the two outputs
must agree to 1e-8 (`GUARD`).  A case that does not is an error in the choice of input, not a reason to skip.  The input is the
project's synthetic one, tone and noise level per channel (`SIGNAL`): behind the filters a tone as strong as the noise beside it for
the USB channel, band-limited noise for the LSB channel (the tone is in the other sideband) and the envelope of both for AM.  What
was tried on the CPU before these were kept: the ANF amplifies 1e-13 to between 1e-10 and 3e-8 on noise with a tone 10 dB above or
below it, whatever the seed, and stays under 1e-9 with the two level.

The AM channel runs the ANR of the case's taps and delay where the other two run the ANF.  An envelope has a mean, which is a pure
tone at 0 Hz in front of the notch filter -- the input class DESIGN.md section 7 records as amplifying: the reference alone moved
1e-7 to 5e-4 there under the guard's noise, with a carrier, without one and with a noise-modulated one.  The ANF is therefore held on
the USB and the LSB channel (and on three such channels where all three run it), the ANR on all.

Without the long form every case here but the short-form channels of the mixed engine fails with QH_ERR_UNSUPPORTED."""
import re

import numpy as np
import pytest

from conftest import rel_rms
from quisk_amd import synth

pytestmark = pytest.mark.gpu

GATE, GUARD = 1e-6, 1e-8
NCH, NBLK = 3, 60
MODES = (1, 0, 6)                                   # USB, LSB, AM
SSB = (1, 0, 1)                                     # where every channel runs the ANF
SIGNAL = ((0.01, 0.05, 1000), (0.002, 0.1, 78), (0.01, 0.05, 1002))     # per channel: tone, sigma, noise seed
BANDS = {1: (300.0, 3000.0), 0: (-3000.0, -300.0), 6: (-4000.0, 4000.0)}
AGC = (0, 4, 1)                                     # channel 0 fixed (12 dB), 1 fast, 2 long
GAIN = {"ANF": (1e-4, 0.1), "ANR": (2e-4, 0.05)}    # two_mu, gamma
QH_ERR_INVALID = -2

_inputs = {}


def _x(nblk=NBLK, per=1024, fs=192000.0):
    """the shared input, never written to"""
    key = (nblk, per, fs)
    if key not in _inputs:
        n = nblk * per
        t = np.arange(n, dtype=np.float64)
        x = np.empty((NCH, n), dtype=np.complex128)
        for ch, (a1, sigma, seed) in enumerate(SIGNAL):     # synth.make_input_numpy's model without the out-of-band tone
            g = np.random.default_rng(seed).standard_normal((n, 2))
            x[ch] = a1 * np.exp(2j * np.pi * ((synth.channel_tones(ch, fs)[0] / fs) * t % 1.0)) + sigma * (g[:, 0] + 1j * g[:, 1])
        x.setflags(write=False)
        _inputs[key] = x
    return _inputs[key]


def _perturbed(x):
    g = np.random.default_rng(20260).standard_normal(x.shape)
    with np.errstate(invalid="ignore"):             # (the isolation case's input holds NaN and inf)
        return x * (1.0 + 1e-13 * g)


class _Ref:
    """One oracle channel under the engine's setter names.  The oracle binds SetRXAANFVals / ANRVals only: Taps and Delay go through
    Vals with the other three values as they stand -- the same flush_anf (anf.c:184-211)."""

    def __init__(self, oracle, size=256, in_rate=192000):
        self.o = oracle.WdspChannel(size * in_rate // 48000, size, in_rate, 48000, 48000)
        self.vals = {}

    def __getattr__(self, name):
        m = re.match(r"SetRXA(ANF|ANR)(Vals|Taps|Delay)$", name)
        if not m:
            return getattr(self.o, name)
        f, what = m.groups()

        def call(*a):
            v = list(a) if what == "Vals" else list(self.vals[f])       # (Taps / Delay before any Vals: an error in the test)
            if what == "Taps":
                v[0] = a[0]
            if what == "Delay":
                v[1] = a[0]
            self.vals[f] = v
            getattr(self.o, "SetRXA%sVals" % f)(*v)
        return call


def _base(ch, modes=MODES):
    steps = [("set", ch, "SetRXAShiftRun", 1), ("set", ch, "SetRXAShiftFreq", synth.shift_freq(ch)), ("set", ch, "RXANBPSetRun", 1),
             ("set", ch, "SetRXAMode", modes[ch]), ("set", ch, "RXASetPassband") + BANDS[modes[ch]], ("set", ch, "SetRXAAGCMode", AGC[ch])]
    if ch == 0:
        steps.append(("set", ch, "SetRXAAGCFixed", 12.0))
    return steps


def _lms(ch, f, position, taps, delay, run=1, modes=MODES):
    if f == "ANF" and modes[ch] == 6:
        f = "ANR"                                   # (the module's docstring)
    return [("set", ch, "SetRXA%sPosition" % f, position), ("set", ch, "SetRXA%sVals" % f, taps, delay) + GAIN[f], ("set", ch, "SetRXA%sRun" % f, run)]


def _play(target, steps, x, ch=None, per=1024):
    """The script on an engine (ch None) or on channel ch's _Ref: ("set", channel, name, args...) and ("run", blocks), or a callable
    for the engine alone.  Returns the outputs of the run steps, one array per step."""
    out, pos = [], 0
    for s in steps:
        if callable(s):
            if ch is None:
                s(target)
        elif s[0] == "run":
            seg = x[:, pos * per:(pos + s[1]) * per]
            pos += s[1]
            out.append(target.process_host(seg) if ch is None else target.xrxa(np.ascontiguousarray(seg[ch])))
        elif ch is None:
            getattr(target, s[2])(s[1], *s[3:])
        elif s[1] in (ch, -1):
            getattr(target, s[2])(*s[3:])
    return out


def _reference(oracle, steps, x, chans=range(NCH)):
    """The oracle's outputs per channel, after the guard has shown that the case's input does not amplify."""
    xp = _perturbed(x)
    refs = {}
    for ch in chans:
        refs[ch] = _play(_Ref(oracle), steps, x, ch)
        twin = _play(_Ref(oracle), steps, xp, ch)
        g = rel_rms(np.concatenate(twin), np.concatenate(refs[ch]))
        assert np.abs(np.concatenate(refs[ch])).max() > 1e-3, (ch, "silent reference")
        assert g < GUARD, "channel %d: the reference alone moves %.2e under 1e-13 of input noise: choose another input" % (ch, g)
    return refs


def _hold(y, refs, what, chans=None):
    """Every channel inside the gate over the whole run, and every run step of it on its own: the step's RMS error against the RMS of
    the channel's whole reference (a stream's first block is the filters' latency, 1e-28 against 1e-28, and has no relative error of
    its own; any later step carries the stream's level).  The figures are printed first."""
    def steps(ch):
        level = np.sqrt(np.mean(np.abs(np.concatenate(refs[ch])) ** 2))
        whole = rel_rms(np.concatenate([seg[ch] for seg in y]), np.concatenate(refs[ch]))
        return [whole] + [float(np.sqrt(np.mean(np.abs(seg[ch] - r) ** 2))) / level for seg, r in zip(y, refs[ch])]
    errs = {ch: steps(ch) for ch in (refs if chans is None else chans)}
    print("%s: %s" % (what, "; ".join("ch %d %s" % (ch, " ".join("%.1e" % v for v in e)) for ch, e in errs.items())), flush=True)
    for ch, e in errs.items():
        assert max(e) < GATE, (what, ch, e)


def _engine(qh, steps, x, **kw):
    e = qh.RxaEngine(NCH, **kw)
    try:
        return _play(e, steps, x, per=e.dsp_insize), e.device_bytes()
    finally:
        e.close()


# ---- parity: every taps / delay pair with each filter and at each position ---------------------------------------------------------
PAIRS = [(65, 16), (128, 16), (1000, 64), (2032, 16), (2048, 16), (128, 0), (64, 65), (100, 2000), (2048, 2047)]
PARITY = []
for i, (taps, delay) in enumerate(PAIRS):           # two cases per pair: each filter and each position once, the four combinations in turn
    PARITY += [("ANF", i & 1, taps, delay), ("ANR", 1 - (i & 1), taps, delay)]


def _parity(f, position, taps, delay):
    return sum((_base(ch) + _lms(ch, f, position, taps, delay) for ch in range(NCH)), []) + [("run", NBLK)]


@pytest.mark.parametrize("f,position,taps,delay", PARITY, ids=["%s-p%d-%d-%d" % c for c in PARITY])
def test_long_form_follows_the_reference(qh, oracle, f, position, taps, delay):
    x = _x()
    steps = _parity(f, position, taps, delay)
    refs = _reference(oracle, steps, x)
    y, _ = _engine(qh, steps, x)
    _hold(y, refs, "%s at %d, %d / %d" % (f, position, taps, delay))


# ---- both forms in one engine -------------------------------------------------------------------------------------------------------
def _mixed(long_form):
    steps = sum((_base(ch, SSB) for ch in range(NCH)), [])
    steps += _lms(0, "ANF", 0, 64, 16)
    steps += _lms(1, "ANF", 1, 256 if long_form else 64, 16)
    steps += _lms(2, "ANF", 0, 48, 20, modes=SSB) + _lms(2, "ANR", 0, 512 if long_form else 48, 32 if long_form else 20)
    return steps + [("run", 20), ("run", 40)]


def test_both_forms_in_one_engine(qh, oracle):
    """channel 0 at 64 / 16 (short), channel 1 at 256 / 16, channel 2 with ANF 48 / 20 (short) and ANR 512 / 32 together: each follows
    its oracle, and channel 0 leaves the bits it leaves in an engine whose channels are all short -- whose memory is smaller by the
    long form's lists and the two filters' rows, which only the first engine has made"""
    x = _x()
    refs = _reference(oracle, _mixed(True), x)
    y, bytes_long = _engine(qh, _mixed(True), x)
    _hold(y, refs, "mixed forms")
    y_short, bytes_short = _engine(qh, _mixed(False), x)
    for a, b in zip(y, y_short):
        assert np.array_equal(a[0], b[0])
    assert bytes_long - bytes_short == 6 * NCH * 4 + 2 * NCH * 4096 * 8, (bytes_long, bytes_short)


# ---- setters in mid-stream -----------------------------------------------------------------------------------------------------------
def _walk():
    steps = sum((_base(ch) for ch in range(NCH)), []) + _lms(0, "ANR", 0, 64, 16) + _lms(1, "ANF", 0, 64, 16) + [("run", 1)]
    steps += [("set", 1, "SetRXAANFVals", 256, 16) + GAIN["ANF"], ("run", 7)]
    steps += [("set", 1, "SetRXAANFVals", 64, 16) + GAIN["ANF"], ("run", 3)]
    steps += [("set", 1, "SetRXAANFTaps", 1024), ("run", 20)]
    steps += [("set", 1, "SetRXAANFDelay", 0), ("run", 1)]
    steps += [("set", 1, "SetRXAANFRun", 0), ("set", 1, "SetRXAANFRun", 1), ("run", 7)]
    steps += [("set", 1, "SetRXAANFPosition", 1), ("run", 3), ("run", 18)]
    assert sum(s[1] for s in steps if s[0] == "run") == NBLK
    return steps


def test_setter_walk_across_the_forms(qh, oracle):
    """channel 1 (LSB, AGC fast) walks 64/16 -> 256/16 -> 64/16 -> Taps 1024 -> Delay 0 -> off / on -> the other position, with calls of
    1, 7, 3 and 20 blocks between: lidx / ngamma cross the forms in LmsState, every setter flushes the rows of the form it leaves
    and of the one it enters"""
    x = _x()
    refs = _reference(oracle, _walk(), x)
    y, _ = _engine(qh, _walk(), x)
    _hold(y, refs, "setter walk")


# ---- how the calls are cut -----------------------------------------------------------------------------------------------------------
CUTS = [1, 2, 5, 13, 39]


def _ragged(cuts):
    return sum((_base(ch) + _lms(ch, "ANF", 0, 1000, 64) + _lms(ch, "ANR", 1, 128, 0) for ch in range(NCH)), []) + [("run", k) for k in cuts]


def test_ragged_calls(qh, oracle):
    """calls of 1, 2, 5, 13 and 39 blocks against one call of 60, ANF 1000 / 64 at position 0 and ANR 128 / 0 at position 1 on every
    channel (the AM channel: the ANR twice over, the second setting of it at position 1 the one that stays).  Both streams are held to
    the oracle at the gate.  Against each other the bound is the gate as well: the long form itself does not depend on the cut (sigma
    is summed afresh for every sample), but the stages around it choose their tile forms by the call's length, and what they differ by
    in the last bit goes through the same fed-back loop as the reference's own rounding."""
    x = _x()
    refs = _reference(oracle, _ragged([NBLK]), x)
    whole, _ = _engine(qh, _ragged([NBLK]), x)
    cut, _ = _engine(qh, _ragged(CUTS), x)
    _hold(whole, refs, "one call of 60")
    joined = [np.concatenate(cut, axis=1)]
    _hold(joined, refs, "calls of %r" % CUTS)
    between = [rel_rms(joined[0][ch], whole[0][ch]) for ch in range(NCH)]
    print("cut against whole: %s" % " ".join("%.1e" % v for v in between), flush=True)
    assert max(between) < GATE, between


# ---- graph replay --------------------------------------------------------------------------------------------------------------------
def test_replayed_calls_leave_the_plain_launches_bits(qh):
    """a long-form ANF at position 0 and a long-form ANR at position 1 on every channel, one block per call on fixed device buffers
    (tests/test_gpu_graph_replay_matrix.py's run): replayed from the captured graphs and launched plainly, bit for bit"""
    import torch
    x = _x(24)
    cfg = sum((_base(ch, SSB) + _lms(ch, "ANF", 0, 256, 16, modes=SSB) + _lms(ch, "ANR", 1, 1000, 0) for ch in range(NCH)), [])
    dev = torch.device("cuda:0")
    outs, launches = [], []
    for replay in (False, True):
        e = qh.RxaEngine(NCH)
        try:
            _play(e, cfg, x)
            e.set_graph_replay(replay)
            d_in = torch.zeros((NCH, 1024), dtype=torch.complex128, device=dev)
            d_out = torch.zeros((NCH, 256), dtype=torch.complex128, device=dev)
            ys = []
            for k in range(24):
                d_in.copy_(torch.from_numpy(np.ascontiguousarray(x[:, k * 1024:(k + 1) * 1024])))
                torch.cuda.synchronize()
                e.process_ptr(d_in.data_ptr(), 1024, d_out.data_ptr(), 256, 1)
                e.synchronize()
                ys.append(d_out.cpu().numpy())
            outs.append(np.concatenate(ys, axis=1))
            launches.append(e.graph_launches())
        finally:
            e.close()
    assert launches[0] == 0 and launches[1] >= 24 - 3, launches
    assert np.all(np.isfinite(outs[0])) and np.abs(outs[0][:, 3 * 256:]).max() > 1e-3
    assert np.array_equal(outs[0], outs[1])


# ---- isolation -----------------------------------------------------------------------------------------------------------------------
def _poison(x):
    bad = np.array(x)
    bad[1, 10 * 1024 + 100:10 * 1024 + 200] = np.nan
    bad[1, 10 * 1024 + 300] = np.inf
    return bad


def _isolation():
    """ANF 64 / 16 (short), ANR 512 / 32 and ANF 256 / 16 on the three channels; 10 blocks, 10 whose start is non-finite on channel 1
    (`_poison`), 10 clean ones that wash the filters in front of the ANR, the setters that flush, 30 blocks"""
    steps = sum((_base(ch, SSB) for ch in range(NCH)), []) + _lms(0, "ANF", 0, 64, 16) + _lms(1, "ANR", 0, 512, 32) + _lms(2, "ANF", 1, 256, 16, modes=SSB)
    steps += [("set", 1, "SetRXAAGCMode", 0)]       # (an AGC that has seen a NaN keeps it: the filter's flush is the subject here)
    steps += [("run", 10), ("run", 10), ("run", 10)]
    steps += [("set", 1, "SetRXAANRVals", 512, 32) + GAIN["ANR"], ("set", 1, "SetRXAANRRun", 0), ("set", 1, "SetRXAANRRun", 1), ("run", 30)]
    return steps


def test_non_finite_input_stays_in_its_channel_and_a_flush_clears_it(qh, oracle):
    """Channel 1's input turns non-finite for a hundred samples.  The other channels leave the bits of an engine that never saw it.
    Channel 1's weights stay NaN, in the reference as here, until a setter flushes them (Vals: weights and ring; off / on: bp1's
    line as well, RXAbp1Set).  The step size does not: lidx only ever moves by constants, a comparison with a NaN takes the
    decrement, and the first clean sample behind the flush clamps it to lidx_min, which is where a new ANR starts.  So behind the flush
    setters the channel follows the oracle that was walked the same way, and that oracle's output is finite."""
    x = _x()
    bad = _poison(x)
    steps = _isolation()
    refs = {ch: _play(_Ref(oracle), steps, bad, ch) for ch in range(NCH)}
    twin = _play(_Ref(oracle), steps, _perturbed(bad), 1)
    assert np.all(np.isfinite(refs[1][3])) and not np.all(np.isfinite(refs[1][1]))
    assert rel_rms(twin[3], refs[1][3]) < GUARD
    y, _ = _engine(qh, steps, bad)
    clean, _ = _engine(qh, steps, x)
    assert not np.all(np.isfinite(y[1][1]))
    for k in range(4):
        for ch in (0, 2):
            assert np.array_equal(y[k][ch], clean[k][ch]), (k, ch)
    assert np.all(np.isfinite(y[3]))
    _hold(y[3:], {ch: r[3:] for ch, r in refs.items()}, "behind the flush setters")


# ---- refusals ------------------------------------------------------------------------------------------------------------------------
def _refusing(refused):
    steps = sum((_base(ch) + _lms(ch, "ANF", 0, 200, 70) + _lms(ch, "ANR", 1, 64, 16) for ch in range(NCH)), [])
    return steps + [("run", 10), refused, ("run", 20)]


def test_values_outside_the_line_are_refused_and_change_nothing(qh, oracle):
    x = _x()
    lib = qh.load()

    def refused(e):
        for f in ("ANF", "ANR"):
            for taps in (0, 2049, -1):
                assert getattr(lib, "qh_rxa_SetRXA%sTaps" % f)(e._h, 1, taps) == QH_ERR_INVALID
                assert getattr(lib, "qh_rxa_SetRXA%sVals" % f)(e._h, -1, taps, 16, 1e-4, 0.1) == QH_ERR_INVALID
            for delay in (-1, 2048):
                assert getattr(lib, "qh_rxa_SetRXA%sDelay" % f)(e._h, 1, delay) == QH_ERR_INVALID
                assert getattr(lib, "qh_rxa_SetRXA%sVals" % f)(e._h, -1, 64, delay, 1e-4, 0.1) == QH_ERR_INVALID
            assert b"taps 1..2048, delay 0..2047" in lib.qh_last_error()

    refs = _reference(oracle, _refusing(refused), x)
    y, _ = _engine(qh, _refusing(refused), x)
    _hold(y, refs, "around the refused setters")


# ---- a new dsp_size ------------------------------------------------------------------------------------------------------------------
SIZE1, SIZE2 = 64, 128


def _resized():
    """(the AM channel with its fade leveller off, as in tests/test_gpu_rxa_rates.py: setSize_amd keeps the detector's two averages,
    amd.c:253-256, and the slow one, tau 1.4 s, rests in no silence a test can afford)"""
    return sum((_base(ch) + _lms(ch, "ANR", ch & 1, 300, 70) for ch in range(NCH)), []) + [("set", 2, "SetRXAAMDFadeLevel", 0)]


def test_a_new_dsp_size_with_a_long_anr_running(qh, oracle):
    """tests/test_gpu_rxa_rates.py's composition for a new dsp_size: signal, silence until every kept line rests (nc 2048 and the
    ANR's window: 48 blocks of 64 are run), the change, signal -- against a fresh channel at the new size.  setSize_anr flushes and
    keeps lidx / ngamma (anr.c:154-158), and in silence both come back to what create_anr sets: lidx falls to lidx_min = 120, its
    first value, and the ngamma left behind multiplies y = 0 once before it is computed anew."""
    x1, x2 = _x(40, 4 * SIZE1), _x(40, 4 * SIZE2)
    cfg = _resized()
    e = qh.RxaEngine(NCH, dsp_size=SIZE1)
    try:
        _play(e, cfg, x1)
        for k in range(0, 40, 5):
            e.process_host(x1[:, k * 4 * SIZE1:(k + 5) * 4 * SIZE1])
        for _ in range(6):
            e.process_host(np.zeros((NCH, 8 * 4 * SIZE1), dtype=np.complex128))
        e.set_dsp_size(SIZE2)
        assert e.dsp_size == SIZE2 and e.dsp_insize == 4 * SIZE2
        y = _play(e, [("run", 15), ("run", 25)], x2, per=4 * SIZE2)
    finally:
        e.close()
    xp = _perturbed(x2)
    refs = {}
    for ch in range(NCH):
        r, twin = _Ref(oracle, size=SIZE2), _Ref(oracle, size=SIZE2)
        refs[ch] = _play(r, cfg + [("run", 15), ("run", 25)], x2, ch, per=4 * SIZE2)
        g = rel_rms(np.concatenate(_play(twin, cfg + [("run", 15), ("run", 25)], xp, ch, per=4 * SIZE2)), np.concatenate(refs[ch]))
        assert g < GUARD, (ch, g)
    _hold(y, refs, "behind set_dsp_size")
