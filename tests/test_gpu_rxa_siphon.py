"""xsiphon in the batched RXA engine (RXA.c:590): get_sip after every call against the oracle's midbuff at HOOK_AUDIO (oracle/
wdsp_oracle.c:1146, the very point of RXA.c:590) pushed through the restated siphon (tests/rxa_taps_ref.Siphon).

The chain agrees with the oracle to 1e-9 relative RMS and the siphon only copies: every read is held to 1e-9 relative RMS of the
reference's read, zeros to zeros.  The siphons are switched on behind WARM blocks: a chain that starts from zeros puts out the precursor
of its filters first (an AM channel's two 2048-tap filters leave 5e-9 of the signal's level in its first 768 samples), where the two
FFT convolutions differ by their rounding, 1e-16 of the signal's level and 3e-8 of such a sample -- a one-sample read there measures the
rounding of the transform, not the tap.  Switched on in mid-stream the ring starts as a flushed one, so the reads of the first calls
still have zeros ahead of the samples.  -m gpu."""
import numpy as np
import pytest

from conftest import rel_rms
from oracle import pyoracle
from rxa_chain_ref import RxaChainRef
from rxa_taps_ref import Siphon
from rxa_taps_util import CALLS, MODES, capture, engine, oracle_channel, passband, signal
from quisk_amd import synth

pytestmark = pytest.mark.gpu
TOL = 1e-9
SIZES = (1, 256, 4095, 4096)
WARM = 24                                                   # blocks ahead of the siphons: past the filters' delay, twice
USB = [1] * len(MODES)


def _warm(e, oracles, x, modes=None):
    """the first WARM blocks of x through both, unchecked, with the siphons on; then every siphon off and on again, which leaves it as
    flush_siphon does.  Returns the rest of x.  modes: the channels run as USB over the first half and take their modes then, on both
    sides at the same block -- the FM loop's atan2 turns the last bit of whichever FFT fills the filters into full scale when it starts
    on an empty chain, and acquires as a smooth function of its input on a primed one (tests/test_gpu_acquisition.py)."""
    n = WARM * e.dsp_insize
    e.set_siphon(-1, 1)
    if modes:
        n //= 2
        e.process_host(np.ascontiguousarray(x[:, :n]))
        for c, o in enumerate(oracles):
            o.xrxa(x[c, :n])
            e.SetRXAMode(c, modes[c]); e.RXASetPassband(c, *passband(modes[c]))
            o.SetRXAMode(modes[c]); o.RXASetPassband(*passband(modes[c]))
        x = x[:, n:]
    e.process_host(np.ascontiguousarray(x[:, :n]))
    for c, o in enumerate(oracles):
        o.xrxa(x[c, :n])
    assert np.any(e.get_sip(0, 4096))
    e.set_siphon(-1, 0); e.set_siphon(-1, 1)
    assert not np.any(e.get_sip(0, 4096))
    return x[:, n:]


def _same(got, want, what, bad=None):
    """the relative RMS error of a read (zeros to zeros: 0); more than TOL is entered in `bad`, or asserted at once without one"""
    r = (0.0 if not np.any(got) else np.inf) if not np.any(want) else rel_rms(got, want)
    if bad is None:
        assert r < TOL, (what, r)
    elif not r < TOL:
        bad.append((what, r))
    return r


def _follow(e, oracles, x, calls, dsp_size=256, sizes=SIZES, sips=None):
    """the calls through the engine and the oracle channels; get_sip of every channel after every call against the restated siphon.
    Returns (engine outputs, oracle outputs, the siphons)."""
    sips = sips or [Siphon(dsp_size) for _ in oracles]
    ys, yr, pos, worst, bad = [], [], 0, 0.0, []
    for k, nb in enumerate(calls):
        n = nb * e.dsp_insize
        ys.append(e.process_host(np.ascontiguousarray(x[:, pos:pos + n])))
        out = []
        for c, o in enumerate(oracles):
            mid, y = capture(o, pyoracle.WdspChannel.HOOK_AUDIO, x[c, pos:pos + n])
            out.append(y)
            sips[c].push(mid)
            for size in sizes:
                worst = max(worst, _same(e.get_sip(c, size), sips[c].suck(size), (k, c, size), bad))
        yr.append(np.stack(out))
        print("call", k, "outputs' rel rms", [rel_rms(ys[-1][c], yr[-1][c]) for c in range(len(oracles))])
        pos += n
    print("worst get_sip rel rms", worst)
    assert not bad, bad
    return np.concatenate(ys, 1), np.concatenate(yr, 1), sips


def _oracles(oracle, modes, dsp_size=256):
    return [oracle_channel(oracle, c, m, dsp_size=dsp_size) for c, m in enumerate(modes)]


def test_every_mode_agc_mode_3(qh, oracle):
    """the default AGC (mode 3) on the five modes; the AM channel runs bp1, so its row lies in the other buffer (L_BP1)"""
    x = signal(MODES, (WARM + sum(CALLS)) * 1024)
    e, os_ = engine(qh, USB), _oracles(oracle, USB)
    try:
        for c, o in enumerate(os_):
            e.SetRXAAGCMode(c, 3); o.SetRXAAGCMode(3)
        x = _warm(e, os_, x, MODES)
        ys, yr, _ = _follow(e, os_, x, CALLS)
        for c in range(5):
            assert rel_rms(ys[c], yr[c]) < TOL, c
    finally:
        e.close()
        for o in os_:
            o.close()


def test_fixed_gain_is_in_the_ring(qh, oracle):
    """AGC mode 0 with a fixed gain other than 1: the chain multiplies it in behind the siphon's point, the ring must hold it"""
    x = signal(MODES, (WARM + sum(CALLS)) * 1024, seed=3)
    e, os_ = engine(qh, USB), _oracles(oracle, USB)
    try:
        for c, o in enumerate(os_):
            db = 6.0 + 7.0 * c
            e.SetRXAAGCMode(c, 0); e.SetRXAAGCFixed(c, db)
            o.SetRXAAGCMode(0); o.SetRXAAGCFixed(db)
        x = _warm(e, os_, x, MODES)
        ys, yr, sips = _follow(e, os_, x, CALLS)
        for c in range(5):
            assert rel_rms(ys[c], yr[c]) < TOL, c
        # a new gain between calls reaches the ring with the next call
        e.SetRXAAGCFixed(0, 31.0); os_[0].SetRXAAGCFixed(31.0)
        x2 = signal(MODES, 5 * 1024, seed=4)
        _follow(e, os_, x2, (5,), sips=sips)
    finally:
        e.close()
        for o in os_:
            o.close()


def test_the_tap_sits_ahead_of_cbl_peak_and_ssql(qh):
    """xcbl, the CW peak filter and SSQL on: the output still matches the whole-chain reference, and the ring holds their INPUT"""
    modes = [1, 4, 6]
    x = signal(modes, (WARM + sum(CALLS)) * 1024, seed=6)
    e = engine(qh, modes)
    refs = []
    for c, m in enumerate(modes):
        r = RxaChainRef()
        r.SetRXAShiftRun(1); r.SetRXAShiftFreq(synth.shift_freq(c)); r.RXANBPSetRun(1); r.SetRXAMode(m); r.RXASetPassband(*passband(m))
        refs.append(r)
    try:
        for c, r in enumerate(refs):
            for name, args in (("SetRXACBLRun", (1,)), ("SetRXASPCWRun", (1,)), ("SetRXASSQLRun", (1,))):
                getattr(e, name)(c, *args); getattr(r, name)(*args)
        e.SetRXAAGCMode(0, 0); e.SetRXAAGCFixed(0, 12.0); refs[0].SetRXAAGCMode(0); refs[0].SetRXAAGCFixed(12.0)
        x = _warm(e, refs, x)
        sips = [Siphon(256) for _ in refs]
        pos = 0
        for k, nb in enumerate(CALLS):
            n = nb * 1024
            y = e.process_host(np.ascontiguousarray(x[:, pos:pos + n]))
            for c, r in enumerate(refs):
                mids = []

                def hook(where, z, aux, r=r, mids=mids):
                    if where == pyoracle.WdspChannel.HOOK_AUDIO:
                        mids.append(z.copy())
                    r._hook(where, z, aux)
                r.o.set_stage_hook(hook)
                yr = r.xrxa(x[c, pos:pos + n])
                sips[c].push(np.concatenate(mids))
                d = rel_rms(y[c], yr) if np.any(yr) else float(np.any(y[c]))
                assert d < TOL, (k, c, d)
                for size in SIZES:
                    _same(e.get_sip(c, size), sips[c].suck(size), (k, c, size))
            pos += n
        assert all(r.ran["cbl"] and r.ran["peaks"] and r.ran["ssql"] for r in refs)
    finally:
        e.close()
        for r in refs:
            r.close()


@pytest.mark.parametrize("dsp_size", [4096, 8192])
def test_blocks_as_long_as_the_ring(qh, oracle, dsp_size):
    """insize >= sipsize: the ring holds the last 4096 samples of the last block and idx stays"""
    calls = (1, 2)
    x = signal([1], sum(calls) * 4 * dsp_size, seed=dsp_size)
    e, os_ = engine(qh, [1], dsp_size=dsp_size), _oracles(oracle, [1], dsp_size=dsp_size)
    try:
        e.set_siphon(0, 1)
        _, _, sips = _follow(e, os_, x, calls, dsp_size=dsp_size)
        assert sips[0].idx == 0
    finally:
        e.close(); os_[0].close()


def test_flush_and_refusals(qh, oracle):
    x = signal([1, 0], 12 * 1024, seed=8)
    e, os_ = engine(qh, [1, 0]), _oracles(oracle, [1, 0])
    lib = qh.load()

    def fixed(o):                                           # (flush_wcpagc zeroes the ring and keeps the loop's gains: with a fixed gain
        o.SetRXAAGCMode(0); o.SetRXAAGCFixed(9.0)           # a flushed chain is a fresh one)
    try:
        e.SetRXAAGCMode(-1, 0); e.SetRXAAGCFixed(-1, 9.0); fixed(os_[0])
        e.set_siphon(0, 1)
        assert not np.any(e.get_sip(0, 4096))               # switched on, no call yet: a flushed siphon
        _follow(e, [os_[0]], x[:, :7 * 1024], (7,))
        assert np.any(e.get_sip(0, 4096))
        e.flush()
        for size in SIZES:
            assert not np.any(e.get_sip(0, size)), size
        # the next call lands as on a fresh ring (the oracle has no flush_rxa: a fresh channel, whose filters start from zeros too)
        os_[0].close()
        os_[0] = oracle_channel(oracle, 0, 1)
        fixed(os_[0])
        _follow(e, [os_[0]], x[:, 7 * 1024:], (5,))
        # refusals: `out` untouched
        out = np.full(2 * 4097, 7.0)
        for size in (4097, -1):
            assert lib.qh_rxa_get_sip(e._h, 0, out.ctypes.data, size) == -2      # QH_ERR_INVALID
            assert np.all(out == 7.0)
        assert lib.qh_rxa_get_sip(e._h, 1, out.ctypes.data, 16) == -2            # channel 1's siphon is off
        assert np.all(out == 7.0)
    finally:
        e.close()
        for o in os_:
            o.close()
