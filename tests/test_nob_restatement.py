"""tests/wdsp_nob_ref.py, the sample-by-sample restatement of WDSP's second noise blanker (xnob, wdsp/nobII.c:157-495), pinned on behaviour
derived by hand from the reference: the counts and the delay, the span of one blank and what fills it in every mode, which pulses merge,
the overflow path, run = 0, which setters start the blanker over, and calls of any length.  No GPU."""
import numpy as np
import pytest

from wdsp_nob_ref import FCOEFS, Nob, run_cuts

RATE = 192000
TYP = dict(slewtime=1e-4, hangtime=1e-4, advtime=1e-4, backtau=0.05, threshold=30.0)


def _quiet(n, seed=1):
    rng = np.random.default_rng(seed)
    ph = rng.uniform(0, 2 * np.pi, n)
    return (1.0 + 0.01 * rng.standard_normal(n)) * np.exp(1j * ph)        # |x| near avg's start value 1.0: nothing triggers


@pytest.mark.parametrize("rate,count,mseq,delay", [(48000, 4, 1200, 1227), (192000, 19, 4800, 4887), (1536000, 153, 38400, 39023)])
def test_counts_and_delay(rate, count, mseq, delay):
    a = Nob(rate, 0, **TYP)
    assert a.counts == (count, count, count, count, mseq)
    assert a.delay == delay == 4 * count + 1 + mseq + 10
    assert a.dline_size == 50690
    assert len(a.awave) == count and len(a.hwave) == count and a.hwave[0] == 0.5 and 0.0 < a.awave[0] < 0.5


def test_the_reference_overruns_its_ring_at_the_limits():
    with pytest.raises(ValueError):
        Nob(1536000, 0, 0.002, 0.002, 0.002, 0.05, 30.0)                    # D = 4 * 3072 + 1 + 38400 + 10 = 50699 >= 50690
    assert Nob(1536000, 0, 0.002, 0.0019, 0.002, 0.05, 30.0).delay < 50690


def test_quiet_input_is_a_pure_delay():
    a = Nob(RATE, 2, **TYP)
    x = _quiet(12000)
    y = a.process(x)
    D = a.delay
    assert a.triggers == 0 and a.blanks == 0
    assert not np.any(y[:D]) and np.array_equal(y[D:], x[:-D])


def _fir(taps):
    i = q = 0.0
    for c, v in zip(FCOEFS, taps):
        i += c * v.real
        q += c * v.imag
    return complex(i, q)


@pytest.mark.parametrize("mode", range(5))
def test_one_isolated_pulse(mode):
    a = Nob(RATE, mode, **TYP)
    asl, adv, hang, hsl, mseq = a.counts                                     # 19 each
    D = a.delay
    x = _quiet(16000)
    t = 3000
    x[t] = 500.0
    y = a.process(x)
    assert (a.triggers, a.blanks, a.merges, a.overflows, a.read_ahead) == (1, 1, 0, 0, 0) and a.state == 0
    # the flag comes under the scan point adv_slew + adv + 1 samples before the pulse's image leaves: the set-up sample o0 still passes
    o0 = t + D - (asl + adv + 1)
    blank = (hang + hsl + 1) - hsl                                           # the impulse and its hang, less the closing slew
    f0, f1 = o0 + 1 + asl, o0 + 1 + asl + adv + blank                        # the fill: [f0, f1); the pulse's image t + D lies inside
    assert f0 + adv == t + D and f1 - f0 == adv + blank == 39
    assert np.array_equal(y[D:o0 + 1], x[:o0 + 1 - D])
    assert np.array_equal(y[f1 + hsl:], x[f1 + hsl - D:-D])
    i1 = _fir([x[t - adv - 1 - k] for k in range(10)])                       # the clean samples at and before out + adv_slew
    i2 = _fir([x[t + blank + k] for k in range(10)])                         # ... and from scan + blank_count on
    start = {0: 0j, 1: i1, 2: complex(0.5 * (i1.real + i2.real), 0.5 * (i1.imag + i2.imag)), 3: i2, 4: i1}[mode]
    if mode < 4:
        assert np.all(y[f0:f1] == start)
        end = start
    else:
        di, dq = (i2.real - i1.real) / (adv + blank), (i2.imag - i1.imag) / (adv + blank)
        assert a.fills[0][7:] == (di, dq, adv + blank)
        v, w = i1.real, i1.imag
        for k in range(f0, f1):                                              # repeated addition, not I1 + k * delta
            assert y[k] == complex(v, w)
            v += di
            w += dq
        end = complex(v, w)
        assert abs(end - i2) < 1e-12 and y[f0] == i1
    last, nxt = x[o0 - D], x[t + hang + hsl + 1]                             # Ilast; Inext: the first sample behind the blank
    for k in range(asl):
        s = 0.5 + a.awave[k]
        assert y[o0 + 1 + k] == complex(last.real * s + (1.0 - s) * start.real, last.imag * s + (1.0 - s) * start.imag)
    for k in range(hsl):
        s = 0.5 - a.hwave[k]
        assert y[f1 + k] == complex(nxt.real * s + (1.0 - s) * end.real, nxt.imag * s + (1.0 - s) * end.imag)
    assert nxt == x[f1 + hsl - D]                                            # the rise ends on the sample that passes next


def test_pulses_closer_than_the_advance_merge_and_farther_do_not():
    base = Nob(RATE, 0, **TYP)
    asl, adv, hang, hsl, mseq = base.counts
    t, D = 3000, base.delay
    reach = (hang + hsl + 1) + (asl + adv)                                    # the look-ahead's last sample is t + reach - 1

    def run(gap):
        a = Nob(RATE, 0, **TYP)
        x = _quiet(16000)
        x[t] = 500.0
        x[t + gap] = 500.0
        return a, a.process(x), x
    a, y, x = run(reach - 1)
    assert (a.triggers, a.blanks, a.merges) == (2, 1, 1)
    z = np.flatnonzero(y[D:] == 0) + D
    # one hole over both: adv_count + blank_count zeros and the rise's first sample (0.5 - hwave[0] is 0)
    assert len(z) == z[-1] - z[0] + 1 and len(z) == adv + (reach + hang + hsl + 1 - hsl) + 1
    a, y, x = run(hang + hsl)                                                 # inside the first one's hang: one sequence, nothing to merge
    assert (a.triggers, a.blanks, a.merges) == (2, 1, 0)
    a, y, x = run(reach + 200)
    assert (a.triggers, a.blanks, a.merges) == (2, 2, 0)
    z = np.flatnonzero(y[D:] == 0) + D
    assert len(z) == 2 * (adv + (hang + 1) + 1)                               # two holes of adv_count + blank_count zeros and the rise's first
    # a pulse the look-ahead just misses passes under the scan point while the first blank plays, and is never blanked
    a, y, x = run(reach)
    assert (a.triggers, a.blanks, a.merges) == (2, 1, 0) and y[t + reach + D] == 500.0


def test_a_burst_longer_than_max_imp_seq_takes_the_overflow_path():
    a = Nob(RATE, 1, **TYP)
    asl, adv, hang, hsl, mseq = a.counts
    D = a.delay
    n = 30000
    x = _quiet(n)
    t, length = 6000, int(0.030 * RATE)
    x[t:t + length:30] = 1000.0                                               # every 30 samples: inside each other's hang (38)
    states = []
    y = np.concatenate([a.process(x[k:k + 50]) for k in range(0, n, 50)])
    assert a.overflows == 1 and a.blanks >= 1 and a.state == 0 and a.overflow == 0
    b = Nob(RATE, 1, **TYP)
    for k in range(0, n, 10):
        b.process(x[k:k + 10])
        states.append((b.state, b.overflow))
    seen = [s for s, _ in states]
    assert all(s in seen for s in (5, 6, 7, 8, 9)) and all(o == 1 for s, o in states if s >= 5) and all(o == 0 for s, o in states if s < 5)
    o0 = t + D - (asl + adv + 1)
    last = t + length - 30 + 1                                                # the last pulse
    assert not np.any(y[o0 + 1 + asl:last + D + hang])                        # zeros from the end of the fall over the whole burst
    assert np.array_equal(y[D:o0 + 1], x[:o0 + 1 - D])
    tail = last + D + hang + hsl + 40
    assert np.array_equal(y[tail:], x[tail - D:-D])                           # ... and a pure delay again


def test_run_zero_copies_and_freezes():
    a = Nob(RATE, 4, **TYP)
    x = _quiet(14000)
    x[9000] = 500.0
    y0 = a.process(x[:8000])
    frozen = (a.avg, a.state, a.in_idx, a.out_idx, a.scan_idx, list(a.dline), list(a.imp), list(a.bfbuff))
    a.SetRun(0)
    mid = _quiet(700, seed=9) * 100.0
    assert np.array_equal(a.process(mid), mid)
    assert frozen == (a.avg, a.state, a.in_idx, a.out_idx, a.scan_idx, list(a.dline), list(a.imp), list(a.bfbuff))
    a.SetRun(1)
    y1 = a.process(x[8000:])
    b = Nob(RATE, 4, **TYP)
    assert np.array_equal(np.concatenate([y0, y1]), b.process(x)) and b.blanks == 1


def test_which_setters_restart():
    x = _quiet(6000)
    for name, arg in (("SetTau", 2e-4), ("SetHangtime", 2e-4), ("SetAdvtime", 2e-4), ("SetBacktau", 0.04), ("SetSamplerate", 96000), ("flush", None)):
        a = Nob(RATE, 1, **TYP)
        a.process(x)
        getattr(a, name)(*(() if arg is None else (arg,)))
        assert not any(a.dline) and not any(a.imp) and not any(a.bfbuff) and a.avg == 1.0 and a.state == 0 and a.out_idx == 0, name
        assert a.in_idx == a.delay and a.scan_idx == a.adv_slew_count + a.adv_count + 1, name
        assert not np.any(a.process(x)[:a.delay]), name
    a = Nob(RATE, 1, **TYP)
    a.SetTau(3e-4)
    assert a.adv_slew_count == a.hang_slew_count == 57                        # both slews
    for name, arg in (("SetThreshold", 25.0), ("SetMode", 3), ("SetRun", 1)):
        a = Nob(RATE, 1, **TYP)
        a.process(x)
        getattr(a, name)(arg)
        y = a.process(x)
        assert np.array_equal(y[:a.delay], x[-a.delay:]), name                # the ring kept its samples


def test_a_mode_set_during_a_blank_shows_at_the_next_set_up():
    x = _quiet(20000)
    x[3000] = 500.0
    x[9000] = 500.0
    a, b = Nob(RATE, 1, **TYP), Nob(RATE, 1, **TYP)
    D = a.delay
    cut = 3000 + D - 10                                                       # inside the first blank's fill
    ya = np.concatenate([a.process(x[:cut]), a.process(x[cut:])])
    y0 = b.process(x[:cut])
    assert b.state in (2, 3)
    b.SetMode(0)
    yb = np.concatenate([y0, b.process(x[cut:])])
    first, second = slice(3000 + D - 60, 3000 + D + 80), slice(9000 + D - 60, 9000 + D + 80)
    assert np.array_equal(ya[first], yb[first])                              # I and Q persist
    assert not np.array_equal(ya[second], yb[second]) and np.count_nonzero(yb[second] == 0) == 39 + 1


@pytest.mark.parametrize("mode", [0, 4])
def test_ragged_calls_equal_one_call(mode):
    rng = np.random.default_rng(5)
    n = 30000
    x = _quiet(n, seed=2)
    for p in rng.integers(100, n - 100, size=25):
        x[p:p + int(rng.integers(1, 4))] = 300.0
    one = Nob(RATE, mode, **TYP)
    want = one.process(x)
    assert one.blanks > 10
    cuts = [0, 1, 2, 300, 4887, 4888, 9000, 9001, 20000, n]
    got = Nob(RATE, mode, **TYP)
    assert np.array_equal(run_cuts(got, x, cuts), want)
    assert (got.blanks, got.merges, got.triggers, got.margin) == (one.blanks, one.merges, one.triggers, one.margin)


def test_forward_gather_is_bounded_by_one_turn_of_the_ring():
    """At 1.536 MHz with no slew, hang or advance and threshold 0.5, unit-magnitude input is a flag on every sample but the quiet ones at
    20000 + 30000 k.  The set-up for the sequence 20001 .. 49999 happens at step 58411, when the ring holds samples 7722 .. 58411: the
    gather from 50000 finds 50000 and, past the write position, 20000, then has gone round; the other eight taps are zeros."""
    rng = np.random.default_rng(0)
    n = 100000
    x = np.exp(2j * np.pi * rng.uniform(size=n)) * (1.0 + 0.05 * rng.uniform(size=n))
    x[20000::30000] *= 0.1
    a = Nob(1536000, 3, 0.0, 0.0, 0.0, 0.05, 0.5)
    assert a.delay == 38411
    y = a.process(x)
    assert a.overflows == 0 and a.short_gathers >= 1
    step, _, _, i2, q2, i, q, _, _, count = a.fills[1]
    assert step == 58411 and count == 29999
    want = FCOEFS[0] * x[50000] + FCOEFS[1] * x[20000]
    assert (i2, q2) == (want.real, want.imag) and (i, q) == (i2, q2)
    assert np.all(y[a.delay + 20001:a.delay + 50000] == complex(i, q))
