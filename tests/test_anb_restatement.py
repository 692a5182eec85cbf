"""tests/wdsp_anb_ref.py, the sample-by-sample restatement of WDSP's noise blanker (xanb, wdsp/nob.c:107-187), pinned on the behaviour the
GPU tests lean on: the delay, the shape of one blanking cycle, the stale htime, the re-trigger during the rise, run = 0, and which
setters start the blanker over.  No GPU."""
import numpy as np

from wdsp_anb_ref import Anb

RATE = 192000
TYP = dict(tau=1e-4, hangtime=1e-4, advtime=1e-4, backtau=0.05, threshold=30.0)


def _quiet(n, seed=1):
    rng = np.random.default_rng(seed)
    ph = rng.uniform(0, 2 * np.pi, n)
    return (1.0 + 0.01 * rng.standard_normal(n)) * np.exp(1j * ph)        # |x| near avg's start value 1.0: nothing triggers


def _counts(a):
    return a.trans_count, a.adv_count, a.hang_count, a.trans_count + a.adv_count


def test_counts_and_tables():
    a = Anb(RATE, **TYP)
    assert _counts(a) == (19, 19, 19, 38) and a.delay == 38
    assert len(a.wave) == 20 and a.wave[0] == 0.5 and abs(a.wave[-1] + 0.5) < 1e-15
    assert Anb(48000, 1e-5, 0.0, 0.0, 0.05, 30.0).trans_count == 2       # max(2, ...)
    b = Anb(1536000, 0.002, 1e-4, 0.002, 0.05, 30.0)
    assert b.delay == 6144 == b.dline_size - 1


def test_quiet_input_is_a_pure_delay():
    a = Anb(RATE, **TYP)
    x = _quiet(3000)
    y = a.process(x)
    T = a.delay
    assert a.triggers == 0
    assert not np.any(y[:T]) and np.array_equal(y[T:], x[:-T])


def _scale(y, x, T):
    """y[i] / x[i - T] where both are defined (x has no zeros)"""
    return (y[T:] / x[:-T]).real


def test_one_isolated_pulse():
    a = Anb(RATE, **TYP)
    tc, adv, hang, T = _counts(a)
    x = _quiet(4000)
    t = 1000
    x[t] = 500.0
    y = a.process(x)
    assert a.triggers == 1
    g = np.concatenate([np.zeros(T), _scale(y, x, T)])                     # g[i]: the scale of output sample i
    assert np.array_equal(y[T:t + 1], x[:t + 1 - T])                       # passes through t itself
    fall = np.array([0.5 + a.wave[k] for k in range(tc + 1)])
    assert np.allclose(g[t + 1:t + 2 + tc], fall, rtol=1e-15, atol=0) and fall[0] == 1.0 and abs(fall[-1]) < 1e-15
    z0 = t + 2 + tc                                                         # zeros: the advance, then the hang
    first_hang = hang + 1                                                   # htime starts at 0: ++htime > hang_count after hang + 1 samples
    z1 = z0 + (adv + 1) + first_hang
    assert not np.any(y[z0:z1])
    assert z0 <= t + T < z1                                                 # the pulse's own delayed image falls inside the zeros
    rise = np.array([0.5 - a.wave[k] for k in range(tc + 1)])
    assert np.allclose(g[z1:z1 + tc + 1], rise, rtol=1e-15, atol=0) and rise[-1] == 1.0
    assert np.array_equal(y[z1 + tc + 1:], x[z1 + tc + 1 - T:-T])           # and passes again
    assert a.state == 0 and a.htime == hang + 1


def test_first_hang_is_longer_by_hang_count():
    a = Anb(RATE, **TYP)
    tc, adv, hang, T = _counts(a)
    x = _quiet(6000)
    x[1000] = 500.0
    x[3000] = 500.0
    y = a.process(x)
    assert a.triggers == 2

    def zeros_after(t):
        z0 = t + 2 + tc
        k = z0
        while not y[k]:
            k += 1
        return k - z0
    # (the rise's first scale, 0.5 - wave[0], is zero too)
    assert zeros_after(1000) == (adv + 1) + (hang + 1) + 1
    assert zeros_after(3000) == (adv + 1) + 1 + 1                           # the stale htime = hang + 1 leaves at once
    assert zeros_after(1000) - zeros_after(3000) == hang


def test_retrigger_during_the_rise_restarts_the_fall_from_the_scale_reached():
    a = Anb(RATE, **TYP)
    tc, adv, hang, T = _counts(a)
    x = _quiet(4000)
    t = 1000
    x[t] = 500.0
    rise0 = t + 2 + tc + (adv + 1) + (hang + 1)                             # first sample of the rise
    t2 = rise0 + 5
    x[t2] = 500.0
    y = a.process(x)
    assert a.triggers == 2
    g = np.concatenate([np.zeros(T), _scale(y, x, T)])
    p = 0.5 - a.wave[5]
    assert abs(g[t2] - p) < 1e-15                                            # the rise runs through t2 ...
    fall = np.array([p * (0.5 + a.wave[k]) for k in range(tc + 1)])
    assert np.allclose(g[t2 + 1:t2 + 2 + tc], fall, rtol=1e-14, atol=1e-17)  # ... and the fall starts from the scale reached there
    assert 0.0 < p < 1.0


def test_run_zero_copies_and_freezes():
    a = Anb(RATE, **TYP)
    x = _quiet(3000)
    x[2990] = 500.0
    y0 = a.process(x[:2000])
    frozen = (a.avg, a.count, a.state, a.in_idx, a.out_idx, list(a.dline))
    a.SetRun(0)
    mid = _quiet(700, seed=9) * 100.0
    assert np.array_equal(a.process(mid), mid)
    assert frozen == (a.avg, a.count, a.state, a.in_idx, a.out_idx, list(a.dline))
    a.SetRun(1)
    y1 = a.process(x[2000:])
    b = Anb(RATE, **TYP)
    assert np.array_equal(np.concatenate([y0, y1]), b.process(x))


def test_resetting_setters_zero_the_delay_line_and_threshold_does_not():
    x = _quiet(1000)
    for name, arg in (("SetTau", 2e-4), ("SetHangtime", 2e-4), ("SetAdvtime", 2e-4), ("SetBacktau", 0.04), ("SetSamplerate", 96000), ("flush", None)):
        a = Anb(RATE, **TYP)
        a.process(x)
        a.htime = 7
        getattr(a, name)(*(() if arg is None else (arg,)))
        assert not any(a.dline) and a.avg == 1.0 and a.count == 0 and a.state == 0 and a.power == 1.0, name
        assert a.htime == 7, name                                            # initBlanker does not touch htime
        assert not np.any(a.process(x)[:a.delay]), name
    a = Anb(RATE, **TYP)
    a.process(x)
    a.SetThreshold(25.0)
    y = a.process(x)
    assert np.array_equal(y[:a.delay], x[-a.delay:])                          # the delay line kept its samples
