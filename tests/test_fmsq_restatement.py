"""The restatement of WDSP's FM squelch (tests/wdsp_fmsq_ref.py) on its own: the state machine by hand, block-size independence, flush
and run semantics, the ready delay, noise against a keyed carrier -- and the margins of every input recipe the GPU tests use, which their
state-for-state comparison rests on.  CPU only."""
import numpy as np
import pytest

from wdsp_fmsq_ref import DECREASE, INCREASE, MUTED, TAIL, UNMUTED, FmLoop, Fmsq, keyed_fm, margins, ready_count

RATE = 48000
CROSS_MARGIN, TAIL_MARGIN = 1e-6, 1e-3
# the recipes of the GPU tests' inputs, here at the dsp rate and without the chain's nbp0 ahead of the loop (the GPU tests that compare
# against the restatement repeat the check on the trigger they really use): tests/test_gpu_rxa_fmsq.py and
# tests/test_gpu_fmsq_isolation_and_replay.py take seeds 3, 7, 11, 17 by channel, a channel listed in start_on beginning on the carrier
# (the second one in the first file); tests/test_gpu_wdsp_fmsq_names.py takes seed 3 with the carrier 1.5 s off / 0.9 s on, 3.4 s long
RECIPES = {"48k": dict(seed=3, rate=48000, seconds=4.2), "96k": dict(seed=3, rate=96000, seconds=4.2),
           "mid_on": dict(seed=7, rate=48000, seconds=4.2, start_on=True), "ch2": dict(seed=11, rate=48000, seconds=4.2),
           "ch3": dict(seed=17, rate=48000, seconds=4.2), "ch3_mid_on": dict(seed=17, rate=48000, seconds=4.2, start_on=True),
           "names": dict(seed=3, rate=48000, seconds=3.4, off=1.5, on=0.9)}


def recipe(name, n=None):
    r = dict(RECIPES[name])
    rate, seconds = r.pop("rate"), r.pop("seconds")
    return keyed_fm(int(seconds * rate) if n is None else n, rate, **r), rate


class _Direct(Fmsq):
    """the machine alone: the `noise` given sample by sample instead of filtered from a trigger"""

    def noise_filter(self, trigger):
        return np.asarray(trigger, dtype=np.float64), np.zeros(len(trigger))


def test_state_machine_by_hand():
    """tiny tables (ntup 2, ntdown 1), averages that follow the input at once (avm = 0), rate 10 so that a tail is 12 samples at most"""
    s = _Direct(10.0, ntup=2, ntdown=1)
    s.run = 1
    s.avm, s.onem_avm, s.longavm, s.onem_longavm = 0.0, 1.0, 0.0, 1.0
    s.ready, s.ramp = 1, 1.0
    #            M    M->I  I    I    I->U  U    U->T  T     T    T->D  D    D->M  M
    noise = [1.0, 0.1, 0.1, 0.1, 0.1, 0.1, 0.8, 0.7, 0.7, 0.7, 0.7, 0.7, 0.7, 0.7]
    x = np.full(len(noise), 2.0 + 1.0j)
    y = s.process(noise, x)
    # longnoise 0.8 at the UNMUTED -> TAIL sample: count = (int)(1.2 * 0.8 * 10) = 9 -> the tail runs 10 more samples; cut here at 7
    assert s.tails == [pytest.approx(9.6)] and s.state == TAIL and s.count == 9 - 7
    assert np.array_equal(s.gain[:7], [0.0, 0.0, s.cup[0], s.cup[1], s.cup[2], 1.0, 1.0]) and s.cup[2] == pytest.approx(1.0)
    assert np.all(y[:2] == 0) and np.all(y[5:] == x[5:])
    y = s.process([0.7, 0.7, 0.7, 0.7, 0.7], x[:5])              # count 2, 1, 0 -> DECREASE (count 1): cdown[0], cdown[1] -> MUTED
    assert np.array_equal(s.gain, [1.0, 1.0, 1.0, s.cdown[0], s.cdown[1]]) and s.state == MUTED and s.count == -1
    s.process([0.1, 0.1, 0.1, 0.1, 0.8, 0.8, 0.5], x[:7])        # up again, a tail, and back to UNMUTED from TAIL below unmute_thresh
    assert s.state == UNMUTED and s.gain[-1] == 1.0
    # not ready: stays muted whatever the noise
    u = _Direct(1000.0, ntup=2, ntdown=1)
    u.run = 1
    u.avm, u.onem_avm = 0.0, 1.0
    u.process([0.0] * 99, np.ones(99, dtype=complex))
    assert u.state == MUTED and not u.ready
    u.process([0.0] * 5, np.ones(5, dtype=complex))
    assert u.ready and u.state != MUTED


@pytest.mark.parametrize("rate", [24000, 48000, 96000, 192000, 44100])
def test_ready_count_is_the_literal_accumulation(rate):
    s = _Direct(float(rate))
    s.run = 1
    n = ready_count(rate)
    s.process(np.zeros(n - 1), np.zeros(n - 1, dtype=complex))
    assert not s.ready
    s.process(np.zeros(1), np.zeros(1, dtype=complex))
    assert s.ready
    assert abs(n - 0.1 * rate) <= 1                              # ... and not taken from rate * 0.1


@pytest.fixture(scope="module")
def keyed():
    """the 48 kHz recipe through the loop: (input, trigger)"""
    z, rate = recipe("48k")
    return z, FmLoop(float(rate)).process(z)


def _chunks(total, sizes):
    pos, k = 0, 0
    while pos < total:
        n = min(sizes[k % len(sizes)], total - pos)
        yield pos, pos + n
        pos += n
        k += 1


def test_block_size_independence(keyed):
    z, trig = keyed
    n = 120000                                                   # through the first opening and closing
    outs = []
    for sizes in ([n], [256], [3 * 256, 256, 17 * 256, 7 * 256, 1]):
        s = Fmsq(RATE, run=1)
        outs.append(np.concatenate([s.process(trig[a:b], z[a:b]) for a, b in _chunks(n, sizes)]))
    assert np.array_equal(outs[0], outs[1]) and np.array_equal(outs[0], outs[2])
    assert np.any(outs[0] == 0) and np.any(outs[0] != 0)


def test_noise_stays_muted_and_a_keyed_carrier_opens_and_closes(keyed):
    z, trig = keyed
    rng = np.random.default_rng(0)
    w = 0.01 * (rng.standard_normal(48000) + 1j * rng.standard_normal(48000))
    s = Fmsq(RATE, run=1)
    y = s.process(FmLoop(float(RATE)).process(w), w)
    # (the filter's empty delay line lets avnoise dip at the very start: what the ready delay is for)
    assert not np.any(y) and s.state == MUTED and s.av[:2000].min() < 0.562 and s.av[4800:].min() > 0.75
    s = Fmsq(RATE, run=1)
    y = s.process(trig, z)
    g = s.gain
    opens = np.flatnonzero((g[:-1] == 0.0) & (g[1:] != 0.0) | (g[:-1] == 0.0) & (np.arange(1, len(g)) == 0))
    assert np.sum((g[1:] == 1.0) & (g[:-1] != 1.0)) >= 3 and np.sum((g[1:] == 0.0) & (g[:-1] != 0.0)) >= 2 and opens.size >= 3
    t = np.arange(len(z)) / RATE
    on = (t % 1.4) >= 0.5
    assert s.av[on & ((t % 1.4) > 0.6)].max() < 0.2 and s.av[~on & ((t % 1.4) > 0.1) & (t > 0.1)].min() > 1.0
    assert len(s.tails) >= 2


def test_flush_and_run_semantics(keyed):
    z, trig = keyed
    a, b = Fmsq(RATE, run=1), Fmsq(RATE, run=1)
    cut = 40000                                                  # on the first carrier, unmuted
    a.process(trig[:cut], z[:cut]); b.process(trig[:cut], z[:cut])
    assert a.state == UNMUTED
    count = a.count
    a.flush()
    assert (a.avnoise, a.longnoise, a.state, a.ready, a.ramp, a.count) == (100.0, 1.0, MUTED, 0, 0.0, count) and not np.any(a.delay)
    y = a.process(trig[cut:cut + 8000], z[cut:cut + 8000])
    n = ready_count(RATE)
    assert not np.any(y[:n - 1]) and np.any(y[n:])               # muted for the ready delay again, then it opens on the carrier
    # run 0: the block as is, and nothing of the state moves (fmsq.c:143,203)
    b.SetRXAFMSQRun(0)
    before = (b.avnoise, b.longnoise, b.state, b.count, b.ready, b.ramp, b.delay.copy())
    y = b.process(trig[cut:cut + 30000], z[cut:cut + 30000])
    assert np.array_equal(y, z[cut:cut + 30000])
    assert before[:6] == (b.avnoise, b.longnoise, b.state, b.count, b.ready, b.ramp) and np.array_equal(before[6], b.delay)
    b.SetRXAFMSQRun(1)
    y = b.process(trig[cut + 30000:cut + 31000], z[cut + 30000:cut + 31000])
    assert b.gain[0] == 1.0                                      # still UNMUTED from before the carrier went: no ramp up
    b.SetRXAFMSQThreshold(0.5)
    assert (b.tail_thresh, b.unmute_thresh) == (0.5, 0.45)
    assert (Fmsq(RATE).tail_thresh, Fmsq(RATE).unmute_thresh) == (0.750, 0.562)


@pytest.mark.parametrize("name", sorted(RECIPES))
def test_margins_of_the_gpu_tests_inputs(name):
    """Every threshold crossing of avnoise keeps both of its samples more than 1e-6 (relative) from the threshold, and every tail count's
    real value lies more than 1e-3 from an integer: the GPU chain's 1e-9 cannot move a decision.  Over the thresholds the GPU tests
    use (the defaults, and SetRXAFMSQThreshold 0.5 / 1.0) and the filters they use (nc 256, 2048, 4096)."""
    z, rate = recipe(name)
    trig = FmLoop(float(rate)).process(z)
    ncs = (2048,) if name != "48k" else (256, 2048, 4096)
    for nc in ncs:
        s = Fmsq(rate, run=1, nc=nc)
        s.process(trig, z)
        cross, tail = margins(s.av, (0.750, 0.562), s.tails)
        print("recipe %s nc %d: crossing margin %.3g, tail margin %.3g, %d tails" % (name, nc, cross, tail, len(s.tails)))
        assert cross > CROSS_MARGIN and tail > TAIL_MARGIN and len(s.tails) >= (1 if name == "names" else 2)
        for thr in (0.5, 1.0):
            s2 = Fmsq(rate, run=1, nc=nc)
            s2.SetRXAFMSQThreshold(thr)
            s2.process(trig, z)
            cross, tail = margins(s2.av, (thr, 0.9 * thr), s2.tails)
            assert cross > CROSS_MARGIN and tail > TAIL_MARGIN, (thr, cross, tail)
