"""The SSQL restatement (tests/rxa_ssql_ref.py) against closed forms and its own invariants.  CPU only."""
import numpy as np

from rxa_ssql_ref import DECREASE, INCREASE, MUTED, UNMUTED, Ssql, edges, syllabic

RATE = 48000


def test_ftov_of_a_steady_tone():
    for f in (300.0, 700.0, 1500.0):
        s = Ssql(RATE)
        n = 4 * s.rsize
        x = np.sin(2 * np.pi * f * np.arange(n) / RATE + 0.3)
        out = s.ftov(x)
        assert abs(np.mean(out[s.rsize:]) - f / s.fmax) < 0.02, (f, np.mean(out[s.rsize:]))


def test_slews_end_points():
    s = Ssql(RATE)
    assert s.ntup == s.ntdown == int(0.070 * RATE)
    assert s.cup[0] == s.muted_gain and abs(s.cup[s.ntup] - 1.0) < 1e-15
    assert s.cdown[0] == 1.0 and abs(s.cdown[s.ntdown] - s.muted_gain) < 1e-15
    assert all(b >= a for a, b in zip(s.cup, s.cup[1:]))


def test_state_machine_by_hand():
    s = Ssql(RATE)
    s.ntup = s.ntdown = 2
    s.cup, s.cdown = [0.0, 0.5, 1.0], [1.0, 0.5, 0.0]
    tr = np.array([0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 1, 0, 0], dtype=np.int8)
    g = s.machine(tr)
    # MUTED until the trigger; the trigger sample itself is still muted; up-ramp cup[0..2]; UNMUTED (1, its tr = 0 starts the
    # down-ramp after it); cdown[0..2]; MUTED again, its tr = 1 sample muted, then the next up-ramp
    assert g.tolist() == [0.0, 0.0, 0.0, 0.0, 0.5, 1.0, 1.0, 1.0, 0.5, 0.0, 0.0, 0.0, 0.5]
    assert s.state == INCREASE and s.count == 0


def _chain(blocks, x, rate=RATE):
    s = Ssql(rate, run=1)
    out, pos = [], 0
    for b in blocks:
        out.append(s.process(x[pos:pos + b]))
        pos += b
    return np.concatenate(out), s


def test_block_size_does_not_matter():
    n = 256 * 560
    x = 0.5 * syllabic(n, RATE, seed=1)
    one, s1 = _chain([n], x)
    even, _ = _chain([256] * (n // 256), x)
    rng = np.random.default_rng(2)
    rag, pos = [], 0
    while pos < n:
        b = int(min(rng.integers(1, 5000), n - pos))
        rag.append(b)
        pos += b
    ragged, _ = _chain(rag, x)
    assert np.array_equal(one, even) and np.array_equal(one, ragged)
    op, cl = edges(np.abs(one) > 0)
    assert op >= 1


def test_flush_keeps_window_trigger_and_machine():
    s = Ssql(RATE, run=1)
    s.process(0.5 * syllabic(RATE, RATE, seed=4))
    keep = (s.wdaverage, s.tr_voltage, s.state, s.count)
    s.flush()
    assert (s.wdaverage, s.tr_voltage, s.state, s.count) == keep
    assert s.prev_in == s.prev_out == s.inlast == 0.0 and s.rcount == 0 and not any(s.ring) and not np.any(s.zi)


def test_noise_stays_muted_and_speech_opens_and_closes():
    n = 6 * RATE
    rng = np.random.default_rng(7)
    s = Ssql(RATE, run=1)
    s.process(0.3 * (rng.standard_normal(n) + 1j * rng.standard_normal(n)))
    assert np.all(s.gain[n // 2:] == 0.0) and s.state == MUTED        # once the ring and the window average have filled
    s = Ssql(RATE, run=1)
    s.process(0.5 * syllabic(n, RATE, seed=5))
    op, cl = edges(s.gain)
    assert op >= 2 and cl >= 2, (op, cl)
    assert s.state in (MUTED, INCREASE, UNMUTED, DECREASE)
