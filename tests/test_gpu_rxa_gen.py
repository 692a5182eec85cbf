"""gen0 in the batched RXA engine (xgen, RXA.c:565) on the bare chain (rxa_gen_util.bare), against the literal restatement of wdsp/gen.c
(tests/wdsp_gen_ref.py): every mode over ragged calls, the setters that reset a mode's state, flush_gen's quirk, and this project's
noise generator against its own restatement.  -m gpu.

Measured on an MI355X (the printed figures; bound 1e-6 both ways): see DESIGN.md section 7, b20."""
import numpy as np
import pytest

from rxa_gen_util import RATE, bare, hold, ref, run, runs
from wdsp_gen_ref import default_seed, noise

pytestmark = pytest.mark.gpu
CALLS = (1, 3, 5, 2, 7)                     # DSP blocks per call


def _engine(qh, modes, dsp_size=64):
    e = bare(qh, len(modes), dsp_size)
    for c, m in enumerate(modes):
        e.SetRXAPreGenMode(c, m)
        e.SetRXAPreGenRun(c, 1)
    return e


def test_tone_and_a_frequency_change_resets_the_phase(qh):
    e = _engine(qh, [0, 0, 0])
    g = [ref(64, 0), ref(64, 0), ref(64, 0)]
    try:
        e.SetRXAPreGenToneMag(0, 0.5); e.SetRXAPreGenToneFreq(0, 700.0)
        e.SetRXAPreGenToneFreq(1, -1250.0)
        g[0].SetToneMag(0.5); g[0].SetToneFreq(700.0); g[1].SetToneFreq(-1250.0)
        got = [runs(e, CALLS)]
        want = [np.array([q.blocks(sum(CALLS)) for q in g])]
        e.SetRXAPreGenToneFreq(0, 700.0)                        # calc_tone: phase 0 again, mid-run
        e.SetRXAPreGenToneMag(1, 0.125)                         # (a magnitude leaves the phase alone)
        g[0].SetToneFreq(700.0); g[1].SetToneMag(0.125)
        got.append(runs(e, CALLS))
        want.append(np.array([q.blocks(sum(CALLS)) for q in g]))
        got, want = np.concatenate(got, 1), np.concatenate(want, 1)
        for c in range(3):
            hold(got[c], want[c], "tone ch %d" % c)
        assert got[0][sum(CALLS) * 64] == complex(0.5, -0.0)
    finally:
        e.close()


def test_two_tone_defaults(qh):
    e = _engine(qh, [1, 1], dsp_size=256)
    try:
        got = runs(e, CALLS)
        want = ref(256, 1).blocks(sum(CALLS))
        hold(got[0], want, "two-tone ch 0")
        hold(got[1], want, "two-tone ch 1")
    finally:
        e.close()


SWEEPS = {"tie": (-2000.0, 2000.0, 400000.0), "no tie": (-2000.0, 2001.7, 400000.0), "never resets": (0.0, 1000.0, -5000.0),
          "always resets": (1000.0, 0.0, 5000.0)}


def test_sweeps_across_resets_and_a_restart_mid_run(qh):
    """the four small sweeps on four channels over 1728 samples (three resets and more of the 481-sample periods), then SetRXAPreGenSweepFreq
    on channels 0 and 2 and SetRXAPreGenSweepRate on 1 and 3 restart them from phase and position 0 in the middle of a period"""
    names = list(SWEEPS)
    e = _engine(qh, [3] * 4)
    g = [ref(64, 3) for _ in names]
    calls = (1, 3, 5, 7, 11)
    try:
        for c, k in enumerate(names):
            f1, f2, r = SWEEPS[k]
            e.SetRXAPreGenSweepMag(c, 0.5 + 0.1 * c); e.SetRXAPreGenSweepFreq(c, f1, f2); e.SetRXAPreGenSweepRate(c, r)
            g[c].SetSweepMag(0.5 + 0.1 * c); g[c].SetSweepFreq(f1, f2); g[c].SetSweepRate(r)
        got = [runs(e, calls)]
        want = [np.array([q.blocks(sum(calls)) for q in g])]
        for c, k in enumerate(names):
            f1, f2, r = SWEEPS[k]
            if c % 2 == 0:
                e.SetRXAPreGenSweepFreq(c, f1 + 100.0, f2 + 100.0); g[c].SetSweepFreq(f1 + 100.0, f2 + 100.0)
            else:
                e.SetRXAPreGenSweepRate(c, 1.5 * r); g[c].SetSweepRate(1.5 * r)
        got.append(runs(e, calls))
        want.append(np.array([q.blocks(sum(calls)) for q in g]))
        got, want = np.concatenate(got, 1), np.concatenate(want, 1)
        for c, k in enumerate(names):
            hold(got[c], want[c], "sweep, " + k)
    finally:
        e.close()


def test_default_sweep_over_two_resets(qh):
    """2 * 480000 + 4096 samples of the default sweep (-20 kHz to +20 kHz at 4 kHz/s), sample for sample, and the 16 samples around each
    reset on their own.  The reference's chain resets at 480000; a closed form would at 480001 and be off by 2 sin(2 pi 20000 / 48000)
    behind it.  Channel 1 runs the tone beside it."""
    P, n, size = 480000, 2 * 480000 + 4096, 256
    e = _engine(qh, [3, 0], dsp_size=size)
    try:
        calls = (1, 3, 5, 1000, 1757, 1000)
        assert sum(calls) * size == n
        got = runs(e, calls)
        want = ref(size, 3).blocks(n // size)
        hold(got[0], want, "default sweep, %d samples" % n)
        for k in (1, 2):
            hold(got[0][k * P - 8:k * P + 8], want[k * P - 8:k * P + 8], "default sweep around reset %d" % k)
        hold(got[1], ref(size, 0).blocks(n // size), "the tone beside it")
    finally:
        e.close()


def test_pulse_with_calls_cut_inside_its_edges(qh):
    """262144 samples at 48 kHz: OFF 143808, UP 96, ON 48000, DOWN 96, OFF again.  Blocks of 64, calls ending at 143872 (inside UP), 153600
    (inside ON) and 191936 (inside DOWN).  Where the output is exactly zero -- OFF, and ctrans[0] at the head of UP -- must agree sample for
    sample, and Q is zero throughout."""
    e = _engine(qh, [6, 6])
    try:
        calls = (2248, 152, 599, 1097)
        assert sum(calls) * 64 == 262144
        got = runs(e, calls)
        want = ref(64, 6).blocks(4096)
        for c in range(2):
            hold(got[c], want, "pulse ch %d" % c)
            assert np.all(got[c].imag == 0.0)
            assert np.array_equal(got[c].real == 0.0, want.real == 0.0)
        assert np.flatnonzero(want.real)[0] == 143809 and np.flatnonzero(want.real)[-1] == 191999
    finally:
        e.close()


def test_flush_in_the_middle_of_on(qh):
    """qh_rxa_flush (flush_gen, RXA.c:534) 9696 samples into ON: OFF then lasts the 38304 samples ON had left"""
    e = _engine(qh, [6, 0])
    g, t = ref(64, 6), ref(64, 0)
    try:
        got = [runs(e, (2400,))]
        want = [g.blocks(2400)]
        tone = [t.blocks(2400)]
        e.flush(); g.flush()
        got.append(runs(e, (300, 301, 200)))
        want.append(g.blocks(801)); tone.append(t.blocks(801))
        got, want = np.concatenate(got, 1), np.concatenate(want)
        hold(got[0], want, "pulse flushed in ON")
        assert np.array_equal(got[0].real == 0.0, want.real == 0.0)
        assert np.all(want.real[153600:153600 + 38305] == 0.0) and want.real[153600 + 38305] != 0.0
        hold(got[1], np.concatenate(tone), "the tone over the flush (flush_gen leaves its phase alone)")
    finally:
        e.close()


def test_silence_and_switching_modes(qh):
    """mode 99 is silence; a mode that is switched away from keeps its state and resumes where it stopped (tone -> sweep -> tone ->
    pulse -> noise -> silence -> tone), and a generator that is switched off passes the chain's own signal (zeros here)"""
    e = _engine(qh, [0, 99])
    g = ref(64, 0)
    try:
        e.SetRXAPreGenSweepFreq(0, -2000.0, 2000.0); e.SetRXAPreGenSweepRate(0, 400000.0)
        g.SetSweepFreq(-2000.0, 2000.0); g.SetSweepRate(400000.0)
        got, want = [], []
        for mode, calls in ((0, (1, 3)), (3, (5, 4)), (0, (3,)), (6, (2,)), (99, (1,)), (3, (7,)), (0, (5,))):
            e.SetRXAPreGenMode(0, mode); g.SetMode(mode)
            got.append(runs(e, calls)); want.append(g.blocks(sum(calls)))
        got, want = np.concatenate(got, 1), np.concatenate(want)
        hold(got[0], want, "modes switched")
        assert np.all(got[1] == 0.0)
        assert np.all(got[0][18 * 64:19 * 64] == 0.0)           # the block of silence
        e.SetRXAPreGenRun(0, 0)
        assert np.all(run(e, 2) == 0.0)
    finally:
        e.close()


def test_modes_4_and_5_are_refused(qh):
    e = _engine(qh, [0, 0])
    try:
        for m in (4, 5):
            e.SetRXAPreGenMode(1, m)
            with pytest.raises(qh.QuiskHipError):
                run(e, 1)
        e.SetRXAPreGenRun(1, 0)                                 # not running: the mode is only a stored field
        hold(run(e, 2)[0], ref(64, 0).blocks(2), "the tone after the refusals (nothing had run)")
    finally:
        e.close()


# ---- noise: this project's generator (wdsp_gen_ref.noise)
ULP = 2.0 ** -52


def test_noise_against_its_restatement_and_however_the_calls_are_cut(qh):
    """Both sides draw the same uniforms and decide c >= 1 on the same bits; what can differ is log, the division, sqrt and three products,
    each within an ulp on either side: 16 ulps of the sample is the bound (measured: printed).  Eight blocks in one call or in eight
    calls: the same bits.  Channels differ, and seeds do."""
    e, f = _engine(qh, [2, 2, 2], dsp_size=256), _engine(qh, [2, 2, 2], dsp_size=256)
    try:
        for q in (e, f):
            q.SetRXAPreGenNoiseMag(-1, 0.25)
            q.set_gen_seed(2, 12345)
        one = run(e, 8)
        eight = runs(f, (1,) * 8)
        assert np.array_equal(one, eight)
        more = run(e, 3)
        for c, seed in enumerate((default_seed(0), default_seed(1), 12345)):
            want = noise(seed, c, 0, 11 * 256, 0.25)
            got = np.concatenate([one[c], more[c]])
            err = max(np.abs(got.real - want.real) / np.abs(want.real), np.abs(got.imag - want.imag) / np.abs(want.imag), key=np.max).max()
            print("noise ch %d: largest error %.3g ulps of the sample" % (c, err / ULP))
            assert err <= 16 * ULP, (c, err)
        assert not np.array_equal(one[0], one[1]) and not np.array_equal(one[0], one[2])
        e.set_gen_seed(0, 12345)                                # channel 0 on channel 2's seed: the stream goes on from the sample it has
        got, want = run(e, 1), noise(12345, 0, 11 * 256, 256, 0.25)     # reached, and the channel is part of the key
        assert np.abs(got[0] - want).max() <= 16 * ULP * np.abs(want).max()
        assert not np.array_equal(got[0], got[2])
    finally:
        e.close(); f.close()


def test_noise_distribution(qh):
    """N = 65536 samples per component at mag 0.25, default seeds, four channels: five standard errors of each statistic under the
    reference's distribution (tests/test_gen_restatement.py holds the restatement to the same)"""
    N, mag = 65536, 0.25
    e = _engine(qh, [2] * 4, dsp_size=256)
    try:
        e.SetRXAPreGenNoiseMag(-1, mag)
        z = runs(e, (1, 3, 5, 247))
        assert z.shape[1] == N
        for c in range(4):
            for x in (z[c].real, z[c].imag):
                assert abs(x.mean()) <= 5.0 * mag / np.sqrt(N)
                assert abs(x.var() / mag ** 2 - 1.0) <= 5.0 * np.sqrt(2.0 / N)
                u = (x - x.mean()) / x.std()
                for lag in range(1, 9):
                    assert abs(np.mean(u[:-lag] * u[lag:])) <= 5.0 / np.sqrt(N), (c, lag)
            assert abs(np.corrcoef(z[c].real, z[c].imag)[0, 1]) <= 5.0 / np.sqrt(N)
    finally:
        e.close()
