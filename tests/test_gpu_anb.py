"""qh_anb_* (WDSP's noise blanker, xanb, wdsp/nob.c:107-187) against the sample-by-sample restatement tests/wdsp_anb_ref.py.

The bank steps the detector's average in time tiles whose start values come from a scan, walks the state machine from event to event
and applies the scale one thread per sample (quisk_amd/csrc/qh_anb.hip); the multiplications are the reference's, on tables from the
same C library, so the gate is np.array_equal wherever the trigger bits agree.  The bits can differ only where a compare sits within
the rounding of the tiled average, eps / (1 - backmult) relative at worst (1e-12 at 192 kHz, 2e-11 at 1.536 MHz with backtau 0.05):
every parity case first asserts, on the restatement alone, a trigger margin of at least 1e-9 -- a condition on the input, not a
tolerance on the output -- and that pulses were found (exact zeros in the reference).  -m gpu."""
import numpy as np
import pytest

from quisk_amd import synth
from wdsp_anb_ref import Anb, run_cuts

pytestmark = pytest.mark.gpu

MARGIN = 1e-9
PARAMS = {
    "typical": dict(tau=1e-4, hangtime=1e-4, advtime=1e-4, backtau=0.05, threshold=30.0),
    "typical20": dict(tau=1e-4, hangtime=1e-4, advtime=1e-4, backtau=0.05, threshold=20.0),
    "limits": dict(tau=0.002, hangtime=1e-4, advtime=0.002, backtau=0.05, threshold=25.0),
    "nohang": dict(tau=1e-4, hangtime=0.0, advtime=1e-4, backtau=0.05, threshold=30.0),
    "dense": dict(tau=1e-4, hangtime=1e-4, advtime=1e-4, backtau=0.05, threshold=1.2),
    "busy": dict(tau=1e-4, hangtime=1e-4, advtime=1e-4, backtau=0.05, threshold=3.0),       # a trigger every thousand samples or so
}
RATES = (48000, 192000, 1536000)


def _input(nch, n, seed, scale=0.8):
    """impulsive_input plus pulses planted across the edges of the detector's tiles (128 samples), the bit words (64) and the walk's
    chunks (4096 samples).  scale 0.8: the mean magnitude of the noise is the average's start value 1.0, so the blanker does not spend
    the first backtau seconds blanking everything."""
    x = synth.impulsive_input(nch, n, seed=seed, scale=scale)
    for c in range(nch):
        for edge in (4096, 8192, 8192 + 64, 12288 - 128, 20480, 20480 + 4096, 30000 // 64 * 64, 36864):
            if edge + 2 < n:
                x[c, edge - 1 - (c % 3):edge + 1 + (c & 1)] += 60.0 * scale * (1 + 0.1 * c)
    return x


def _reference(rate, prm, x, cuts):
    refs, anbs = [], []
    for c in range(x.shape[0]):
        a = Anb(rate, **prm)
        refs.append(run_cuts(a, x[c], cuts))
        anbs.append(a)
    return np.stack(refs), anbs


def _check_input(ref, anbs, what=""):
    for a in anbs:
        print("anb case %s: trigger margin %.3e, %d triggers" % (what, a.margin, a.triggers))
        assert a.margin >= MARGIN, (what, a.margin)
        assert a.triggers > 0
    assert np.count_nonzero(ref == 0) > ref.shape[0] * (anbs[0].delay + 20)          # pulses were found


@pytest.mark.parametrize("rate", RATES)
@pytest.mark.parametrize("name", sorted(PARAMS))
def test_matches_restatement_bit_exact(qh, rate, name):
    prm = PARAMS[name]
    n, nch = 50000, 2
    x = _input(nch, n, seed=rate // 1000 + len(name))
    cuts = [0, 1, 300, 5000, 5001, 23456, n]                    # ragged calls, one of them a single sample
    ref, anbs = _reference(rate, prm, x, cuts)
    _check_input(ref, anbs, "%s@%d" % (name, rate))
    ref1, _ = _reference(rate, prm, x, [0, n])
    assert np.array_equal(ref, ref1)
    nb = qh.WdspNoiseBlanker(nch, rate, **prm)
    assert nb.delay(0) == anbs[0].delay and nb.delay(nch - 1) == anbs[0].delay
    y = np.concatenate([nb.process_host(x[:, a:b]) for a, b in zip(cuts[:-1], cuts[1:])], axis=1)
    diff = np.argwhere(y != ref)
    print("anb case %s@%d: %d samples differ, first %s" % (name, rate, len(diff), diff[:1].tolist()))
    assert np.array_equal(y, ref)
    one = qh.WdspNoiseBlanker(nch, rate, **prm).process_host(x)         # ... against one call
    assert np.array_equal(one, ref)


def test_calls_shorter_than_the_delay(qh):
    rate, prm = 1536000, PARAMS["limits"]
    n = 30000
    x = _input(1, n, seed=41)
    cuts = list(range(0, 2000, 1)) [:40] + list(range(2000, n, 1777)) + [n]     # forty calls of one sample, then calls shorter than T = 6144
    ref, anbs = _reference(rate, prm, x, cuts)
    _check_input(ref, anbs, "short calls")
    nb = qh.WdspNoiseBlanker(1, rate, **prm)
    assert nb.delay() == 6144
    y = np.concatenate([nb.process_host(x[:, a:b]) for a, b in zip(cuts[:-1], cuts[1:])], axis=1)
    assert np.array_equal(y, ref)


SETS = [PARAMS["typical"], PARAMS["limits"], PARAMS["nohang"], PARAMS["dense"], PARAMS["busy"]]


def _mixed_bank(qh, rate):
    nb = qh.WdspNoiseBlanker(len(SETS), rate, **SETS[0])
    for c, p in enumerate(SETS):
        nb.set_tau(p["tau"], c); nb.set_hangtime(p["hangtime"], c); nb.set_advtime(p["advtime"], c)
        nb.set_backtau(p["backtau"], c); nb.set_threshold(p["threshold"], c)
    return nb


def test_channels_with_different_settings_in_one_bank(qh):
    rate, n = 192000, 40000
    x = _input(len(SETS), n, seed=77)
    cuts = [0, 7, 9000, 9001, 26000, n]
    refs, anbs = [], []
    for c, p in enumerate(SETS):
        a = Anb(rate, **p)
        refs.append(run_cuts(a, x[c], cuts))
        anbs.append(a)
        print("anb mixed ch %d: margin %.3e, %d triggers" % (c, a.margin, a.triggers))
        assert a.margin >= MARGIN and a.triggers > 0
    ref = np.stack(refs)
    assert all(np.count_nonzero(r == 0) > a.delay + 20 for r, a in zip(refs, anbs))
    nb = _mixed_bank(qh, rate)
    assert [nb.delay(c) for c in range(len(SETS))] == [a.delay for a in anbs]
    y = np.concatenate([nb.process_host(x[:, a:b]) for a, b in zip(cuts[:-1], cuts[1:])], axis=1)
    for c in range(len(SETS)):
        assert np.array_equal(y[c], ref[c]), c


@pytest.mark.parametrize("victim", [0, 2, 4])
def test_no_channel_reaches_another(qh, victim):
    """Two banks with the same settings and the same ragged stream; from the third call on the second bank's victim channel gets
    another, 50 dB louder signal and other settings.  Every other channel comes out bit-identical (test_gpu_channel_isolation.py)."""
    rate, n = 192000, 40000
    x = _input(len(SETS), n, seed=5)
    x2 = x.copy()
    rng = np.random.default_rng(victim)
    cuts = [0, 7, 9000, 9001, 26000, n]
    x2[victim, cuts[2]:] = 300.0 * x[victim, cuts[2]:] + 1e3 * rng.standard_normal(n - cuts[2])
    a, b = _mixed_bank(qh, rate), _mixed_bank(qh, rate)
    ya, yb = [], []
    for k, (lo, hi) in enumerate(zip(cuts[:-1], cuts[1:])):
        if k == 2:
            b.set_tau(0.0015, victim); b.set_threshold(3.0, victim); b.set_hangtime(0.003, victim)
        if k == 3:
            b.set_run(0, victim)
        if k == 4:
            b.set_run(1, victim); b.flush(victim)
        ya.append(a.process_host(x[:, lo:hi])); yb.append(b.process_host(x2[:, lo:hi]))
    ya, yb = np.concatenate(ya, axis=1), np.concatenate(yb, axis=1)
    others = [c for c in range(len(SETS)) if c != victim]
    assert np.array_equal(ya[others], yb[others])
    assert not np.array_equal(ya[victim], yb[victim])


def test_setters_run_and_flush_between_calls(qh):
    rate = 192000
    x = _input(1, 60000, seed=13)[0]
    nb, ref = qh.WdspNoiseBlanker(1, rate, **PARAMS["typical"]), Anb(rate, **PARAMS["typical"])
    plan = [(0, 9000, None), (9000, 9100, ("threshold", "SetThreshold", 8.0)), (9100, 20000, ("tau", "SetTau", 3e-4)),
            (20000, 26000, ("run", "SetRun", 0)), (26000, 26050, ("run", "SetRun", 1)), (26050, 33000, ("hangtime", "SetHangtime", 0.0)),
            (33000, 40000, ("flush", "flush", None)), (40000, 47000, ("advtime", "SetAdvtime", 0.0011)), (47000, 53000, ("backtau", "SetBacktau", 0.01)),
            (53000, 60000, ("samplerate", "SetSamplerate", 96000))]
    ys, rs = [], []
    for lo, hi, act in plan:
        if act:
            mine, theirs, v = act
            if v is None:
                nb.flush(); ref.flush()
            else:
                getattr(nb, "set_" + mine)(v); getattr(ref, theirs)(v)
            assert nb.delay() == ref.delay
        ys.append(nb.process_host(x[None, lo:hi])[0]); rs.append(ref.process(x[lo:hi]))
    y, r = np.concatenate(ys), np.concatenate(rs)
    print("anb setters: trigger margin %.3e, %d triggers" % (ref.margin, ref.triggers))
    assert ref.margin >= MARGIN and np.count_nonzero(r == 0) > 500
    assert np.array_equal(y[20000:26000], x[20000:26000])               # run = 0: undelayed copy
    assert np.array_equal(y, r)


def test_quiet_input_is_a_pure_delay(qh):
    rng = np.random.default_rng(3)
    x = np.exp(2j * np.pi * rng.uniform(size=(2, 20000)))                  # |x| = avg's start value: nothing triggers
    nb = qh.WdspNoiseBlanker(2, 192000, **PARAMS["typical"])
    y = nb.process_host(x)
    T = nb.delay()
    assert T == 38 and not np.any(y[:, :T]) and np.array_equal(y[:, T:], x[:, :-T])
    nb.flush()
    assert np.array_equal(nb.process_host(x), y)


def test_refusals_change_nothing(qh):
    L = qh.load()
    ok = dict(samplerate=192000.0, tau=1e-4, hangtime=1e-4, advtime=1e-4, backtau=0.05, threshold=30.0)
    order = ("samplerate", "tau", "hangtime", "advtime", "backtau", "threshold")
    bad = [("tau", -1e-6), ("tau", 0.0021), ("tau", float("nan")), ("advtime", -1e-6), ("advtime", 0.0021), ("samplerate", 0.0),
           ("samplerate", -48000.0), ("samplerate", 1536001.0), ("samplerate", float("nan")), ("backtau", 0.0), ("backtau", -0.05),
           ("backtau", float("inf")), ("backtau", float("nan")), ("threshold", float("inf")), ("threshold", float("nan")), ("hangtime", -1e-6)]
    for k, v in bad:
        args = dict(ok, **{k: v})
        assert not L.qh_anb_create(0, 1, *[args[o] for o in order], None), (k, v)
        with pytest.raises(qh.QuiskHipError):
            qh.WdspNoiseBlanker(1, **args)
    x = _input(2, 20000, seed=3)
    nb, clean = qh.WdspNoiseBlanker(2, **ok), qh.WdspNoiseBlanker(2, **ok)
    y0, c0 = nb.process_host(x[:, :9000]), clean.process_host(x[:, :9000])
    assert np.array_equal(y0, c0)
    for k, v in bad:
        assert getattr(L, "qh_anb_set_" + k)(nb._h, -1, v) == -2, (k, v)            # QH_ERR_INVALID
        assert getattr(L, "qh_anb_set_" + k)(nb._h, 1, v) == -2, (k, v)
    assert L.qh_anb_set_tau(nb._h, 2, 1e-4) == -2 and L.qh_anb_flush(nb._h, -2) == -2
    assert nb.delay(0) == 38 and nb.delay(1) == 38
    assert np.array_equal(nb.process_host(x[:, 9000:]), clean.process_host(x[:, 9000:]))     # no restart, no other setting


def test_overlapping_device_rows_are_refused_and_host_in_place_works(qh):
    import torch
    L = qh.load()
    n = 6000
    x = _input(2, n, seed=9)
    nb = qh.WdspNoiseBlanker(2, 192000, **PARAMS["typical"])
    want = qh.WdspNoiseBlanker(2, 192000, **PARAMS["typical"]).process_host(x)
    d = torch.from_numpy(x).cuda()
    o = torch.empty_like(d)
    torch.cuda.synchronize()
    assert L.qh_anb_process(nb._h, d.data_ptr(), n, d.data_ptr(), n, n) == -2            # in place
    assert L.qh_anb_process(nb._h, d.data_ptr(), n, d.data_ptr() + 16 * (n - 1), n, n) == -2   # one shared sample
    nb.process_ptr(d.data_ptr(), n, o.data_ptr(), n, n)                                    # the refusals left the state alone
    nb.synchronize()
    assert np.array_equal(o.cpu().numpy(), want)
    buf = x.copy()
    inplace = qh.WdspNoiseBlanker(2, 192000, **PARAMS["typical"])
    qh.lib.check(L.qh_anb_process_host(inplace._h, buf.ctypes.data, n, buf.ctypes.data, n, n))
    assert np.array_equal(buf, want)
