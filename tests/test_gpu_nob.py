"""qh_nob_* (WDSP's second noise blanker, xnob, wdsp/nobII.c:157-495) against the sample-by-sample restatement tests/wdsp_nob_ref.py.

The bank steps the detector's average in time tiles whose start values come from a scan, walks the ten-state machine from event to
event and lets the lanes of the walk write the slews and fills over a delayed copy (quisk_amd/csrc/qh_nob.hip); sums and products are
the reference's in its order, on tables from the same C library, and the mode-4 line is the reference's repeated addition, so the gate
is np.array_equal everywhere, mode-4 fills included.  The flags can differ only where a compare sits within the rounding of the tiled
average, eps / (1 - backmult) relative at worst (1e-12 at 192 kHz, 2e-11 at 1.536 MHz with backtau 0.05): every parity case first
asserts, on the restatement alone, a trigger margin of at least 1e-9 -- a condition on the input, not a tolerance on the output -- and
that the input exercises what the case is for (blanks, merged sequences, the overflow path, reads ahead of the write position).  -m gpu."""
import numpy as np
import pytest

from quisk_amd import synth
from wdsp_nob_ref import Nob, run_cuts

pytestmark = pytest.mark.gpu

MARGIN = 1e-9
PARAMS = {
    "typical": dict(slewtime=1e-4, hangtime=1e-4, advtime=1e-4, backtau=0.05, threshold=30.0),
    "typical20": dict(slewtime=1e-4, hangtime=1e-4, advtime=1e-4, backtau=0.05, threshold=20.0),
    "nohang": dict(slewtime=1e-4, hangtime=0.0, advtime=1e-4, backtau=0.05, threshold=30.0),
    "zeroslew": dict(slewtime=0.0, hangtime=1e-4, advtime=1e-4, backtau=0.05, threshold=30.0),
    "longadv": dict(slewtime=1e-4, hangtime=0.0, advtime=0.002, backtau=0.05, threshold=30.0),     # adv_count > hang_count + 11: the look-ahead passes the write position
    "dense": dict(slewtime=1e-4, hangtime=1e-4, advtime=1e-4, backtau=0.05, threshold=2.0),
    "burst": dict(slewtime=1e-4, hangtime=1e-4, advtime=1e-4, backtau=0.05, threshold=4.0),        # with a 30 ms pulse train in the input
}
RATES = (48000, 192000, 1536000)


def _prm(name, rate):
    """PARAMS[name]; "dense" at 1.536 MHz with threshold 3: at 2 the noise alone holds one sequence open for good (a flag every 23
    samples against a hang of 306) and nothing is left to merge."""
    return dict(PARAMS[name], threshold=3.0) if (name, rate) == ("dense", 1536000) else PARAMS[name]


LENGTH = {48000: 40000, 192000: 40000, 1536000: 150000}


def _train(x, start, seconds, rate, gap, amp):
    stop = min(len(x), start + int(seconds * rate))
    x[start:stop:gap] += amp


def _input(nch, n, seed, rate=192000, name="typical", scale=0.8):
    """impulsive_input (mean magnitude of the noise: the average's start value 1.0) plus pulses planted across the edges of the
    detector's tiles (128 samples), the flag words (64) and 4096-sample chunks; for "burst" a 30 ms train of pulses inside each other's
    hang (one sequence longer than max_imp_seq: the overflow path); for "longadv" a 24.5 ms and a 30 ms train of pulses 0.6 (adv_slew +
    adv) apart (sequences merged by the look-ahead up to max_imp_seq, where it reads beyond the newest sample)."""
    x = synth.impulsive_input(nch, n, seed=seed, scale=scale)
    p = PARAMS[name]
    for c in range(nch):
        for edge in (4096, 8192, 8192 + 64, 12288 - 128, 20480, 20480 + 4096, 30000 // 64 * 64, 36864):
            if edge + 2 < n:
                x[c, edge - 1 - (c % 3):edge + 1 + (c & 1)] += 60.0 * scale * (1 + 0.1 * c)
        if name == "burst":
            gap = max(2, int(p["hangtime"] * rate) + int(p["slewtime"] * rate))
            _train(x[c], n // 4 + 17 * c, 0.030, rate, gap, 100.0)
        if name == "longadv":
            gap = int(0.6 * (int(p["advtime"] * rate) + int(p["slewtime"] * rate)))
            _train(x[c], n // 30 + 5 * c, 0.0245, rate, gap, 400.0)
            _train(x[c], n // 3 + 5 * c, 0.030, rate, gap, 400.0)
    return x


def _reference(rate, mode, prm, x, cuts):
    refs, nobs = [], []
    for c in range(x.shape[0]):
        a = Nob(rate, mode, **prm)
        refs.append(run_cuts(a, x[c], cuts))
        nobs.append(a)
    return np.stack(refs), nobs


def _check_input(nobs, name="", what=""):
    for a in nobs:
        print("nob case %s: trigger margin %.3e, %d triggers, %d blanks, %d merges, %d overflows, %d reads ahead" %
              (what, a.margin, a.triggers, a.blanks, a.merges, a.overflows, a.read_ahead))
        assert a.margin >= MARGIN, (what, a.margin)
        assert a.triggers > 0 and a.blanks > 0
        if name == "dense":
            assert a.merges > 0
        if name == "burst":
            assert a.overflows > 0
        if name == "longadv":
            assert a.read_ahead > 0 and a.merges > 0


def _cuts(n):
    return [0, 1, 300, 5000, 5001, 23456, n]                    # ragged calls, one of them a single sample, most shorter than the delay


def _case(rate, name, mode):
    n, nch = LENGTH[rate], 2
    x = _input(nch, n, seed=rate // 1000 + len(name) + mode, rate=rate, name=name)
    ref, nobs = _reference(rate, mode, _prm(name, rate), x, _cuts(n))
    return x, ref, nobs


@pytest.mark.parametrize("mode", range(5))
@pytest.mark.parametrize("rate", RATES)
@pytest.mark.parametrize("name", sorted(PARAMS))
def test_matches_restatement_bit_exact(qh, rate, name, mode):
    prm = _prm(name, rate)
    x, ref, nobs = _case(rate, name, mode)
    nch, n = x.shape
    cuts = _cuts(n)
    _check_input(nobs, name, "%s@%d mode %d" % (name, rate, mode))
    nb = qh.WdspNoiseBlanker2(nch, rate, mode, **prm)
    assert nb.delay(0) == nobs[0].delay and nb.delay(nch - 1) == nobs[0].delay
    y = np.concatenate([nb.process_host(x[:, a:b]) for a, b in zip(cuts[:-1], cuts[1:])], axis=1)
    diff = np.argwhere(y != ref)
    print("nob case %s@%d mode %d: %d samples differ, first %s" % (name, rate, mode, len(diff), diff[:1].tolist()))
    assert np.array_equal(y, ref)
    one = qh.WdspNoiseBlanker2(nch, rate, mode, **prm).process_host(x)   # ... against one call
    assert np.array_equal(one, ref)


def test_one_sample_calls_and_calls_shorter_than_the_delay(qh):
    rate, prm, mode = 192000, PARAMS["typical"], 4
    n = 30000
    x = _input(1, n, seed=41)
    cuts = list(range(40)) + list(range(40, n, 1777)) + [n]              # forty calls of one sample, then calls shorter than D = 4887
    ref, nobs = _reference(rate, mode, prm, x, cuts)
    _check_input(nobs, what="short calls")
    nb = qh.WdspNoiseBlanker2(1, rate, mode, **prm)
    assert nb.delay() == 4887
    y = np.concatenate([nb.process_host(x[:, a:b]) for a, b in zip(cuts[:-1], cuts[1:])], axis=1)
    assert np.array_equal(y, ref)


SETS = [("typical", 0), ("longadv", 4), ("nohang", 1), ("dense", 2), ("zeroslew", 3), ("burst", 4)]


def _mixed_bank(qh, rate):
    nb = qh.WdspNoiseBlanker2(len(SETS), rate, 0, **PARAMS["typical"])
    for c, (name, mode) in enumerate(SETS):
        p = PARAMS[name]
        nb.set_tau(p["slewtime"], c); nb.set_hangtime(p["hangtime"], c); nb.set_advtime(p["advtime"], c)
        nb.set_backtau(p["backtau"], c); nb.set_threshold(p["threshold"], c); nb.set_mode(mode, c)
    return nb


def _mixed_input(n, seed, rate):
    return np.stack([_input(1, n, seed=seed + c, rate=rate, name=name)[0] for c, (name, _) in enumerate(SETS)])


def test_channels_with_different_settings_and_modes_in_one_bank(qh):
    rate, n = 192000, 40000
    x = _mixed_input(n, 77, rate)
    cuts = [0, 7, 9000, 9001, 26000, n]
    refs, nobs = [], []
    for c, (name, mode) in enumerate(SETS):
        a = Nob(rate, mode, **PARAMS[name])
        refs.append(run_cuts(a, x[c], cuts))
        nobs.append(a)
        _check_input([a], name, "mixed ch %d" % c)
    nb = _mixed_bank(qh, rate)
    assert [nb.delay(c) for c in range(len(SETS))] == [a.delay for a in nobs]
    y = np.concatenate([nb.process_host(x[:, a:b]) for a, b in zip(cuts[:-1], cuts[1:])], axis=1)
    for c in range(len(SETS)):
        assert np.array_equal(y[c], refs[c]), c


@pytest.mark.parametrize("victim", [0, 2, 5])
def test_no_channel_reaches_another(qh, victim):
    """Two banks with the same settings and the same ragged stream; from the third call on the second bank's victim channel gets
    another, 50 dB louder signal and other settings.  Every other channel comes out bit-identical."""
    rate, n = 192000, 40000
    x = _mixed_input(n, 5, rate)
    x2 = x.copy()
    rng = np.random.default_rng(victim)
    cuts = [0, 7, 9000, 9001, 26000, n]
    x2[victim, cuts[2]:] = 300.0 * x[victim, cuts[2]:] + 1e3 * rng.standard_normal(n - cuts[2])
    a, b = _mixed_bank(qh, rate), _mixed_bank(qh, rate)
    ya, yb = [], []
    for k, (lo, hi) in enumerate(zip(cuts[:-1], cuts[1:])):
        if k == 2:
            b.set_tau(0.0015, victim); b.set_threshold(3.0, victim); b.set_hangtime(0.001, victim); b.set_mode(2, victim)
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
    x = _input(1, 110000, seed=13)[0]
    x[30000:30002] += 70.0                                                 # a pulse whose blank the call boundary at 34880 cuts
    nb, ref = qh.WdspNoiseBlanker2(1, rate, 1, **PARAMS["typical"]), Nob(rate, 1, **PARAMS["typical"])
    D = ref.delay
    plan = [(0, 9000, None), (9000, 9100, ("threshold", "SetThreshold", 8.0)), (9100, 20000, ("mode", "SetMode", 4)),
            (20000, 30000 + D - 7, ("mode", "SetMode", 2)), (30000 + D - 7, 42000, ("mode", "SetMode", 0)),      # ... during a blank
            (42000, 48000, ("run", "SetRun", 0)), (48000, 48050, ("run", "SetRun", 1)), (48050, 56000, ("tau", "SetTau", 3e-4)),
            (56000, 66000, ("hangtime", "SetHangtime", 0.0)), (66000, 74000, ("flush", "flush", None)),
            (74000, 84000, ("advtime", "SetAdvtime", 0.0011)), (84000, 94000, ("backtau", "SetBacktau", 0.01)),
            (94000, 110000, ("samplerate", "SetSamplerate", 96000))]
    ys, rs = [], []
    for lo, hi, act in plan:
        if act:
            mine, theirs, v = act
            if v is None:
                nb.flush(); ref.flush()
            else:
                getattr(nb, "set_" + mine)(v); getattr(ref, theirs)(v)
            assert nb.delay() == ref.delay
            if lo == 30000 + D - 7:
                assert ref.state in (2, 3)                                  # the mode changes inside a fill
        ys.append(nb.process_host(x[None, lo:hi])[0]); rs.append(ref.process(x[lo:hi]))
    y, r = np.concatenate(ys), np.concatenate(rs)
    print("nob setters: trigger margin %.3e, %d triggers, %d blanks" % (ref.margin, ref.triggers, ref.blanks))
    assert ref.margin >= MARGIN and ref.blanks > 20
    assert np.array_equal(y[42000:48000], x[42000:48000])               # run = 0: undelayed copy
    diff = np.flatnonzero(y != r)
    print("nob setters: %d samples differ, first %s" % (len(diff), diff[:1].tolist()))
    assert np.array_equal(y, r)


def test_quiet_input_is_a_pure_delay(qh):
    rng = np.random.default_rng(3)
    x = np.exp(2j * np.pi * rng.uniform(size=(2, 20000)))                  # |x| = avg's start value: nothing triggers
    nb = qh.WdspNoiseBlanker2(2, 192000, 2, **PARAMS["typical"])
    y = nb.process_host(x)
    D = nb.delay()
    assert D == 4887 and not np.any(y[:, :D]) and np.array_equal(y[:, D:], x[:, :-D])
    nb.flush()
    assert np.array_equal(nb.process_host(x), y)


def test_refusals_change_nothing(qh):
    L = qh.load()
    ok = dict(samplerate=192000.0, mode=4, slewtime=1e-4, hangtime=1e-4, advtime=1e-4, backtau=0.05, threshold=30.0)
    order = ("samplerate", "mode", "slewtime", "hangtime", "advtime", "backtau", "threshold")
    setter = dict(slewtime="tau")
    bad = [("slewtime", -1e-6), ("slewtime", 0.0021), ("slewtime", float("nan")), ("advtime", -1e-6), ("advtime", 0.0021), ("advtime", float("nan")),
           ("hangtime", -1e-6), ("hangtime", 0.0021), ("hangtime", float("inf")), ("samplerate", 0.0), ("samplerate", -48000.0),
           ("samplerate", 1536001.0), ("samplerate", float("nan")), ("backtau", 0.0), ("backtau", -0.05), ("backtau", float("inf")),
           ("backtau", float("nan")), ("threshold", float("inf")), ("threshold", float("nan")), ("mode", -1), ("mode", 5)]
    for k, v in bad:
        args = dict(ok, **{k: v})
        assert not L.qh_nob_create(0, 1, *[args[o] for o in order], None), (k, v)
        with pytest.raises(qh.QuiskHipError):
            qh.WdspNoiseBlanker2(1, **args)
    # the reference's own overrun: every time at its maximum at 1.536 MHz puts the write position beyond the ring
    top = dict(ok, samplerate=1536000.0, slewtime=0.002, hangtime=0.002, advtime=0.002)
    assert not L.qh_nob_create(0, 1, *[top[o] for o in order], None)
    near = qh.WdspNoiseBlanker2(1, **dict(top, hangtime=0.0019))
    assert near.delay() == 4 * 3072 - 154 + 1 + 38400 + 10 < 50690
    assert L.qh_nob_set_hangtime(near._h, 0, 0.002) == -2 and near.delay() == 4 * 3072 - 154 + 1 + 38400 + 10
    x = _input(2, 20000, seed=3)
    nb, clean = qh.WdspNoiseBlanker2(2, **ok), qh.WdspNoiseBlanker2(2, **ok)
    y0, c0 = nb.process_host(x[:, :9000]), clean.process_host(x[:, :9000])
    assert np.array_equal(y0, c0)
    for k, v in bad:
        assert getattr(L, "qh_nob_set_" + setter.get(k, k))(nb._h, -1, v) == -2, (k, v)            # QH_ERR_INVALID
        assert getattr(L, "qh_nob_set_" + setter.get(k, k))(nb._h, 1, v) == -2, (k, v)
    assert L.qh_nob_set_tau(nb._h, 2, 1e-4) == -2 and L.qh_nob_flush(nb._h, -2) == -2
    assert nb.delay(0) == 4887 and nb.delay(1) == 4887
    assert np.array_equal(nb.process_host(x[:, 9000:]), clean.process_host(x[:, 9000:]))     # no restart, no other setting


def test_device_rows_with_strides_and_in_place(qh):
    import torch
    L = qh.load()
    n, stride_in, stride_out = 12000, 12100, 12345
    x = _input(2, n, seed=9)
    want = qh.WdspNoiseBlanker2(2, 192000, 4, **PARAMS["dense"]).process_host(x)
    ref, nobs = _reference(192000, 4, PARAMS["dense"], x, [0, n])
    _check_input(nobs, "dense", "device rows")
    assert np.array_equal(want, ref)
    nb = qh.WdspNoiseBlanker2(2, 192000, 4, **PARAMS["dense"])
    d = torch.zeros((2, stride_in), dtype=torch.complex128, device="cuda")
    d[:, :n] = torch.from_numpy(x).cuda()
    o = torch.full((2, stride_out), float("nan"), dtype=torch.complex128, device="cuda")
    torch.cuda.synchronize()
    # rows that share a byte with the input rows are refused (an output is the input D samples back) and leave the state alone
    assert L.qh_nob_process(nb._h, d.data_ptr(), stride_in, d.data_ptr(), stride_in, n) == -2
    assert L.qh_nob_process(nb._h, d.data_ptr(), stride_in, d.data_ptr() + 16 * (n - 1), stride_in, n) == -2
    for lo, hi in ((0, 5000), (5000, n)):
        nb.process_ptr(d.data_ptr() + 16 * lo, stride_in, o.data_ptr() + 16 * lo, stride_out, hi - lo)
    nb.synchronize()
    got = o.cpu().numpy()
    assert np.array_equal(got[:, :n], want) and np.all(np.isnan(got[:, n:]))
    assert np.array_equal(d[:, :n].cpu().numpy(), x)
    buf = x.copy()                                                          # the host form in place
    inplace = qh.WdspNoiseBlanker2(2, 192000, 4, **PARAMS["dense"])
    qh.lib.check(L.qh_nob_process_host(inplace._h, buf.ctypes.data, n, buf.ctypes.data, n, n))
    assert np.array_equal(buf, want)


def _crowded_input(n, seed=0):
    """Unit-magnitude samples, every one a flag at threshold 0.5, but for a quiet one (magnitude 0.1) every 30000 samples."""
    rng = np.random.default_rng(seed)
    x = np.exp(2j * np.pi * rng.uniform(size=n)) * (1.0 + 0.05 * rng.uniform(size=n))
    x[20000::30000] *= 0.1
    return x


def test_forward_gather_stops_after_one_turn_of_the_ring(qh):
    """Fewer than ten slots of the ring without a flag: the forward gather ends after one turn with zeros for the taps it has not
    found (the reference's loop would not return).  Mode 3, the forward sum alone: the backward taps of the bank come from the
    history it keeps, those of the reference from bfbuff, which may be older than the ring (include/quiskhip.h, qh_nob_create)."""
    rate, mode, n = 1536000, 3, 160000
    prm = dict(slewtime=0.0, hangtime=0.0, advtime=0.0, backtau=0.05, threshold=0.5)
    x = _crowded_input(n)
    cuts = [0, 1, 50000, 58411, 58412, 120000, n]
    ref = Nob(rate, mode, **prm)
    r = run_cuts(ref, x, cuts)
    print("nob crowded ring: trigger margin %.3e, %d blanks, %d overflows, %d short gathers" % (ref.margin, ref.blanks, ref.overflows, ref.short_gathers))
    assert ref.margin >= MARGIN and ref.blanks >= 4 and ref.overflows == 0 and ref.short_gathers >= 2
    nb = qh.WdspNoiseBlanker2(1, rate, mode, **prm)
    y = np.concatenate([nb.process_host(x[None, a:b])[0] for a, b in zip(cuts[:-1], cuts[1:])])
    assert np.array_equal(y, r)
