"""qh_varsamp_* (WDSP's variable-ratio resampler, xvarsamp, wdsp/varsamp.c:124-179) against the sample-by-sample restatement
tests/wdsp_varsamp_ref.py.

The bank walks the control recurrence one lane per channel with the reference's own statements in IEEE doubles and then makes every output
sample on its own (quisk_amd/csrc/qh_varsamp.hip), so the gates are
  counts   np.array_equal with the restatement's, call by call and channel by channel;
  samples  |y - ref| <= (rsize + 4) 2^-52 B per sample, B = sum_j |hs[j]| |x[i - j]| from the restatement: the standard bound of a dot
           product of rsize terms added in any order, taken twice for the two sides, with room for a fused interpolation.  Derived, not
           measured; one step's error in h_offset at delta >= 1e-4 would cost six orders of magnitude more, and no var of the cases is
           closer to 1 than that but var = 1 itself.
-m gpu."""
import functools

import numpy as np
import pytest

from wdsp_varsamp_ref import Varsamp

pytestmark = pytest.mark.gpu

EPS = 2.0 ** -52
N = 5000
# a one-sample call, a second one (no output when down-sampling by two), calls shorter than rsize = 140, one call of 3900 samples whose
# outputs cross fifteen tiles of 256, and an empty call
CUTS = [0, 1, 2, 40, 139, 400, 400, 4300, N]
PAIRS = [(48000, 48000), (48000, 96000), (96000, 48000)]


def _input(nch, n, seed):
    rng = np.random.default_rng(seed)
    t = np.arange(n)
    x = 0.3 * (rng.standard_normal((nch, n)) + 1j * rng.standard_normal((nch, n)))
    for c in range(nch):
        x[c] += np.exp(2j * np.pi * (0.031 + 0.07 * c) * t)
    return x


def _vars(ncalls, nch, seed, lo=0.96, hi=1.04):
    """var per call and channel within [lo, hi], none closer to 1 than 1e-4 but 1 itself (the first call of channel 0)"""
    rng = np.random.default_rng(seed)
    v = rng.uniform(lo, hi, size=(ncalls, nch))
    v[np.abs(v - 1.0) < 1e-4] = 1.0003
    v[0, 0] = 1.0
    return v


def _reference(designs, varmode, x, cuts, var, acts=None):
    """the restatement, channel by channel -> per call a list over channels of (y, B); acts[k]: called on every channel's Varsamp (and its
    index) before call k"""
    refs = [Varsamp(*d[:3], **(d[3] if len(d) > 3 else {}), varmode=varmode) for d in designs]
    calls = []
    for k, (a, b) in enumerate(zip(cuts[:-1], cuts[1:])):
        if acts and acts.get(k):
            for c, r in enumerate(refs):
                acts[k](r, c)
        calls.append([r.process(x[c, a:b], float(var[k][c])) for c, r in enumerate(refs)])
    return calls, refs


def _bank(qh, designs, varmode):
    in_rate, out_rate, R = designs[0][:3]
    vs = qh.WdspVarResampler(len(designs), in_rate, out_rate, R=R, varmode=varmode, **(designs[0][3] if len(designs[0]) > 3 else {}))
    for c, d in enumerate(designs[1:], start=1):
        assert d[2] == R
        if d[:2] != (in_rate, out_rate):
            vs.set_rates(d[0], d[1], ch=c)
    return vs


def _compare(what, calls_ref, calls_gpu, rsizes):
    """counts exactly, samples within the derived bound -> the worst ratio of error to bound"""
    worst = 0.0
    for k, (ref, (y, counts)) in enumerate(zip(calls_ref, calls_gpu)):
        want = [len(r[0]) for r in ref]
        assert np.array_equal(counts, want), (what, k, counts.tolist(), want)
        for c, (yr, B) in enumerate(ref):
            if not len(yr):
                continue
            err = np.abs(y[c, :len(yr)] - yr)
            bound = (rsizes[c] + 4) * EPS * B
            ratio = float(np.max(err / np.maximum(bound, 1e-300)))
            worst = max(worst, ratio)
            assert np.all(err <= bound), (what, k, c, ratio)
    print("varsamp %s: worst |y - ref| / bound %.4f" % (what, worst))
    return worst


def _run(vs, x, cuts, var, acts=None):
    out = []
    for k, (a, b) in enumerate(zip(cuts[:-1], cuts[1:])):
        if acts and acts.get(k):
            acts[k](vs)
        out.append(vs.process_host(x[:, a:b], var[k]))
    return out


@functools.lru_cache(maxsize=None)
def _plain_case(pair, R, varmode):
    designs = [pair + (R,)] * 2
    x = _input(2, N, seed=pair[1] // 1000 + R + varmode)
    var = _vars(len(CUTS) - 1, 2, seed=R + varmode)
    calls, refs = _reference(designs, varmode, x, CUTS, var)
    return designs, x, var, calls, [r.rsize for r in refs]


@pytest.mark.parametrize("varmode", [0, 1])
@pytest.mark.parametrize("R", [64, 1024])
@pytest.mark.parametrize("pair", PAIRS)
def test_matches_restatement(qh, oracle, pair, R, varmode):
    designs, x, var, calls, rsizes = _plain_case(pair, R, varmode)
    if pair == (96000, 48000):
        assert len(calls[1][0][0]) == 0                         # the second one-sample call makes nothing
    assert sum(len(c[0][0]) for c in calls) > 2000
    vs = _bank(qh, designs, varmode)
    assert [vs.rsize(c) for c in range(2)] == rsizes
    got = _run(vs, x, CUTS, var)
    _compare("%s R %d varmode %d" % (pair, R, varmode), calls, got, rsizes)
    for (y, counts), v in zip(got, var):                        # behind a row's count the host form leaves its zeros
        for c in range(2):
            assert not np.any(y[c, counts[c]:])


@pytest.mark.parametrize("varmode", [0, 1])
def test_var_at_the_ends_of_its_range(qh, oracle, varmode):
    """var 0.5 and 2.0, the limits the bank accepts; 384 k -> 48 k (rsize 1120) takes the kernel's window from LDS at var 2 and straight
    from memory at var 1 and 0.5, where 256 outputs span more inputs than the launch's LDS holds"""
    designs = [(48000, 48000, 64), (384000, 48000, 64)]
    cuts = [0, 1, 700, 2600, 2601, N]
    var = np.array([[2.0, 2.0], [2.0, 2.0], [0.5, 1.0], [0.5, 0.5], [1.0003, 2.0]])
    x = _input(2, N, seed=17 + varmode)
    calls, refs = _reference(designs, varmode, x, cuts, var)
    rsizes = [r.rsize for r in refs]
    assert rsizes == [140, 1120]
    got = _run(_bank(qh, designs, varmode), x, cuts, var)
    _compare("var at 0.5 and 2, varmode %d" % varmode, calls, got, rsizes)


def test_channels_of_different_designs_in_one_bank(qh, oracle):
    designs = [(48000, 48000, 64), (48000, 96000, 64), (96000, 48000, 64)]
    x = _input(3, N, seed=5)
    var = _vars(len(CUTS) - 1, 3, seed=6)
    acts_ref = {0: lambda r, c: r.set_bandwidth(300.0, 9000.0) if c == 0 else None}
    calls, refs = _reference(designs, 1, x, CUTS, var, acts_ref)
    rsizes = [r.rsize for r in refs]
    vs = _bank(qh, designs, 1)
    vs.set_bandwidth(300.0, 9000.0, ch=0)
    assert [vs.rsize(c) for c in range(3)] == rsizes == [140, 140, 280]
    _compare("mixed designs", calls, _run(vs, x, CUTS, var), rsizes)


def test_ragged_calls_are_one_call(qh, oracle):
    """varmode 0 and a constant var: the recurrence does not see the cuts, and the sums are the same sums"""
    x = _input(2, N, seed=8)
    a, b = qh.WdspVarResampler(2, 48000, 48000, R=64, varmode=0), qh.WdspVarResampler(2, 48000, 48000, R=64, varmode=0)
    parts = _run(a, x, CUTS, [[0.97, 1.0003]] * (len(CUTS) - 1))
    y1, c1 = b.process_host(x, [0.97, 1.0003])
    assert np.array_equal(np.sum([c for _, c in parts], axis=0), c1)
    for c in range(2):
        assert np.array_equal(np.concatenate([y[c, :cnt[c]] for y, cnt in parts]), y1[c, :c1[c]])


def test_run_flush_and_set_rates_in_mid_stream(qh, oracle):
    designs = [(48000, 48000, 64)] * 2
    cuts = [0, 500, 900, 1300, 2000, 2700, 3400, N]
    x = _input(2, N, seed=21)
    var = _vars(len(cuts) - 1, 2, seed=22)

    def ref_run(v):
        def f(r, c):
            r.run = v
        return f

    acts_ref = {1: ref_run(0), 2: ref_run(1), 3: lambda r, c: r.flush(), 4: lambda r, c: r.set_rates(48000, 96000) if c == 1 else None,
                5: lambda r, c: r.set_rates(96000, 48000) if c == 1 else None, 6: lambda r, c: r.set_bandwidth(-1.0, 8000.0)}
    acts = {1: lambda b: b.set_run(0), 2: lambda b: b.set_run(1), 3: lambda b: b.flush(), 4: lambda b: b.set_rates(48000, 96000, ch=1),
            5: lambda b: b.set_rates(96000, 48000, ch=1), 6: lambda b: b.set_bandwidth(-1.0, 8000.0)}
    calls, refs = _reference(designs, 1, x, cuts, var, acts_ref)
    vs = _bank(qh, designs, 1)
    got = _run(vs, x, cuts, var, acts)
    assert np.array_equal(got[1][0][:, :400], x[:, 500:900]) and got[1][1].tolist() == [400, 400]     # run = 0 copies n and reports n
    # the rsize of channel 1 changes call by call: compare every call with the rsize in force
    for k, rs in enumerate([[140, 140]] * 4 + [[140, 140], [140, 280], [140, 280]]):
        _compare("setters, call %d" % k, calls[k:k + 1], got[k:k + 1], rs)
    assert [vs.rsize(0), vs.rsize(1)] == [refs[0].rsize, refs[1].rsize] == [140, 280]


def test_refusals_change_nothing(qh, oracle):
    import torch
    L = qh.load()
    ok = dict(in_rate=48000, out_rate=48000, R=64, fc=0.0, fc_low=-1.0, gain=1.0, var=1.0, varmode=1)
    order = ("in_rate", "out_rate", "R", "fc", "fc_low", "gain", "var", "varmode")
    bad = [("in_rate", 0), ("in_rate", -48000), ("out_rate", 0), ("out_rate", 48000 * 16 + 1), ("in_rate", 48000 * 17), ("R", 0), ("R", -4),
           ("R", 32768), ("var", float("nan")), ("var", float("inf")), ("var", 0.0), ("var", -1.0), ("var", 0.49), ("var", 2.01),
           ("gain", float("nan")), ("fc", float("inf"))]
    for k, v in bad:
        args = dict(ok, **{k: v})
        assert not L.qh_varsamp_create(0, 1, *[args[o] for o in order], None), (k, v)
        with pytest.raises(qh.QuiskHipError):
            qh.WdspVarResampler(1, **args)
    designs = [(48000, 48000, 64)] * 2
    cuts = [0, 900, 2000]
    x = _input(2, 2000, seed=31)
    var = np.array([[1.01, 0.97], [0.99, 1.02]])
    calls, refs = _reference(designs, 1, x, cuts, var)
    vs = _bank(qh, designs, 1)
    first = vs.process_host(x[:, :900], var[0])
    # the setters
    assert L.qh_varsamp_set_rates(vs._h, -1, 0, 48000) == -2 and L.qh_varsamp_set_rates(vs._h, 1, 48000, -1) == -2
    assert L.qh_varsamp_set_rates(vs._h, 0, 48000, 48000 * 16 + 1) == -2 and L.qh_varsamp_set_rates(vs._h, 2, 48000, 48000) == -2
    assert L.qh_varsamp_set_bandwidth(vs._h, -1, float("nan"), 3000.0) == -2 and L.qh_varsamp_flush(vs._h, -2) == -2
    assert L.qh_varsamp_set_run(vs._h, 2, 0) == -2
    # the call: a var out of range on one channel, an output stride below max_out, rows that share a byte
    n = 1100
    d = torch.from_numpy(x[:, 900:]).cuda()
    mo = vs.max_out(n, var[1])
    assert n * 1.02 <= mo <= n * 1.02 + 4
    o = torch.zeros((2, mo), dtype=torch.complex128, device="cuda")
    cnt = torch.zeros(2, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    for v in ([0.99, float("nan")], [2.5, 1.0], [1.0, 0.0], [float("inf"), 1.0], [1.0, -1.0], [0.4999, 1.0]):
        v = np.array(v)
        assert L.qh_varsamp_process(vs._h, d.data_ptr(), n, o.data_ptr(), mo, n, v.ctypes.data, cnt.data_ptr()) == -2, v
        assert L.qh_varsamp_max_out(vs._h, n, v.ctypes.data) == -2
    v = np.ascontiguousarray(var[1])
    assert L.qh_varsamp_process(vs._h, d.data_ptr(), n, o.data_ptr(), mo - 1, n, v.ctypes.data, cnt.data_ptr()) == -2
    assert L.qh_varsamp_process(vs._h, d.data_ptr(), n, o.data_ptr(), n - 1, n, v.ctypes.data, cnt.data_ptr()) == -2
    assert L.qh_varsamp_process(vs._h, d.data_ptr(), n, d.data_ptr(), mo, n, v.ctypes.data, cnt.data_ptr()) == -2                   # in place
    assert L.qh_varsamp_process(vs._h, d.data_ptr(), n, d.data_ptr() + 16 * (n - 1), mo, n, v.ctypes.data, cnt.data_ptr()) == -2    # one shared sample
    assert L.qh_varsamp_process(vs._h, d.data_ptr(), n - 1, o.data_ptr(), mo, n, v.ctypes.data, cnt.data_ptr()) == -2                 # in_stride < n
    vs.synchronize()
    assert not torch.any(o != 0).item() and cnt.tolist() == [0, 0]
    second = vs.process_host(x[:, 900:], var[1])
    _compare("after the refusals", calls, [first, second], [140, 140])


def test_device_rows_nothing_behind_the_count_and_stream_order(qh, oracle):
    """process, process, then one synchronize on device rows prefilled with NaN: the samples and counts of the host form, bit for bit, and
    every element behind a row's count still NaN"""
    import torch
    designs = [(48000, 48000, 64), (48000, 96000, 64), (96000, 48000, 64)]
    x = _input(3, 3000, seed=41)
    var = np.array([[1.04, 0.97, 1.01], [0.96, 1.0003, 1.04]])
    twin, vs = _bank(qh, designs, 1), _bank(qh, designs, 1)
    want = [twin.process_host(x[:, :1700], var[0]), twin.process_host(x[:, 1700:], var[1])]
    d = torch.from_numpy(x).cuda()
    outs, cnts = [], []
    torch.cuda.synchronize()
    for k, (a, b) in enumerate([(0, 1700), (1700, 3000)]):
        mo = vs.max_out(b - a, var[k]) + 7
        o = torch.full((3, mo), complex(float("nan"), float("nan")), dtype=torch.complex128, device="cuda")
        c = torch.full((3,), -1, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        vs.process_ptr(d.data_ptr() + 16 * a, 3000, o.data_ptr(), mo, b - a, var[k], c.data_ptr())
        outs.append(o); cnts.append(c)
    vs.synchronize()
    for k in range(2):
        y, c = outs[k].cpu().numpy(), cnts[k].cpu().numpy()
        wy, wc = want[k]
        assert np.array_equal(c, wc)
        for ch in range(3):
            assert np.array_equal(y[ch, :c[ch]], wy[ch, :c[ch]])
            assert np.all(np.isnan(y[ch, c[ch]:].real)) and np.all(np.isnan(y[ch, c[ch]:].imag))
            assert c[ch] < y.shape[1]
    # an empty call: nothing made, nothing written, the count 0
    o = torch.full((3, 4), complex(float("nan"), float("nan")), dtype=torch.complex128, device="cuda")
    c = torch.full((3,), -1, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    assert vs.max_out(0, var[1]) == 0
    vs.process_ptr(d.data_ptr(), 3000, o.data_ptr(), 4, 0, var[1], c.data_ptr())
    vs.synchronize()
    assert c.tolist() == [0, 0, 0] and torch.all(torch.isnan(o.real)).item()


def test_a_refusal_for_every_channel_leaves_different_designs_alone(qh, oracle):
    """A setter with ch = -1 that is refused, on a bank whose two channels hold different designs (48000 -> 96000 beside 96000 -> 48000):
    QH_ERR_INVALID, and both channels' next outputs are those of a twin bank that never received the call, bit for bit.  No single value
    is refused for one of the designs and taken by the other -- a refusal looks at the rates, R and the band edges' finiteness, and a
    ch = -1 call gives every channel the same ones -- so the designs are set apart with set_rates on channel 1 first (_bank)."""
    L = qh.load()
    designs = [(48000, 96000, 64), (96000, 48000, 64)]
    x = _input(2, 192, seed=37)
    var = np.array([[1.01, 0.97], [0.99, 1.02], [1.003, 0.98]])
    bank, twin = _bank(qh, designs, 1), _bank(qh, designs, 1)
    refused = [lambda h: L.qh_varsamp_set_rates(h, -1, 48000, 0), lambda h: L.qh_varsamp_set_bandwidth(h, -1, float("nan"), 3000.0),
               lambda h: L.qh_varsamp_set_rates(h, -1, 48000, 48000 * 16 + 1)]
    for k, call in enumerate([None] + refused[:2]):
        if call:
            assert call(bank._h) == -2 and refused[2](bank._h) == -2
        (ya, ca), (yb, cb) = bank.process_host(x[:, 64 * k:64 * k + 64], var[k]), twin.process_host(x[:, 64 * k:64 * k + 64], var[k])
        assert list(ca) == list(cb) and min(ca) > 0 and np.array_equal(ya, yb), k
