"""qh_resample_* (WDSP's fixed-ratio resampler, xresample and xresampleF, wdsp/resample.c:121-157, 296-330) against the sample-by-sample
restatement tests/wdsp_resample_ref.py run on the library's own taps (qh_resample_taps).

Count and phase are a closed form the bank's host side evaluates, and every output sample is made on its own (quisk_amd/csrc/
qh_resample.hip), so the gates are
  taps     the oracle's calc_resample table within 4e-16 of the largest tap (the gate tests/test_design_host.py holds the design to);
  counts   np.array_equal with the restatement's, call by call and channel by channel;
  complex  |y - ref| <= (cpp + 4) 2^-52 B per component, B = sum_j |h[n + j]| |ring| from the restatement: the standard bound of a dot
           product of cpp terms added in any order, taken for the two sides, with room for fused products.  Derived, not measured;
  float    equal as floats, or one float ulp apart where the restatement's double sum lies within that same bound of the midpoint of the
           two floats -- checked sample by sample, no quota.
-m gpu."""
import functools

import numpy as np
import pytest

from wdsp_resample_ref import Resample, ResampleF

pytestmark = pytest.mark.gpu

EPS = 2.0 ** -52
N = 5000
# a one-sample call, a second one (no output when decimating by two), calls shorter than cpp, one call of 3900 samples whose outputs
# cross many tiles of 256, and an empty call
CUTS = [0, 1, 2, 40, 139, 400, 400, 4300, N]
PAIRS = [(48000, 44100), (44100, 48000), (96000, 48000), (48000, 96000), (48000, 48000), (384000, 48000)]
SIZES = {(48000, 44100): (147, 160, 153), (44100, 48000): (160, 147, 141), (96000, 48000): (1, 2, 281), (48000, 96000): (2, 1, 141),
         (48000, 48000): (1, 1, 141), (384000, 48000): (1, 8, 1121)}


def _input(nch, n, seed):
    rng = np.random.default_rng(seed)
    t = np.arange(n)
    x = 0.3 * (rng.standard_normal((nch, n)) + 1j * rng.standard_normal((nch, n)))
    for c in range(nch):
        x[c] += np.exp(2j * np.pi * (0.031 + 0.07 * c) * t)
    return x


def _refs(bank, kw=None):
    """a restatement per channel with the design in force on the bank and the bank's own taps"""
    out = []
    for c in range(bank.nch):
        r = Resample(48000, 48000, **(kw or {})) if bank.dtype == "c64" else ResampleF(48000, 48000)
        out.append(r)
    return out


def _sync(refs, bank, rates):
    """put every restatement on its channel's rates with the bank's taps"""
    for c, r in enumerate(refs):
        r.set_rates(rates[c][0], rates[c][1], taps=bank.taps(c))
        assert (r.L, r.M, r.cpp) == (bank.L(c), bank.M(c), bank.cpp(c))


def _run(bank, x, cuts, acts=None):
    out = []
    for k, (a, b) in enumerate(zip(cuts[:-1], cuts[1:])):
        if acts and acts.get(k):
            acts[k](bank)
        out.append(bank.process_host(x[:, a:b]))
    return out


def _run_ref(refs, x, cuts, acts=None):
    calls = []
    for k, (a, b) in enumerate(zip(cuts[:-1], cuts[1:])):
        if acts and acts.get(k):
            for c, r in enumerate(refs):
                acts[k](r, c)
        calls.append([(r.process(x[c, a:b]), r.cpp, r.run) for c, r in enumerate(refs)])
    return calls


def _compare(what, calls_ref, calls_gpu, slack=1.0):
    """counts exactly, samples within the derived bound -> the worst ratio of error to bound"""
    worst = 0.0
    for k, (ref, (y, counts)) in enumerate(zip(calls_ref, calls_gpu)):
        want = [len(r[0][0]) if r[2] else 0 for r in ref]
        assert np.array_equal(counts, want), (what, k, counts.tolist(), want)
        for c, (res, cpp, run) in enumerate(ref):
            yr, B = res[0], res[1]
            if not len(yr):
                continue
            got = y[c, :len(yr)]
            if not run:
                assert np.array_equal(got, yr), (what, k, c)
                continue
            if yr.dtype == np.complex128:
                for err, b in ((np.abs(got.real - yr.real), B.real), (np.abs(got.imag - yr.imag), B.imag)):
                    bound = slack * (cpp + 4) * EPS * b
                    ratio = float(np.max(err / np.maximum(bound, 1e-300)))
                    worst = max(worst, ratio)
                    assert np.all(err <= bound), (what, k, c, ratio)
            else:
                sums = res[2]
                bad = np.nonzero(got != yr)[0]
                for i in bad:                           # one ulp apart, and the double sum within the bound of the midpoint of the two
                    assert got[i] == np.nextafter(yr[i], got[i]), (what, k, c, i, got[i], yr[i])
                    mid = 0.5 * (float(got[i]) + float(yr[i]))
                    ratio = abs(sums[i] - mid) / ((cpp + 4) * EPS * B[i])
                    worst = max(worst, ratio)
                    assert ratio <= 1.0, (what, k, c, i, ratio)
                if len(bad):
                    print("resample %s call %d ch %d: %d of %d floats one ulp off at a rounding midpoint" % (what, k, c, len(bad), len(yr)))
    print("resample %s: worst |y - ref| / bound %.4f" % (what, worst))
    return worst


@pytest.mark.parametrize("pair", PAIRS)
def test_matches_restatement(qh, oracle, pair):
    x = _input(2, N, seed=pair[0] // 1000 + pair[1] // 100)
    bank = qh.WdspResampler(2, *pair)
    assert (bank.L(0), bank.M(0), bank.cpp(0)) == (bank.L(1), bank.M(1), bank.cpp(1)) == SIZES[pair]
    want, L, M, ncoef, cpp = oracle.resample_taps(*pair)
    taps = bank.taps(0)
    assert taps.shape == (L, cpp) and np.abs(taps.reshape(-1) - want).max() <= 4e-16 * np.abs(want).max()
    assert np.array_equal(taps, bank.taps(1))
    refs = _refs(bank)
    _sync(refs, bank, [pair] * 2)
    calls = _run_ref(refs, x, CUTS)
    if pair == (96000, 48000):
        assert len(calls[1][0][0][0]) == 0                      # the second one-sample call makes nothing
    expect = [bank.out_count(b - a) for a, b in zip(CUTS[:1], CUTS[1:2])]
    got = _run(bank, x, CUTS)
    assert expect[0] == got[0][1][0]
    assert sum(int(c[0]) for _, c in got) == -(-N * L // M)
    _compare("%s" % (pair,), calls, got)
    for (y, counts), (a, b) in zip(got, zip(CUTS[:-1], CUTS[1:])):      # behind a row's count the host form leaves its zeros
        assert y.shape[1] >= bank.max_out(b - a)
        for c in range(2):
            assert not np.any(y[c, counts[c]:])


@pytest.mark.parametrize("pair", [(48000, 44100), (48000, 96000), (96000, 48000), (384000, 48000)])
def test_real_floats_match_restatement(qh, oracle, pair):
    x = _input(2, N, seed=pair[1] // 100 + 3).real.astype(np.float32)
    bank = qh.WdspResampler(2, *pair, dtype="r32")
    refs = _refs(bank)
    _sync(refs, bank, [pair] * 2)
    if pair == (48000, 44100):
        assert bank.cpp(0) == 146
    if pair == (48000, 96000):
        assert bank.cpp(0) == 134
    calls = _run_ref(refs, x, CUTS)
    got = _run(bank, x, CUTS)
    assert got[3][0].dtype == np.float32
    _compare("float %s" % (pair,), calls, got)


def test_channels_of_different_designs_in_one_bank(qh, oracle):
    rates = [(48000, 44100), (44100, 48000), (48000, 44100)]
    x = _input(3, N, seed=5)
    bank = qh.WdspResampler(3, 48000, 44100)
    bank.set_rates(44100, 48000, ch=1)
    bank.set_bandwidth(300.0, 9000.0, ch=2)
    assert [(bank.L(c), bank.M(c), bank.cpp(c)) for c in range(3)] == [(147, 160, 153), (160, 147, 141), (147, 160, 153)]
    assert not np.array_equal(bank.taps(0), bank.taps(2))
    refs = _refs(bank)
    refs[2].fcin, refs[2].fc_low = 9000.0, 300.0
    _sync(refs, bank, rates)
    _compare("mixed designs", _run_ref(refs, x, CUTS), _run(bank, x, CUTS))


@pytest.mark.parametrize("design", [dict(rates=(48000, 48000), ncoef=5000), dict(rates=(8000, 7999), ncoef=0)])
def test_windows_that_do_not_fit_the_tile(qh, oracle, design):
    """cpp 5001: no tile's window fits LDS, the inputs are read straight from memory; L 7999: a tile cannot hold every tap row, a block
    takes 256 consecutive outputs with a row per lane"""
    rates, n = design["rates"], 2600
    x = _input(2, n, seed=11)
    bank = qh.WdspResampler(2, *rates, ncoef=design["ncoef"])
    refs = _refs(bank, dict(ncoef=design["ncoef"]))
    _sync(refs, bank, [rates] * 2)
    assert refs[0].cpp == (5001 if design["ncoef"] else 141)
    cuts = [0, 1, 300, 300, 2100, n]
    _compare("cpp %d, L %d" % (refs[0].cpp, refs[0].L), _run_ref(refs, x, cuts), _run(bank, x, cuts))


def test_ragged_calls_are_one_call(qh, oracle):
    x = _input(2, N, seed=8)
    a, b = qh.WdspResampler(2, 48000, 44100), qh.WdspResampler(2, 48000, 44100)
    parts = _run(a, x, CUTS)
    y1, c1 = b.process_host(x)
    assert np.array_equal(np.sum([c for _, c in parts], axis=0), c1)
    refs = _refs(b)
    _sync(refs, b, [(48000, 44100)] * 2)
    one = _run_ref(refs, x, [0, N])
    joined = np.stack([np.concatenate([y[c, :cnt[c]] for y, cnt in parts]) for c in range(2)])
    _compare("ragged calls against one call", one, [(joined, c1)], slack=2.0)
    _compare("one call", one, [(y1, c1)])


def test_setters_in_mid_stream(qh, oracle):
    cuts = [0, 500, 900, 1300, 2000, 2700, 3400, 4100, N]
    x = _input(2, N, seed=21)
    bank = qh.WdspResampler(2, 48000, 44100)
    refs = _refs(bank)
    _sync(refs, bank, [(48000, 44100)] * 2)

    def ref_run(v):
        def f(r, c):
            r.run = v
        return f

    def ref_rates(i, o):
        def f(r, c):
            if c == 1:
                r.set_rates(i, o, taps=bank.taps(1))
        return f

    # the bank goes first, call by call, so that the restatement can take the taps in force
    got, calls = [], []
    acts = {1: lambda b: b.set_run(0), 2: lambda b: b.set_run(1), 3: lambda b: b.flush(), 4: lambda b: b.set_rates(48000, 96000, ch=1),
            5: lambda b: b.set_rates(96000, 48000, ch=1), 6: lambda b: b.set_fc_low(250.0), 7: lambda b: b.set_bandwidth(-1.0, 8000.0)}

    def ref_fc_low(r, c):
        r.fc_low = 250.0
        r.calc(taps=bank.taps(c))

    def ref_bw(r, c):
        r.fc_low, r.fcin = -1.0, 8000.0
        r.calc(taps=bank.taps(c))

    acts_ref = {1: ref_run(0), 2: ref_run(1), 3: lambda r, c: r.flush(), 4: ref_rates(48000, 96000), 5: ref_rates(96000, 48000), 6: ref_fc_low, 7: ref_bw}
    for k in range(len(cuts) - 1):
        got += _run(bank, x, cuts[k:k + 2], {0: acts.get(k)})
        calls += _run_ref(refs, x, cuts[k:k + 2], {0: acts_ref.get(k)})
    assert np.array_equal(got[1][0][:, :400], x[:, 500:900]) and got[1][1].tolist() == [0, 0]       # run = 0 copies n and reports 0
    assert [(bank.L(c), bank.M(c), bank.cpp(c)) for c in range(2)] == [(r.L, r.M, r.cpp) for r in refs] == [(147, 160, 153), (1, 2, 281)]
    _compare("setters", calls, got)


def test_an_unchanged_value_keeps_the_history(qh, oracle):
    x = _input(2, 2000, seed=23)
    bank, twin = qh.WdspResampler(2, 48000, 44100, fc=9000.0), qh.WdspResampler(2, 48000, 44100, fc=9000.0)
    a0, b0 = bank.process_host(x[:, :1000]), twin.process_host(x[:, :1000])
    bank.set_fc_low(-1.0)
    bank.set_bandwidth(-1.0, 9000.0)
    a1, b1 = bank.process_host(x[:, 1000:]), twin.process_host(x[:, 1000:])
    assert np.array_equal(a0[0], b0[0]) and np.array_equal(a1[0], b1[0]) and np.array_equal(a1[1], b1[1])
    bank.set_bandwidth(-1.0, 9000.5)                            # a change: the stream starts over, as one that has seen nothing
    fresh = qh.WdspResampler(2, 48000, 44100, fc=9000.5)
    a2, f2 = bank.process_host(x[:, :700]), fresh.process_host(x[:, :700])
    assert np.array_equal(a2[0], f2[0]) and np.array_equal(a2[1], f2[1])


def test_refusals_change_nothing(qh, oracle):
    import torch
    L = qh.load()
    ok = dict(in_rate=48000, out_rate=44100, fc=0.0, ncoef=0, gain=1.0, dtype=0)
    order = ("in_rate", "out_rate", "fc", "ncoef", "gain", "dtype")
    bad = [("in_rate", 0), ("in_rate", -48000), ("out_rate", 0), ("out_rate", -1), ("out_rate", 44101), ("in_rate", 2000000000), ("ncoef", -1),
           ("ncoef", 4194304), ("ncoef", 2147483647), ("gain", float("nan")), ("fc", float("inf")), ("gain", float("-inf")), ("dtype", 2)]
    for k, v in bad:
        args = dict(ok, **{k: v})
        assert not L.qh_resample_create(0, 1, *[args[o] for o in order], None), (k, v)
    with pytest.raises(qh.QuiskHipError):
        qh.WdspResampler(1, 48000, 0)
    assert not L.qh_resample_create(0, 0, *[ok[o] for o in order], None)
    x = _input(2, 2000, seed=31)
    bank = qh.WdspResampler(2, 48000, 44100)
    refs = _refs(bank)
    _sync(refs, bank, [(48000, 44100)] * 2)
    calls = _run_ref(refs, x, [0, 900, 2000])
    first = bank.process_host(x[:, :900])
    taps = bank.taps(1)
    # the setters
    h = bank._h
    assert L.qh_resample_set_rates(h, -1, 0, 48000) == -2 and L.qh_resample_set_rates(h, 1, 48000, -1) == -2
    assert L.qh_resample_set_rates(h, 0, 48000, 44101) == -2 and L.qh_resample_set_rates(h, 2, 48000, 48000) == -2
    assert L.qh_resample_set_rates(h, 1, 2000000000, 3) == -2
    assert L.qh_resample_set_fc_low(h, -1, float("nan")) == -2 and L.qh_resample_set_bandwidth(h, 0, 100.0, float("inf")) == -2
    assert L.qh_resample_flush(h, -2) == -2 and L.qh_resample_set_run(h, 2, 0) == -2
    assert L.qh_resample_set_run(None, 0, 0) == -2 and L.qh_resample_flush(None, 0) == -2 and L.qh_resample_max_out(None, 4) == -2
    assert L.qh_resample_taps(h, 0, None, 1 << 20) == -2 and L.qh_resample_taps(h, 0, taps.ctypes.data, taps.size - 1) == -2
    assert L.qh_resample_out_count(h, 2, 10) == -2 and L.qh_resample_max_out(h, -1) == -2
    fbank = qh.WdspResampler(1, 48000, 44100, dtype="r32")
    assert L.qh_resample_set_fc_low(fbank._h, 0, 100.0) == -2 and L.qh_resample_set_bandwidth(fbank._h, 0, 100.0, 3000.0) == -2
    assert np.array_equal(bank.taps(1), taps)
    # the call: an output stride below max_out, rows that share a byte, null pointers
    n = 1100
    d = torch.from_numpy(x[:, 900:]).cuda()
    mo = bank.max_out(n)
    assert mo == -(-n * 147 // 160)
    o = torch.zeros((2, mo), dtype=torch.complex128, device="cuda")
    cnt = np.full(2, -7, dtype=np.int32)
    torch.cuda.synchronize()
    P = L.qh_resample_process
    assert P(h, d.data_ptr(), n, o.data_ptr(), mo - 1, n, cnt.ctypes.data) == -2
    assert P(h, d.data_ptr(), n, d.data_ptr(), mo, n, cnt.ctypes.data) == -2                    # in place
    assert P(h, d.data_ptr(), n, d.data_ptr() + 16 * (n - 1), mo, n, cnt.ctypes.data) == -2     # one shared sample
    assert P(h, d.data_ptr(), n - 1, o.data_ptr(), mo, n, cnt.ctypes.data) == -2                # in_stride < n
    assert P(h, None, n, o.data_ptr(), mo, n, cnt.ctypes.data) == -2 and P(h, d.data_ptr(), n, None, mo, n, cnt.ctypes.data) == -2
    assert P(h, d.data_ptr(), n, o.data_ptr(), mo, n, None) == -2 and P(None, d.data_ptr(), n, o.data_ptr(), mo, n, cnt.ctypes.data) == -2
    assert P(h, d.data_ptr(), n, o.data_ptr(), mo, -1, cnt.ctypes.data) == -2
    bank.synchronize()
    assert not torch.any(o != 0).item() and cnt.tolist() == [-7, -7]
    second = bank.process_host(x[:, 900:])
    _compare("after the refusals", calls, [first, second])


def test_device_rows_nothing_behind_the_count_and_stream_order(qh, oracle):
    """process, process, then one synchronize on device rows prefilled with NaN: the samples and counts of the host form, bit for bit, and
    every element behind a row's count still NaN; a channel that does not run has its n samples copied and nothing behind them"""
    import torch
    rates = [(48000, 44100), (48000, 96000), (96000, 48000)]
    x = _input(3, 3000, seed=41)

    def make():
        b = qh.WdspResampler(3, *rates[0])
        b.set_rates(*rates[1], ch=1)
        b.set_rates(*rates[2], ch=2)
        return b

    twin, bank = make(), make()
    want = [twin.process_host(x[:, :1700]), twin.process_host(x[:, 1700:])]
    d = torch.from_numpy(x).cuda()
    outs, cnts = [], []
    torch.cuda.synchronize()
    for k, (a, b) in enumerate([(0, 1700), (1700, 3000)]):
        mo = bank.max_out(b - a) + 7
        o = torch.full((3, mo), complex(float("nan"), float("nan")), dtype=torch.complex128, device="cuda")
        torch.cuda.synchronize()
        cnts.append(bank.process_ptr(d.data_ptr() + 16 * a, 3000, o.data_ptr(), mo, b - a))
        outs.append(o)
    bank.synchronize()
    for k in range(2):
        y, c = outs[k].cpu().numpy(), cnts[k]
        wy, wc = want[k]
        assert np.array_equal(c, wc)
        for ch in range(3):
            assert np.array_equal(y[ch, :c[ch]], wy[ch, :c[ch]])
            assert np.all(np.isnan(y[ch, c[ch]:].real)) and np.all(np.isnan(y[ch, c[ch]:].imag))
            assert c[ch] < y.shape[1]
    # torch tensors, one channel switched off: its samples are copied, its count is 0, nothing behind the copy
    bank.set_run(0, ch=1)
    twin.set_run(0, ch=1)
    wy, wc = twin.process_host(x[:, :800])
    o = torch.full((3, bank.max_out(800) + 3), complex(float("nan"), float("nan")), dtype=torch.complex128, device="cuda")
    y, c = bank.process(d[:, :800], out=o)
    bank.synchronize()
    y = y.cpu().numpy()
    assert np.array_equal(c, wc) and c[1] == 0 and bank.max_out(800) == 800
    assert np.array_equal(y[1, :800], x[1, :800]) and np.all(np.isnan(y[1, 800:].real))
    for ch in (0, 2):
        assert np.array_equal(y[ch, :c[ch]], wy[ch, :c[ch]]) and np.all(np.isnan(y[ch, c[ch]:].real))
    # an empty call: nothing made, nothing written, the counts 0
    o = torch.full((3, 4), complex(float("nan"), float("nan")), dtype=torch.complex128, device="cuda")
    torch.cuda.synchronize()
    assert bank.max_out(0) == 0
    c = bank.process_ptr(d.data_ptr(), 3000, o.data_ptr(), 4, 0)
    bank.synchronize()
    assert c.tolist() == [0, 0, 0] and torch.all(torch.isnan(o.real)).item()


def test_a_channel_does_not_see_its_neighbour(qh, oracle):
    x = _input(2, 3000, seed=51)
    a = qh.WdspResampler(2, 48000, 44100)
    want = [a.process_host(x[:, :1300]), a.process_host(x[:, 1300:])]
    b = qh.WdspResampler(2, 48000, 44100)
    x2 = x.copy()
    x2[1] = _input(1, 3000, seed=52)[0] * 7.0
    g0 = b.process_host(x2[:, :1300])
    b.set_rates(48000, 96000, ch=1)
    g1 = b.process_host(x2[:, 1300:])
    for (wy, wc), (gy, gc) in zip(want, (g0, g1)):
        assert wc[0] == gc[0] and np.array_equal(wy[0, :wc[0]], gy[0, :gc[0]])     # channel 0's bits do not move
    assert g1[1][1] == 2 * 1700


def test_a_refusal_for_every_channel_leaves_different_designs_alone(qh, oracle):
    """A setter with ch = -1 that is refused, on a bank whose two channels hold different designs (48000 -> 44100 beside 48000 -> 24000):
    QH_ERR_INVALID, and both channels' next outputs are those of a twin bank that never received the call, bit for bit.  No single value
    is refused for one of the designs and taken by the other -- a refusal looks at the rates, ncoef and the band edges' finiteness, and a
    ch = -1 call gives every channel the same ones -- so the designs are set apart with set_rates on channel 1 first."""
    L = qh.load()
    x = _input(2, 192, seed=37)
    bank, twin = qh.WdspResampler(2, 48000, 44100), qh.WdspResampler(2, 48000, 44100)
    for b in (bank, twin):
        b.set_rates(48000, 24000, ch=1)
        assert [(b.L(c), b.M(c), b.cpp(c)) for c in range(2)] == [(147, 160, 153), (1, 2, 281)]
    refused = [lambda h: L.qh_resample_set_rates(h, -1, 48000, 0), lambda h: L.qh_resample_set_fc_low(h, -1, float("nan")),
               lambda h: L.qh_resample_set_bandwidth(h, -1, 100.0, float("inf"))]
    for k, call in enumerate([None] + refused[:2]):
        if call:
            assert call(bank._h) == -2 and refused[2](bank._h) == -2
        (ya, ca), (yb, cb) = bank.process_host(x[:, 64 * k:64 * k + 64]), twin.process_host(x[:, 64 * k:64 * k + 64])
        assert ca.tolist() == cb.tolist() and min(ca) > 0 and np.array_equal(ya, yb), k
    assert [(bank.L(c), bank.M(c), bank.cpp(c)) for c in range(2)] == [(147, 160, 153), (1, 2, 281)]
