"""Channel isolation: no channel's input or settings reach another channel's output.

The reference runs one WDSP DSP thread per channel and one filter.c struct per stream, so one channel's samples and setters cannot
move another channel's output.  The device entry points are batched and share work across channels (paired tiles, partitioned
stages sized by the longest channel, forms chosen over every channel, sub-set launches, graph replay), so the property is asserted
here, differentially and without an oracle: two objects with identical settings are fed the same ragged stream, and from the third
call on the second object's victim channel v gets another, 50 dB louder signal with a carrier in its passband.  Every channel other
than v (and v's pair partner where a paired form runs, see below) must come out bit-identical, side outputs (meters, panadapter
pixels and S-meter) included.

Pair partners.  Two real channels may ride as the real and imaginary parts of one complex transform: the engine's AM / SAM bp1 and FM
de-emphasis stages (run_band's `pairs`: neighbours of the mode's channel list, a channel left over paired with itself) and the Quisk
receiver bank's real audio filters (Stage::set_pair: 2p with 2p + 1, the last of an odd count with itself; USB, AM and FM, not
DGT-IQ).  The partner sees v's samples only through the rounding of the shared transform, so it is not bit-identical: the engine's
AM / SAM partners and the receiver bank's partners are bounded by 64 eps max|v| sqrt(4096) (test_pair_partner_coupling_is_rounding_only,
_assert_qrx_partner_bounded); the engine's FM partner, whose paired stage output the API does not show, and the process bank's
partner (squelch and noise blanker decide on sample values) are held to their oracle gate or only exempt.

Non-finite containment (the D tests) -- the audit.  A NaN or Inf is fed only to kernels where no loop trip count and no address
depends on a sample value:
  cleared   the overlap-save FIR tiles (qh_osfir.hpp) and the FIR bank's polyphase forms (qh_fir.hip, hist_next and
            hist_update_kernel), the half-band cascade (qh_hbcascade.*: its segment loops run on n_in and nch only), the rational
            resampler (qh_polyphase.hip), the engine's front stage, shift and nbp0 / bp1 band stages including the partitioned form
            (long_gather / long_add / long_hist: loops on n, lh and nch), the panadapter's FFT, average and pixel kernels (the
            pixel loop's bins come from rate, zoom and width, quisk_amd/csrc/qh_pan.hip bscope_graph_kernel).
  left out  AGC (qh_agc_tiled.hpp walks regime steps with `while (p < cnt)`), process_agc (qh_qagc.hip's regime chains), the SNBA
            and EMNR scratch walks, the noise blanker, the analyzer's pixel path, the meters (mlog10 indexing): a NaN reaching a
            data-driven loop can spin a kernel.  The AM / FM detectors (PLL verify, AM leveller) are left out too: not audited here.
The D tests therefore run SSB with AGC mode 0, meters off, and the filter banks and panadapter.  So no paired form (AM / SAM bp1, FM
de-emphasis, the receiver bank's audio filters) ever gets a burst, and whether a NaN in one half of a pair tile reaches the partner
(the issue's fix 2) is not assessed here; nor is a burst into the partitioned bp1 stage (it runs only in those modes).

Left out of the issue's list: an AGC-on pair partner against its oracle (the pair partners run at fixed gain only), RXASetNC on one
FM channel (the FM filters are shared, what a differing FM nc does is not settled here), and set_agc of the Quisk banks, which is one
setting for the whole bank and has no one-channel form.

Partitioned stages (nc > 4096): run_band runs K = max over channels partitions for every channel; a channel whose own impulse
response is shorter used to add its further partitions too, with zero masks over the older part of its delay line -- NaN * 0 = NaN,
so one burst kept it non-finite for 4096 K samples where the reference recovers after its own nc.  Partitions beyond a channel's own
impulse response are no longer added (long_add_kernel); test_partitioned_stage_burst_recovers_within_own_nc is the case.  -m gpu."""
import numpy as np
import pytest

from quisk_amd import synth

pytestmark = pytest.mark.gpu

METER_TYPES = (0, 1, 2, 3, 5, 6)
PASSBAND = {1: (300.0, 3000.0), 6: (-4000.0, 4000.0), 10: (-4000.0, 4000.0), 5: (-8000.0, 8000.0)}


# ---------------------------------------------------------------------------------------------------------------- helpers
def _loud(n, fs, f_carrier, seed):
    """another finite signal for the victim: other noise, ~50 dB louder, a carrier at f_carrier"""
    rng = np.random.default_rng(seed)
    t = np.arange(n)
    return (300.0 * (rng.standard_normal(n) + 1j * rng.standard_normal(n)) * 0.01
            + 30.0 * np.exp(2j * np.pi * f_carrier / fs * t))


def _victims(nch):
    return sorted({0, nch // 2, nch - 1})


def _alt(x, v, start, fs=192000.0, f_carrier=None, seed=777):
    y = x.copy()
    n = x.shape[1] - start
    if f_carrier is None:
        f_carrier = 1500.0 - synth.shift_freq(v)          # the RXA shift brings it to +1500 Hz: inside every passband used here
    y[v, start:] = _loud(n, fs, f_carrier, seed + v).astype(x.dtype)
    return y


def _differential(make, step, xa, xb, calls, side=None):
    """Feed make()'s two objects xa and xb call by call; returns per call (outs_a, outs_b, sides_a, sides_b)."""
    a, b = make(), make()
    res = []
    pos = 0
    try:
        for n in calls:
            ya = step(a, np.ascontiguousarray(xa[:, pos:pos + n]))
            yb = step(b, np.ascontiguousarray(xb[:, pos:pos + n]))
            sa = side(a) if side else None
            sb = side(b) if side else None
            res.append((ya, yb, sa, sb))
            pos += n
    finally:
        for o in (a, b):
            o.close()
    return res


def _assert_isolated(res, nch, v, skip=(), side_rows=True):
    """every channel but v and `skip` bit-identical in every call; v itself moved (the test bites)"""
    moved = False
    for k, (ya, yb, sa, sb) in enumerate(res):
        for c in range(nch):
            if c == v:
                moved = moved or not np.array_equal(ya[c], yb[c])
                continue
            if c in skip:
                continue
            assert np.array_equal(ya[c], yb[c]), ("call", k, "channel", c, "victim", v,
                                                  float(np.nanmax(np.abs(ya[c] - yb[c])) if ya[c].size else 0.0))
            if sa is not None and side_rows:
                assert np.array_equal(np.asarray(sa[c]), np.asarray(sb[c])), ("side output", k, c, v, sa[c], sb[c])
    assert moved, "the victim's output did not change: the test would not see a leak"


def _pair_partner(group, v):
    """run_band's pairs: neighbours in the mode's channel list, a channel left over is its own partner"""
    i = group.index(v)
    j = i ^ 1
    return group[j] if j < len(group) else v


# ---------------------------------------------------------------------------------------------------------------- RXA engine
def _rxa(qh, nch, modes=(1,), agc=0, agc_on=None, meters=False, nc=None, extra=None):
    def make():
        e = qh.RxaEngine(nch)
        for c in range(nch):
            m = modes[c % len(modes)]
            e.SetRXAShiftRun(c, 1); e.SetRXAShiftFreq(c, synth.shift_freq(c)); e.RXANBPSetRun(c, 1)
            e.SetRXAMode(c, m); e.RXASetPassband(c, *PASSBAND[m])
            if nc and nc.get(c):
                e.RXASetNC(c, nc[c])
            on = agc_on is None or c in agc_on
            e.SetRXAAGCMode(c, agc if on else 0)
            e.SetRXAAGCFixed(c, 3.0 + c)
        e.enable_meters(meters)
        if extra:
            extra(e)
        return e
    return make


def _rxa_step(e, x):
    return e.process_host(x)


def _meters(nch):
    return lambda e: [tuple(e.GetRXAMeter(c, mt) for mt in METER_TYPES) for c in range(nch)]


CALLS_RXA = [30, 7, 1, 24, 2, 40, 1, 16]          # DSP blocks per call (1024 input samples each)


def _run_rxa(qh, nch, v, calls=CALLS_RXA, meters=False, sig=None, **kw):
    n = sum(calls) * 1024
    if sig is None:
        x = synth.make_input_numpy(nch, n)
    else:
        x = np.stack([synth.make_mode_input_numpy(sig[c % len(sig)], c, n) for c in range(nch)])
    xb = _alt(x, v, sum(calls[:2]) * 1024)
    return _differential(_rxa(qh, nch, meters=meters, **kw), _rxa_step, x, xb, [c * 1024 for c in calls],
                         side=_meters(nch) if meters else None)


@pytest.mark.parametrize("meters", [False, True], ids=["meters_off", "meters_on"])
@pytest.mark.parametrize("nch", [4, 5])
def test_rxa_ssb_fused_chain(qh, nch, meters):
    for v in _victims(nch):
        _assert_isolated(_run_rxa(qh, nch, v, meters=meters), nch, v)


C4 = (1, 6, 5, 10)                                 # USB, AM, FM, SAM by c mod 4
C4_SIG = ("usb", "am", "fm", "am")


@pytest.mark.parametrize("meters", [False, True], ids=["split_direct_fused", "per_mode_meters"])
@pytest.mark.parametrize("nch", [8, 11])
def test_rxa_config4_mix(qh, nch, meters):
    for v in _victims(nch):
        m = C4[v % 4]
        group = [c for c in range(nch) if C4[c % 4] == m]
        skip = () if m == 1 else (_pair_partner(group, v),)
        _assert_isolated(_run_rxa(qh, nch, v, meters=meters, modes=C4, sig=C4_SIG), nch, v, skip=skip)


@pytest.mark.parametrize("agc", [1, 2, 3, 4])
def test_rxa_agc_every_channel_tiled(qh, agc):
    nch = 5
    for v in _victims(nch):
        _assert_isolated(_run_rxa(qh, nch, v, agc=agc), nch, v)


@pytest.mark.parametrize("who", ["victim", "other"])
def test_rxa_agc_on_one_channel_moves_every_channel_to_the_per_mode_path(qh, who):
    nch = 5
    for v in _victims(nch):
        on = {v} if who == "victim" else {(v + 1) % nch}
        _assert_isolated(_run_rxa(qh, nch, v, agc=3, agc_on=on, meters=True), nch, v)


def test_rxa_short_calls_down_to_one_block(qh):
    nch = 5
    calls = [3, 2, 1, 1, 2, 1, 1, 1, 3, 1]
    for v in _victims(nch):
        _assert_isolated(_run_rxa(qh, nch, v, calls=calls), nch, v)
        _assert_isolated(_run_rxa(qh, nch, v, calls=calls, agc=4), nch, v)


@pytest.mark.parametrize("stage", ["EMNR", "SNBA", "ANF", "ANR"])
@pytest.mark.parametrize("where", ["victim", "all"])
def test_rxa_noise_stages(qh, stage, where):
    nch = 5

    for v in _victims(nch):
        def extra(e, v=v):
            if stage == "EMNR":
                e.load_emnr_tables()
            for c in (range(nch) if where == "all" else (v,)):
                getattr(e, "SetRXA%sRun" % stage)(c, 1)
        _assert_isolated(_run_rxa(qh, nch, v, extra=extra), nch, v)


@pytest.mark.parametrize("big", [8192, 65536])
def test_rxa_long_nc_on_another_channel(qh, big):
    nch = 4
    for v in _victims(nch):
        other = (v + 1) % nch
        _assert_isolated(_run_rxa(qh, nch, v, nc={v: 2048, other: big}), nch, v)


def test_rxa_graph_replay_block_at_a_time(qh):
    import torch
    nch, nblk = 5, 40
    dev = torch.device("cuda:0")
    x = synth.make_input_numpy(nch, nblk * 1024)
    for v in _victims(nch):
        xb = _alt(x, v, 2 * 1024)
        outs = []
        for src in (x, xb):
            e = _rxa(qh, nch)()
            e.set_graph_replay(True)
            d_in = torch.empty((nch, 1024), dtype=torch.complex128, device=dev)
            d_out = torch.empty((nch, 256), dtype=torch.complex128, device=dev)
            ys = []
            for b in range(nblk):
                d_in.copy_(torch.from_numpy(np.ascontiguousarray(src[:, b * 1024:(b + 1) * 1024])))
                torch.cuda.synchronize(dev)
                e.process_ptr(d_in.data_ptr(), 1024, d_out.data_ptr(), 256, 1)
                e.synchronize()
                ys.append(d_out.cpu().numpy().copy())
            assert e.graph_launches() > 0
            e.close()
            outs.append(ys)
        res = [(a, b, None, None) for a, b in zip(*outs)]
        _assert_isolated(res, nch, v)


def test_rxa_audio_egress_bytes(qh):
    import torch
    nch, calls = 5, [12, 3, 1, 20]
    dev = torch.device("cuda:0")
    x = synth.make_input_numpy(nch, sum(calls) * 1024)
    for v in _victims(nch):
        xb = _alt(x, v, sum(calls[:2]) * 1024)
        outs = []
        for src in (x, xb):
            e = _rxa(qh, nch)()
            fmt = qh.AudioFormat("i16", volume=0.37, prescale=2147483647.0)
            ys, pos = [], 0
            for nb in calls:
                d_in = torch.from_numpy(np.ascontiguousarray(src[:, pos * 1024:(pos + nb) * 1024])).to(dev)
                rowb = nb * 256 * fmt.frame_bytes
                d_out = torch.zeros((nch, rowb), dtype=torch.uint8, device=dev)
                torch.cuda.synchronize(dev)
                e.process_audio_ptr(d_in.data_ptr(), nb * 1024, d_out.data_ptr(), rowb, nb, fmt)
                e.synchronize()
                ys.append(d_out.cpu().numpy().copy())
                pos += nb
            e.close()
            outs.append(ys)
        _assert_isolated([(a, b, None, None) for a, b in zip(*outs)], nch, v)


# ---------------------------------------------------------------------------------------------------------------- setters
SETTERS = {
    "shift": lambda e, v: e.SetRXAShiftFreq(v, synth.shift_freq(v) + 250.0),
    "passband": lambda e, v: e.RXASetPassband(v, 500.0, 2400.0),
    "mode_am": lambda e, v: (e.SetRXAMode(v, 6), e.RXASetPassband(v, *PASSBAND[6])),
    "agc_fixed": lambda e, v: e.SetRXAAGCFixed(v, -7.0),
    "notch": lambda e, v: (e.RXANBPAddNotch(v, 0, 1500.0, 200.0, 1), e.RXANBPSetNotchesRun(v, 1)),
    "nc_1024": lambda e, v: e.RXASetNC(v, 1024),
}
# setters that move a form shared by every channel: the others then only keep their oracle gates (tests/test_gpu_long_nc.py,
# tests/test_gpu_rxa_fuzz.py); named here, not asserted bit for bit
SHARED_FORM = {
    "agc_mode": ("AGC on one channel moves every channel to the per-mode path", lambda e, v: e.SetRXAAGCMode(v, 3)),
    "mode_am": ("AM on one channel moves every channel to the per-mode path", SETTERS["mode_am"]),
    "nc_8192": ("nc > 2048 moves every channel to 8192-point tiles", lambda e, v: e.RXASetNC(v, 8192)),
    "nc_65536": ("nc > 4096 moves every channel to partitions", lambda e, v: e.RXASetNC(v, 65536)),
    "emnr": ("EMNR moves every channel to the per-mode path", lambda e, v: (e.load_emnr_tables(), e.SetRXAEMNRRun(v, 1))),
    "snba": ("SNBA moves every channel to the per-mode path", lambda e, v: e.SetRXASNBARun(v, 1)),
}


def _setter_run(qh, nch, v, setter, calls=CALLS_RXA, per_mode=False):
    x = synth.make_input_numpy(nch, sum(calls) * 1024)
    make = _rxa(qh, nch, agc=3 if per_mode else 0, agc_on={(v + 1) % nch} if per_mode else None)
    a, b = make(), make()
    res, pos, tiles = [], 0, []
    try:
        for k, nb in enumerate(calls):
            if k == 2:
                setter(b, v)
            seg = np.ascontiguousarray(x[:, pos:pos + nb * 1024])
            res.append((a.process_host(seg), b.process_host(seg), None, None))
            tiles.append((a.band_tile(), b.band_tile()))
            pos += nb * 1024
    finally:
        a.close(); b.close()
    return res, tiles


# (a mode change to AM takes a linear chain to the per-mode path: SHARED_FORM["mode_am"]; on that path already, it moves nothing shared)
@pytest.mark.parametrize("name,per_mode", [(n, p) for n in sorted(SETTERS) for p in (False, True) if p or n != "mode_am"])
def test_setter_on_one_channel_leaves_the_others_bit_identical(qh, name, per_mode):
    nch = 5
    for v in _victims(nch):
        res, tiles = _setter_run(qh, nch, v, SETTERS[name], per_mode=per_mode)
        assert all(ta == tb for ta, tb in tiles), tiles          # no shared form moved
        _assert_isolated(res, nch, v)


@pytest.mark.parametrize("name", sorted(SHARED_FORM))
def test_setter_that_moves_a_shared_form_keeps_the_others_close(qh, name):
    """The shared form moves for every channel: the others are not bit-identical then, but a change of form is a change of rounding
    only -- they stay within 1e-9 (the SSB oracle gate of tests/test_gpu_long_nc.py) of the run without the setter.  The nc setters'
    move is asserted by band_tile(); the move to the per-mode path has no flag the API reads back."""
    nch = 5
    why, setter = SHARED_FORM[name]
    for v in _victims(nch):
        res, tiles = _setter_run(qh, nch, v, setter)
        if name in ("nc_8192", "nc_65536"):               # the band tile is the observable form: 4096 before, 8192 after
            assert tiles[1] == (4096, 4096) and tiles[2] == (4096, 8192), (why, tiles)
        moved = False
        for k, (ya, yb, _, _) in enumerate(res):
            moved = moved or not np.array_equal(ya[v], yb[v])
            for c in range(nch):
                if c == v:
                    continue
                d = np.sqrt(np.sum(np.abs(ya[c] - yb[c]) ** 2) / max(np.sum(np.abs(ya[c]) ** 2), 1e-300))
                assert d < 1e-9, (why, k, c, v, d)
        assert moved, why


def test_set_nc_zeroes_only_the_channels_own_delay_lines(qh, oracle):
    """RXASetNC(v, nc) with the form unchanged (2048 -> 1024 -> 2048): the other channels bit for bit; v restarts from zeros as the
    reference's setNc_fircore does (firmin.c:454-466): v against the oracle given the same two calls, every call within 1e-9"""
    from conftest import rel_rms
    nch = 4
    x = synth.make_input_numpy(nch, sum(CALLS_RXA) * 1024)
    for v in _victims(nch):
        res, tiles = _setter_run(qh, nch, v, lambda e, c: (e.RXASetNC(c, 1024), e.RXASetNC(c, 2048)))
        assert all(ta == tb for ta, tb in tiles)
        _assert_isolated(res, nch, v)
        o = oracle.WdspChannel(1024, 256, 192000, 48000, 48000)
        o.SetRXAShiftRun(1); o.SetRXAShiftFreq(synth.shift_freq(v)); o.RXANBPSetRun(1); o.SetRXAMode(1)
        o.RXASetPassband(*PASSBAND[1]); o.SetRXAAGCMode(0); o.SetRXAAGCFixed(3.0 + v)
        pos = 0
        for k, nb in enumerate(CALLS_RXA):
            if k == 2:
                o.RXASetNC(1024); o.RXASetNC(2048)
            want = o.xrxa(x[v, pos:pos + nb * 1024])
            pos += nb * 1024
            assert rel_rms(res[k][1][v], want) < 1e-9, (v, k, rel_rms(res[k][1][v], want))


# ---------------------------------------------------------------------------------------------------------------- Quisk-native
# quisk_amd.rxfilter modes with a Stage pair form (qh_qrx.hip: the SSB / AM / FM audio interpolators and AM's / FM's audio filters call
# set_pair); DGT-IQ has none (is_iq: U = 1, no audio filter), so nothing is exempt there
QRX_PAIRED = {3, 4, 5}


def _qrx_partner(mode, nch, v):
    """Stage::set_pair: 2p with 2p + 1, the last of an odd count alone; v itself where no pair form runs"""
    return (v ^ 1 if (v ^ 1) < nch else v) if mode in QRX_PAIRED else v


def _assert_qrx_partner_bounded(res, v, partner):
    """The partner sees v only through the rounding of the shared kStageNfft = 4096-point transforms: at most
    64 eps max|v| sqrt(4096) per output sample (fixed gain: the bank's process_agc is off), as for the engine's pairs."""
    if partner == v:
        return
    eps = np.finfo(np.float64).eps
    vmax = max(float(np.abs(yb[v]).max()) for _, yb, _, _ in res if yb.size)
    worst = max(float(np.abs(ya[partner] - yb[partner]).max()) for ya, yb, _, _ in res if ya.size)
    assert worst <= 64 * eps * vmax * np.sqrt(4096), (v, partner, worst, vmax)


@pytest.mark.parametrize("mode", [3, 4, 5, 9])        # quisk_amd.rxfilter modes: USB / AM / FM / DGT-IQ
@pytest.mark.parametrize("nch", [4, 5])
def test_quisk_rx_bank(qh, mode, nch):
    fs = 192000
    calls = [19200, 4800, 960, 9600, 19200]
    x = synth.make_input_numpy(nch, sum(calls))
    for v in _victims(nch):
        xb = _alt(x, v, sum(calls[:2]), f_carrier=1500.0)
        partner = _qrx_partner(mode, nch, v)
        res = _differential(lambda: qh.QuiskRxBank(nch, fs, mode), lambda o, s: o.process_host(s), x, xb, calls)
        _assert_isolated(res, nch, v, skip=(partner,))
        _assert_qrx_partner_bounded(res, v, partner)


def _lowpass(ntaps, fc, fs):
    k = np.arange(ntaps) - (ntaps - 1) / 2.0
    return 2.0 * fc / fs * np.sinc(2.0 * fc / fs * k) * np.hamming(ntaps)


# The banks start with one-tap filters, and the rx filter's tile overlap is taken from the longest filter over every channel
# (Stage::set_taps, P from taps_len): every channel gets a 301-tap filter first, then v a different one no longer than that (the form
# stays), or a longer one, which moves that shared form -- "set_filters_longer", held to rounding below
BASE_FILTER = 301
QRX_SETTERS = {
    "set_tune": lambda o, v: o.set_tune(v, 7000),
    "set_filters": lambda o, v: o.set_filters(v, _lowpass(161, 1200.0, 48000.0), np.zeros(161)),
    "set_filters_longer": lambda o, v: o.set_filters(v, _lowpass(1001, 1800.0, 48000.0), np.zeros(1001)),
}


@pytest.mark.parametrize("bank", ["rx", "process"])
@pytest.mark.parametrize("name", sorted(QRX_SETTERS))
@pytest.mark.parametrize("mode", [3, 9])
def test_quisk_bank_setter_on_one_channel(qh, bank, name, mode):
    """set_tune / set_filters on channel v only; set_agc is one setting for the whole bank (qh_qrx_set_agc, qh_qps_set_agc take no
    channel), so it has no one-channel form to test"""
    nch = 5
    fs = 192000 if bank == "rx" else 48000
    calls = [fs // 10, fs // 40, fs // 200, fs // 20, fs // 10]
    x = synth.make_input_numpy(nch, sum(calls), fs=float(fs))

    def make():
        o = qh.QuiskRxBank(nch, fs, mode) if bank == "rx" else qh.QuiskProcessBank(nch, fs, mode, 2700, playback_rate=48000)
        o.set_filters(-1, _lowpass(BASE_FILTER, 1800.0, 48000.0), np.zeros(BASE_FILTER))
        return o
    for v in _victims(nch):
        a, b = make(), make()
        res, pos = [], 0
        try:
            for k, n in enumerate(calls):
                if k == 2:
                    QRX_SETTERS[name](b, v)
                seg = np.ascontiguousarray(x[:, pos:pos + n])
                res.append((a.process_host(seg), b.process_host(seg), None, None))
                pos += n
        finally:
            a.close(); b.close()
        partner = _qrx_partner(mode, nch, v)
        if name == "set_filters_longer":              # a shared form moved: the others only change by rounding
            for k, (ya, yb, _, _) in enumerate(res):
                for c in range(nch):
                    if c != v and ya[c].size:
                        d = float(np.sqrt(np.sum(np.abs(ya[c] - yb[c]) ** 2) / max(np.sum(np.abs(ya[c]) ** 2), 1e-300)))
                        assert d < 1e-12, (k, c, v, d)
            continue
        _assert_isolated(res, nch, v, skip=(partner,))
        if bank == "rx":
            _assert_qrx_partner_bounded(res, v, partner)


def test_quisk_process_bank_squelch_and_noise_blanker(qh):
    nch, fs = 5, 48000
    calls = [4800, 1200, 480, 4800, 2400]
    x = synth.make_input_numpy(nch, sum(calls), fs=fs)

    def make():
        b = qh.QuiskProcessBank(nch, fs, 3, 2700, playback_rate=48000)
        b.set_noise_blanker(2)
        b.set_ssb_squelch(True, 60)
        return b
    for v in _victims(nch):
        xb = _alt(x, v, sum(calls[:2]), fs=fs, f_carrier=1500.0)
        # USB: the audio interpolator's pair form; the partner is exempt from the bit-for-bit check but not bounded here: the
        # bank's squelch and noise blanker are decisions on sample values, which a last-bit change may flip
        partner = _qrx_partner(3, nch, v)
        res = _differential(make, lambda o, s: o.process_host(s), x, xb, calls, side=lambda o: list(o.squelch_flags()))
        _assert_isolated(res, nch, v, skip=(partner,))


def test_quisk_agc(qh):
    nch = 5
    calls = [2400, 480, 4800, 1, 960]
    x = synth.make_input_numpy(nch, sum(calls), fs=48000.0)

    def make():
        a = qh.QuiskAgc(nch, 48000)
        a.set_agc(-1, 80.0)
        return a
    for v in _victims(nch):
        xb = _alt(x, v, sum(calls[:2]), fs=48000.0, f_carrier=1500.0)
        _assert_isolated(_differential(make, lambda o, s: o.process_host(s), x, xb, calls), nch, v)


def test_noise_blanker(qh):
    nch = 5
    calls = [6000, 1000, 12000, 7, 3000]
    x = synth.make_input_numpy(nch, sum(calls))
    for v in _victims(nch):
        xb = _alt(x, v, sum(calls[:2]), f_carrier=1500.0)
        res = _differential(lambda: qh.NoiseBlanker(nch, 192000, 2), lambda o, s: o.process_host(s), x, xb, calls)
        _assert_isolated(res, nch, v)


# ---------------------------------------------------------------------------------------------------------------- filter banks
def _gold(key):
    import os
    return np.load(os.path.join(os.path.dirname(__file__), "golden", "filter_golden.npz"))[key]


def _fir_make(qh, nch, kind, decim):
    taps = _gold("taps98")
    if kind == "complex":
        taps = taps * np.exp(2j * np.pi * 0.1 * np.arange(taps.size))
    return lambda: qh.FirBank(nch, taps, decim, dtype=1 if kind == "f32" else 0)


FIR_CALLS = [5000, 37, 4096, 1, 700, 9000]


@pytest.mark.parametrize("decim", [1, 2, 4, 8, 32])
@pytest.mark.parametrize("kind", ["f64", "f32", "complex"])
def test_fir_bank(qh, kind, decim):
    nch = 5
    x = synth.make_input_numpy(nch, sum(FIR_CALLS))
    if kind == "f32":
        x = x.astype(np.complex64)
    for v in _victims(nch):
        xb = _alt(x, v, sum(FIR_CALLS[:2]), f_carrier=1500.0)
        _assert_isolated(_differential(_fir_make(qh, nch, kind, decim), lambda o, s: o.process_host(s), x, xb, FIR_CALLS), nch, v)


@pytest.mark.parametrize("nstage", [4, 8])
@pytest.mark.parametrize("dtype", [0, 1], ids=["f64", "f32"])
def test_half_band_cascade(qh, nstage, dtype):
    nch = 5
    u = 1 << nstage
    calls = [u * 40, u, u * 300, u * 3]
    x = synth.make_input_numpy(nch, sum(calls))
    if dtype:
        x = x.astype(np.complex64)
    for v in _victims(nch):
        xb = _alt(x, v, sum(calls[:2]), f_carrier=100.0)
        res = _differential(lambda: qh.HalfBandCascade(nch, nstage, dtype=dtype), lambda o, s: o.process_host(s), x, xb, calls)
        _assert_isolated(res, nch, v)


@pytest.mark.parametrize("interp,decim", [(6, 5), (4, 5), (8, 1)])
def test_rational_fir(qh, interp, decim):
    nch = 5
    calls = [3000, 7, 1200, 1, 5000]
    x = synth.make_input_numpy(nch, sum(calls))
    for v in _victims(nch):
        xb = _alt(x, v, sum(calls[:2]), f_carrier=1500.0)
        res = _differential(lambda: qh.RationalFir(nch, _gold("taps98"), interp, decim), lambda o, s: o.process_host(s), x, xb, calls)
        _assert_isolated(res, nch, v)


# ---------------------------------------------------------------------------------------------------------------- display
def _pan_step(o, s):
    o.feed_host(s)
    g = o.get_graph()
    return None if g is None else g


@pytest.mark.parametrize("nch,fft_size,width", [(5, 4096, 1024), (5, 15360, 960), (64, 16384, 1024)], ids=["pow2", "bluestein", "64x16384"])
def test_panadapter(qh, nch, fft_size, width):
    calls = [fft_size * 2 + 17, 333, fft_size * 3, 1, fft_size * 2]
    x = synth.make_input_numpy(nch, sum(calls))
    for v in _victims(nch):
        xb = _alt(x, v, sum(calls[:2]), f_carrier=20000.0)
        raw = _differential(lambda: qh.Panadapter(nch, fft_size, width, 192000.0), _pan_step, x, xb, calls)
        res = []
        for ga, gb, _, _ in raw:
            assert (ga is None) == (gb is None)
            if ga is not None:
                res.append((ga[0], gb[0], list(ga[1]), list(gb[1])))
        assert res
        _assert_isolated(res, nch, v)


@pytest.mark.parametrize("ndisp", [4, 5])
def test_analyzer_bank_several_displays(qh, ndisp):
    """AnalyzerBank: one display's samples must not reach another display's pixel rows (they are found per call, like the
    panadapter's block ranges)"""
    from test_gpu_analyzer import RATE, _cfg
    size, bf, npix = 1024, 256, 500
    cfg = _cfg(size, bf, 512, npix)
    chunks = [3 * bf, bf, 5 * bf, 2 * bf, 8 * bf, bf, 4 * bf]
    x = synth.make_input_numpy(ndisp, sum(chunks), a1=0.3)

    def make():
        g = qh.AnalyzerBank(ndisp, size)
        g.SetDisplaySampleRate(RATE)
        g.SetAnalyzer(*cfg["args"])
        return g

    def step(g, seg):
        return g.rows_host(0) if g.feed_host(0, seg) else None
    for v in _victims(ndisp):
        xb = _alt(x, v, sum(chunks[:2]), f_carrier=20000.0)
        raw = _differential(make, step, x, xb, chunks)
        res = []
        for ra, rb, _, _ in raw:
            assert (ra is None) == (rb is None)
            if ra is not None:
                res.append((np.asarray(ra), np.asarray(rb), None, None))
        assert res
        _assert_isolated(res, ndisp, v)


# ---------------------------------------------------------------------------------------------------------------- ingest
def _hermes_bytes_of(nrx, r):
    """the byte offsets of a 512-byte Hermes frame that carry receiver r, found by the CPU restatement of the unpacking"""
    from oracle import ingest_oracle as io
    buf = np.random.default_rng(1).integers(0, 256, 512, dtype=np.uint8)
    base = io.hermes_frames(buf.tobytes(), nrx)
    own = []
    for i in range(512):
        b = buf.copy()
        b[i] ^= 0x55
        d = io.hermes_frames(b.tobytes(), nrx)
        if not np.array_equal(d[r], base[r]):
            own.append(i)
    return np.array(own)


@pytest.mark.parametrize("nrx", [3, 4])
def test_unpack_several_channels_in_one_frame(qh, nrx):
    """Hermes frames hold every receiver's samples interleaved: new bytes for receiver v leave the others' samples bit for bit"""
    from oracle import ingest_oracle as io
    nframes = 40
    buf = np.random.default_rng(nrx).integers(0, 256, 512 * nframes, dtype=np.uint8)
    fmt = qh.IqFormat.hermes(nrx)
    for v in _victims(nrx):
        own = _hermes_bytes_of(nrx, v)
        bb = buf.copy()
        idx = (np.arange(nframes)[:, None] * 512 + own[None, :]).ravel()
        bb[idx] = np.random.default_rng(100 + v).integers(0, 256, idx.size, dtype=np.uint8)
        n = io.hermes_frames(buf.tobytes(), nrx).shape[1]
        ya = qh.ingest.unpack_host(buf.tobytes(), fmt, nrx, 6, n)
        yb = qh.ingest.unpack_host(bb.tobytes(), fmt, nrx, 6, n)
        _assert_isolated([(ya, yb, None, None)], nrx, v)


def test_rxa_process_packed(qh):
    """qh_rxa_process_packed: 24-bit wire samples decoded in the front kernel's load, one channel's bytes replaced"""
    nch, calls = 5, [12, 3, 1, 20]
    n = sum(calls) * 1024
    x = synth.make_input_numpy(nch, n)
    fmt = qh.IqFormat.le24(1.0 / 2 ** 31)

    def wire(z):
        q = np.round(np.stack([z.real, z.imag], axis=1) * 2 ** 23).astype("<i4")
        return q.view(np.uint8).reshape(-1, 2, 4)[:, :, :3].reshape(-1)
    for v in _victims(nch):
        start = sum(calls[:2]) * 1024
        xb = _alt(x, v, start)
        xb[v, start:] *= 0.002                                 # another signal, scaled into the 24-bit range
        outs = []
        for src in (x, xb):
            raws = [wire(src[c]) for c in range(nch)]
            e = _rxa(qh, nch)()
            ys, pos = [], 0
            for nb in calls:
                lo, hi = pos * 1024 * 6, (pos + nb) * 1024 * 6
                ys.append(e.process_packed_host(b"".join(r[lo:hi].tobytes() for r in raws), fmt, hi - lo, nb))
                pos += nb
            e.close()
            outs.append(ys)
        _assert_isolated([(a, b, None, None) for a, b in zip(*outs)], nch, v)


# ---------------------------------------------------------------------------------------------------------------- pair partners
def test_pair_partner_coupling_is_rounding_only(qh):
    """The FM de-emphasis and AM / SAM bp1 stages run two real channels as one complex transform.  v's samples enter the
    partner's output only through that transform's rounding: per output sample at most ~ eps * log2(N) * max|stage signal| for
    each pass, so 64 eps * max|v's output| * sqrt(N) with N = 4096 (run_band's pair form launches kNfft = 4096-point tiles at
    nc 2048) is a bound with margin (sqrt(4096) = 64 against log2 = 12).  For AM / SAM the paired bp1 stage is the last filter, so
    max|v's output| is its stage output.  FM's paired stage is the de-emphasis: its output still holds the discriminator's
    out-of-band content, which the audio filter after it removes, so the API shows no stage output to put in the bound.  The FM
    partner is held to its oracle gate instead (1e-6 relative, tests/test_gpu_long_nc.py) and its coupling is printed.
    Fixed gain (AGC mode 0), so that no AGC branch amplifies the rounding change.  Every channel outside the pair bit-identical."""
    nch = 8
    eps = np.finfo(np.float64).eps
    nfft = 4096
    for v in (1, 2, 5, 6):                              # AM and FM channels of the mix (C4 by c mod 4)
        m = C4[v % 4]
        group = [c for c in range(nch) if C4[c % 4] == m]
        partner = _pair_partner(group, v)
        assert partner != v
        res = _run_rxa(qh, nch, v, modes=C4, sig=C4_SIG)
        _assert_isolated(res, nch, v, skip=(partner,))
        vmax = max(float(np.abs(yb[v]).max()) for _, yb, _, _ in res)
        worst = max(float(np.abs(ya[partner] - yb[partner]).max()) for ya, yb, _, _ in res)
        if m == 5:
            ya_p = np.concatenate([ya[partner] for ya, _, _, _ in res])
            yb_p = np.concatenate([yb[partner] for _, yb, _, _ in res])
            rel = float(np.sqrt(np.sum(np.abs(ya_p - yb_p) ** 2) / np.sum(np.abs(ya_p) ** 2)))
            print("pair (%d, %d) FM: partner moved by %.3e (%.1f eps max|v|), relative %.2e" % (v, partner, worst, worst / eps / vmax, rel))
            assert rel < 1e-6, (v, partner, rel)
            continue
        bound = 64 * eps * vmax * np.sqrt(nfft)
        print("pair (%d, %d) mode %d: partner moved by %.3e, bound %.3e" % (v, partner, m, worst, bound))
        assert worst <= bound, (v, partner, worst, bound)


# ---------------------------------------------------------------------------------------------------------------- non-finite bursts
BURST = (complex(np.nan, 0.0), complex(np.inf, 0.0), complex(0.0, -np.inf), complex(np.nan, np.nan))


def _burst(x, v, at):
    """four samples of NaN and +-Inf into channel v from input sample `at`"""
    y = x.copy()
    y[v, at:at + len(BURST)] = np.asarray(BURST, dtype=y.dtype)
    return y


def _assert_contained(res, nch, v, bound, out_pos=None):
    """others bit-identical in every call, v bit-identical from output sample `bound` on"""
    pos = 0
    for k, (ya, yb, _, _) in enumerate(res):
        n = ya.shape[1]
        for c in range(nch):
            if c != v:
                assert np.array_equal(ya[c], yb[c]), ("call", k, "channel", c)
        if pos >= bound:
            assert np.array_equal(ya[v], yb[v]), ("victim not recovered in call", k, "from", pos, "bound", bound,
                                                  int(np.sum(~np.isfinite(yb[v]))))
        elif pos + n > bound:
            assert np.array_equal(ya[v][bound - pos:], yb[v][bound - pos:]), ("victim not recovered", k, bound)
        pos += n
    assert pos > bound + 64, (pos, bound)          # the stream runs past the bound


def _direct_fir(x, taps, decim):
    y = np.convolve(x, taps)[:x.size]
    return y[::decim]


@pytest.mark.parametrize("dtype", [0, 1], ids=["f64", "f32"])
@pytest.mark.parametrize("calls", [[5000, 37, 4096, 1, 700, 9000], [40, 30, 97, 50, 33, 200, 64] * 20], ids=["long_calls", "calls_below_history"])
@pytest.mark.parametrize("decim", [1, 4])
def test_fir_bank_burst(qh, dtype, calls, decim):
    nch = 4
    taps = _gold("taps98")
    x = synth.make_input_numpy(nch, sum(calls))
    if dtype:
        x = x.astype(np.complex64)
    at = sum(calls) // 3
    for v in _victims(nch):
        xb = _burst(x, v, at)
        res = _differential(lambda: qh.FirBank(nch, taps, decim, dtype=dtype), lambda o, s: o.process_host(s), x, xb, calls)
        # the last input sample whose window holds the burst, plus one, plus one overlap-save tile (kStageNfft = 4096 points): a
        # tile that loads a non-finite sample spreads it over all its outputs through the transform
        end = at + 4 + taps.size + 4096
        bound = -(-end // decim) + 1
        _assert_contained(res, nch, v, bound)
        ref = _direct_fir(xb[v].astype(np.complex128), taps, decim)
        assert np.all(np.isfinite(ref[bound:])) and not np.all(np.isfinite(ref))


@pytest.mark.parametrize("nstage", [4, 8])
@pytest.mark.parametrize("dtype", [0, 1], ids=["f64", "f32"])
def test_half_band_cascade_burst(qh, nstage, dtype):
    nch = 4
    u = 1 << nstage
    calls = [u * 40, u, u * 300, u * 3, u * 200]
    x = synth.make_input_numpy(nch, sum(calls))
    if dtype:
        x = x.astype(np.complex64)
    at = u * 100 + 5
    # each HB45 stage's 43 taps at its own input rate: sum_s 43 * 2^s input samples <= 43 * 2^nstage, one output more
    bound = (at + 4 + 43 * u) // u + 2
    for v in _victims(nch):
        xb = _burst(x, v, at)
        res = _differential(lambda: qh.HalfBandCascade(nch, nstage, dtype=dtype), lambda o, s: o.process_host(s), x, xb, calls)
        _assert_contained(res, nch, v, bound)
        y = xb[v].astype(np.complex128)
        for _ in range(nstage):                          # the reference: quisk_cDecim2HB45 per stage, a 43-tap FIR then every 2nd
            y = _direct_fir(y, qh.hb45_taps(), 2)
        assert np.all(np.isfinite(y[bound:])) and not np.all(np.isfinite(y))


@pytest.mark.parametrize("interp,decim", [(6, 5), (4, 5), (8, 1)])
def test_rational_fir_burst(qh, interp, decim):
    nch = 4
    taps = _gold("taps98")
    calls = [3000, 7, 1200, 1, 5000, 4000]
    x = synth.make_input_numpy(nch, sum(calls))
    at = 4200
    bound = ((at + 4) * interp + taps.size) // decim + interp + 2
    for v in _victims(nch):
        xb = _burst(x, v, at)
        res = _differential(lambda: qh.RationalFir(nch, taps, interp, decim), lambda o, s: o.process_host(s), x, xb, calls)
        _assert_contained(res, nch, v, bound)
        up = np.zeros(xb[v].size * interp, dtype=np.complex128)
        up[::interp] = xb[v]
        with np.errstate(invalid="ignore"):
            ref = _direct_fir(up, taps, decim)
        assert np.all(np.isfinite(ref[bound:]))


def _rxa_burst_bound(at_in, nc):
    """first output sample (48 kHz) from which an SSB chain is clean again after a burst ending at input sample at_in (192 kHz):
    the front stage's tile at the input rate (4096 samples), nbp0's own nc, one DSP block and one band tile (8192 points)"""
    return (at_in + 4 + 4096) // 4 + nc + 256 + 8192


@pytest.mark.parametrize("nc_v", [2048, 4096, 8192])
def test_partitioned_stage_burst_recovers_within_own_nc(qh, oracle, nc_v):
    """Channel 1 at nc 65536 runs nbp0 in 16 partitions for every channel; the victim's own nc is shorter.  Before the fix the
    victim's output stayed non-finite for 16 x 4096 samples after the burst (NaN x zero mask); the reference recovers after
    its own nc."""
    nch, v = 3, 0
    calls = [40, 30, 1, 60, 7, 90, 2, 100, 30]           # 360 DSP blocks: 92160 outputs, more than 65536 past the burst
    x = synth.make_input_numpy(nch, sum(calls) * 1024)
    at = 45 * 1024 + 100
    xb = _burst(x, v, at)
    res = _differential(_rxa(qh, nch, nc={v: nc_v, 1: 65536, 2: 8192}), _rxa_step, x, xb, [c * 1024 for c in calls])
    bound = _rxa_burst_bound(at, nc_v)
    assert not np.all(np.isfinite(np.concatenate([yb[v] for _, yb, _, _ in res])))
    _assert_contained(res, nch, v, bound)
    o = oracle.WdspChannel(1024, 256, 192000, 48000, 48000)
    o.SetRXAShiftRun(1); o.SetRXAShiftFreq(synth.shift_freq(v)); o.RXANBPSetRun(1); o.SetRXAMode(1)
    o.RXASetPassband(*PASSBAND[1]); o.RXASetNC(nc_v); o.SetRXAAGCMode(0); o.SetRXAAGCFixed(3.0)
    with np.errstate(invalid="ignore", over="ignore"):
        ref = o.xrxa(xb[v])
    assert np.all(np.isfinite(ref[bound:])) and not np.all(np.isfinite(ref))


def test_partitioned_stage_shrink_and_regrow_with_a_burst_between(qh):
    """channel 1's nc 65536 -> 8192 (K 16 -> 2), a burst into the victim, then 65536 again (K back to 16): the
    victim (nc 8192) must not pick its burst or stale samples up from the part of its row the longer form exposes again."""
    nch, v = 3, 0
    plan = [(40, 65536), (30, None), (60, 8192), (40, None), (30, 65536), (200, None)]
    x = synth.make_input_numpy(nch, sum(p[0] for p in plan) * 1024)
    at = 150 * 1024 + 10                                # inside the stretch at K = 2
    xb = _burst(x, v, at)
    make = _rxa(qh, nch, nc={v: 8192, 1: 65536, 2: 2048})
    a, b = make(), make()
    res, pos = [], 0
    try:
        for nb, nc1 in plan:
            if nc1:
                a.RXASetNC(1, nc1); b.RXASetNC(1, nc1)
            res.append((a.process_host(np.ascontiguousarray(x[:, pos * 1024:(pos + nb) * 1024])),
                        b.process_host(np.ascontiguousarray(xb[:, pos * 1024:(pos + nb) * 1024])), None, None))
            pos += nb
    finally:
        a.close(); b.close()
    _assert_contained(res, nch, v, _rxa_burst_bound(at, 8192))


@pytest.mark.parametrize("nch,fft_size,width", [(5, 4096, 1024), (5, 15360, 960)], ids=["pow2", "bluestein"])
def test_panadapter_burst(qh, nch, fft_size, width):
    """the victim's pixels go non-finite, the others' do not move"""
    calls = [fft_size * 2 + 17, 333, fft_size * 3, 1, fft_size * 2]
    x = synth.make_input_numpy(nch, sum(calls))
    for v in _victims(nch):
        xb = _burst(x, v, fft_size * 2 + 200)
        raw = _differential(lambda: qh.Panadapter(nch, fft_size, width, 192000.0), _pan_step, x, xb, calls)
        hit = False
        for ga, gb, _, _ in raw:
            if ga is None:
                continue
            for c in range(nch):
                if c != v:
                    assert np.array_equal(ga[0][c], gb[0][c]) and ga[1][c] == gb[1][c], c
            hit = hit or not np.all(np.isfinite(gb[0][v]))
        assert hit
