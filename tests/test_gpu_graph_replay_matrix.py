"""qh_rxa_set_graph_replay across the engine's stages: a call replayed from a captured hipGraph must leave the bits a plain call leaves.

The replay rests on one rule (qh_engine.hpp, struct Engine): the host side of process() changes nothing from call to call but the six
ping-pong flags.  A stage that keeps anything else per call on the host -- a ring index, a carry slot, a kernel argument passed by
value -- works on the plain path and replays a stale argument from the graph.  This file holds every stage to that rule.

1. The stage matrix (ROWS, test_replayed_equals_plain).  One stream goes through a plain and through a replaying engine on fixed
   device buffers, at 1 and 4 blocks per call and, where a stage has a time-tiled form, at 64 or 128.  Outputs and meters are equal
   bit for bit, finite and not silent.  The replay count is derived from the number of calls, so an engine that silently stopped
   replaying turns the row red.  A last chunk goes through process_host, which never replays, so it starts from the flags the
   replays left on the host.

2. The replayed engine against a reference (test_replayed_against_oracle), one block per call, so that the pair of engines cannot be
   wrong together.  The reference is the CPU oracle (oracle/wdsp_oracle.c).  It has no xssql, xcbl, xspeak or xmpeak: rows with those
   stages are compared with the restatements (tests/rxa_ssql_ref.py, tests/rxa_audio_peak_ref.py) applied to the output of a plain
   engine that has the stages off and an identity panel, and that engine is compared with the oracle.  Every tolerance and every
   settle span is the one an existing parity test asserts:

   - 1e-6 relative RMS: the fp64 chain (test_gpu_rxa_fuzz.py);
   - 1e-4: rows in which ANF or ANR runs (test_gpu_rxa_fuzz.py);
   - 1e-9: against the restatements (test_gpu_rxa_ssql.py, test_gpu_rxa_audio_peak.py);
   - 1e-5: a channel of the seeded walk once SNBA has run on it (the walk of test_gpu_snba_parity.py);
   - FM, and rows with an FM channel: compared from block 150 on, the loop's start-up (test_gpu_demod_parity.py; DESIGN.md, parity
     caveat);
   - SAM: compared from block 3900 on, as test_gpu_demod_parity.py compares SAM with the fade leveller.  Its 1.4 s average
     remembers the pull-in; 2.4e-5 is still left 320 blocks in;
   - the FM row's low-SNR channel gives the verify pass repairs to do.  A loop that slips amplifies last-bit differences, so that
     channel is held bit for bit only, like the carrier-less channels of test_gpu_tiled_detectors.py;
   - nc_65536: one USB and one AM channel are held to the oracle; the other two differ from them in shift and noise seed only.

3. Events between replayed calls (EVENTS, test_events_between_replayed_calls): the entry points that never replay but move the same
   flags, the synchronising getters, the flush, the band tile preference, replay off and on, and a setter of each newer stage.  Each
   event comes once before an even and once before an odd call (AT), so each of the two graph slots is the next one to run once.
   A packed, audio or host call stands in place of a process_ptr call and moves the flags as that call would have: it shows that the
   slots are still right afterwards, not that another slot is reached.

4. A seeded walk over the setters that test_gpu_rxa_fuzz.py's menus predate (_apply3), block at a time, against a plain twin bit for
   bit and against restatement and oracle.

Cost, measured on one MI355X: 62 s for the 160 tests, beside 33 s for tests/test_gpu_rxa_fuzz.py on the same machine.  The CPU
oracle convolving 65536 taps is the largest part (16 s for nc_65536, whose AM channel needs 257 blocks to be heard at all, 8 s for the
row beside it); the bit-equality rows, the events and the walk together take about 30 s.  -m gpu."""
import numpy as np
import pytest
import torch          # before libquiskhip: one HIP runtime per process (torch's), as in bench.py

from conftest import rel_rms
from quisk_amd import synth
from rxa_audio_peak_ref import AudioPeakChain, panel
from rxa_ssql_ref import Ssql, edges, syllabic
from test_gpu_rxa_parity import _agc_signal
from test_gpu_snba_parity import crackle

pytestmark = pytest.mark.gpu

LSB, USB, CWL, CWU, FM, AM, SAM = 0, 1, 3, 4, 5, 6, 10
STAGE_PREFIXES = ("SetRXASSQL", "SetRXASPCW", "SetRXAmpeak", "SetRXACBL")      # stages the C oracle does not have: restated in Python
# (a configuration is a list of (name, channel, args...): a setter for that channel, -1 for all; channel None: an engine-level call)
METERS = range(7)                                                              # S, ADC and AGC meters, peak and average, and the AGC gain


def _passband(mode):
    return (-8000.0, 8000.0) if mode == FM else (-4000.0, 4000.0) if mode in (AM, SAM) else (-3000.0, -300.0) if mode in (LSB, CWL) else \
        (300.0, 3000.0)


def _chans(modes, shift=synth.shift_freq):
    out = []
    for c, m in enumerate(modes):
        out += [("SetRXAShiftRun", c, 1), ("SetRXAShiftFreq", c, shift(c)), ("RXANBPSetRun", c, 1), ("SetRXAMode", c, m),
                ("RXASetPassband", c) + _passband(m)]
    return out


# ---- inputs -----------------------------------------------------------------------------------------------------------------------
def _in_default(modes, n, fs=192000.0):
    x = np.empty((len(modes), n), dtype=np.complex128)
    for c, m in enumerate(modes):
        x[c] = synth.make_mode_input_numpy("fm" if m == FM else "am" if m in (AM, SAM) else "usb", c, n, fs=fs)
    return x


def _in_bursts(modes, n, fs=192000.0):
    """test_gpu_rxa_ssql.py's syllabic tone, gated 80 ms on / 80 ms off so that the squelch opens and closes within 64 blocks"""
    t = np.arange(n) / fs
    x = np.empty((len(modes), n), dtype=np.complex128)
    for c, m in enumerate(modes):
        z = syllabic(n, fs, seed=c, on=0.08, off=0.08)
        car = np.exp(-2j * np.pi * ((synth.shift_freq(c) * t) % 1.0))
        x[c] = (0.1 + 0.05 * z.real) * car if m in (AM, SAM) else 0.3 * (np.conj(z) if m in (LSB, CWL) else z) * car
    return x


def _in_fm_low_snr(modes, n, fs=192000.0):
    x = _in_default(modes, n, fs)
    x[-1] = synth.make_mode_input_numpy("fm", len(modes) - 1, n, fs=fs, sigma=0.08)      # carrier 0.1: the loop slips now and then
    return x


def _in_crackle(modes, n, fs=192000.0):
    return np.stack([crackle(c, n, m, rate=25.0) for c, m in enumerate(modes)])


def _in_fades(modes, n, fs=192000.0):
    """64 ms at full level, 64 ms 60 dB down, in turn: the AM squelch closes all the way to exact zeros, and opens again"""
    t = np.arange(n) / fs
    return _in_default(modes, n, fs) * np.where((t % 0.128) < 0.064, 1.0, 1e-3)


def _in_steps(modes, n, fs=192000.0):
    return np.stack([_agc_signal(n, fs) for _ in modes])


# ---- the rows ---------------------------------------------------------------------------------------------------------------------
def _row(modes, extra=(), nblks=(1, 4), make=_in_default, tol=1e-6, settle=0, rates=(192000, 48000, 48000), ncalls=None, meters=True,
         shift=synth.shift_freq, oracle_chans=None, replays=True):
    cfg = _chans(modes, shift) + list(extra)
    if not any(c[0] == "enable_meters" for c in cfg):
        cfg.append(("enable_meters", None, meters))
    return dict(modes=modes, cfg=cfg, nblks=nblks, make=make, tol=tol, settle=settle, rates=rates, ncalls=ncalls or {}, replays=replays,
                oracle_chans=oracle_chans)


SSQL_ON = [("SetRXASSQLRun", -1, 1), ("SetRXASSQLThreshold", -1, 0.3), ("SetRXASSQLTauMute", -1, 0.01), ("SetRXASSQLTauUnMute", -1, 0.01)]


def _speak(c):
    return [("SetRXASPCWFreq", c, 800.0), ("SetRXASPCWBandwidth", c, 50.0), ("SetRXASPCWGain", c, 1.5), ("SetRXASPCWRun", c, 1)]


def _mpeak(c):
    return [("SetRXAmpeakFilEnable", c, 0, 1), ("SetRXAmpeakFilEnable", c, 1, 1), ("SetRXAmpeakFilFreq", c, 0, 1000.0),
            ("SetRXAmpeakFilBw", c, 0, 100.0), ("SetRXAmpeakFilFreq", c, 1, 1400.0), ("SetRXAmpeakFilGain", c, 1, 2.0), ("SetRXAmpeakRun", c, 1)]


def _mpeak_wide(c):
    return [("SetRXAmpeakFilFreq", c, 0, 700.0), ("SetRXAmpeakFilBw", c, 0, 600.0), ("SetRXAmpeakFilFreq", c, 1, 1600.0),
            ("SetRXAmpeakFilBw", c, 1, 600.0), ("SetRXAmpeakRun", c, 1)]


def _nr(run, pos):
    return [(run, 0, 1), (run, 1, 1), (run, 2, 1), (run, 3, 1)] + [(pos, c, c & 1) for c in range(4)]


# a 65536-tap linear-phase filter delays by 128 blocks of 256, an AM channel's two by 256: the stream must outlast that to be heard
LONG, LONG2 = {1: 168, 4: 42, 64: 12}, {1: 288, 4: 72, 64: 12}
ROWS = {
    "ssql": _row([USB, AM, USB, AM], SSQL_ON, make=_in_bursts, ncalls={1: 64, 4: 16}),
    "audio_peak_apart": _row([CWU, USB, AM, USB], _speak(0) + _mpeak(1) + [("SetRXACBLRun", 2, 1)], nblks=(1, 4, 64)),
    "audio_peak_together": _row([CWU, USB, AM, USB], _speak(0) + _mpeak(0) + [("SetRXACBLRun", 0, 1)] + _speak(2) + _mpeak(2) +
                                [("SetRXACBLRun", 2, 1)], nblks=(1, 4, 64)),
    # the stages behind one another behind the AGC, on a channel without bp1 (USB) and on one with it (AM), beside channels without
    # the squelch.  (Wide peaks: behind the 50 Hz CW peak the syllabic detector hears one steady tone and never opens.)
    "ssql_audio_peak_agc": _row([USB, AM, USB, AM], [("SetRXAAGCMode", -1, 3)] + SSQL_ON[1:] + [("SetRXASSQLRun", 0, 1), ("SetRXASSQLRun", 1, 1)] +
                                _mpeak_wide(0) + _mpeak_wide(1) + [("SetRXACBLRun", 0, 1), ("SetRXACBLRun", 1, 1)] + _speak(2) + _mpeak(3),
                                nblks=(1, 4, 64), make=_in_bursts, ncalls={1: 64, 4: 16}),
    "fm": _row([FM] * 4, [("SetRXACTCSSRun", 0, 1), ("SetRXACTCSSRun", 1, 0), ("SetRXAFMLimRun", 1, 1), ("SetRXAFMLimGain", 1, 0.4),
                          ("SetRXACTCSSRun", 2, 1), ("SetRXAFMLimRun", 2, 1), ("SetRXAFMLimGain", 2, 0.4), ("SetRXACTCSSRun", 3, 0)],
               nblks=(1, 4, 64), make=_in_fm_low_snr, settle=150, oracle_chans=(0, 1, 2)),
    "sam": _row([SAM] * 6, [("SetRXAAMDSBMode", c, c % 3) for c in range(6)] + [("SetRXAAMDFadeLevel", c, c // 3) for c in range(6)],
                nblks=(1, 4, 128), settle=3900),
    "snba": _row([USB, AM, USB, AM], [("SetRXASNBARun", -1, 1)], make=_in_crackle),
    "emnr": _row([USB, USB, AM, AM], [("load_emnr_tables", None)] + _nr("SetRXAEMNRRun", "SetRXAEMNRPosition"), ncalls={1: 48}),
    "anf": _row([USB, USB, AM, AM], _nr("SetRXAANFRun", "SetRXAANFPosition"), tol=1e-4),
    "anr": _row([USB, USB, AM, AM], _nr("SetRXAANRRun", "SetRXAANRPosition"), tol=1e-4),
    "amsq": _row([AM, AM, USB, AM], [("SetRXAAMSQRun", -1, 1), ("SetRXAAMSQThreshold", -1, -40.0), ("SetRXAAMSQMaxTail", -1, 0.02)],
                 make=_in_fades, ncalls={1: 48, 4: 12}),
    "nc_8192": _row([USB, AM, USB, AM], [("RXASetNC", -1, 8192)], nblks=(1, 4, 64), ncalls={1: 48, 4: 12}),
    "nc_65536": _row([USB, AM, USB, AM], [("RXASetNC", -1, 65536)], nblks=(1, 4, 64), ncalls=LONG2, oracle_chans=(0, 1)),
    "nc_2048_beside_65536": _row([USB, USB, AM, AM], [("RXASetNC", 1, 65536), ("RXASetNC", 3, 8192)], nblks=(1, 4, 64), ncalls=LONG),
    "mp": _row([USB, FM, USB, FM], [("RXASetMP", -1, 1)], settle=150),
    "band_tile_8192": _row([USB, AM, FM, USB], [("set_band_tile", None, 8192)], settle=150),
    "band_tile_6144": _row([USB, AM, FM, USB], [("set_band_tile", None, 6144)], settle=150),
    "agc": _row([USB] * 4, [("SetRXAAGCMode", 0, 0), ("SetRXAAGCFixed", 0, 20.0), ("SetRXAAGCMode", 1, 1), ("SetRXAAGCMode", 2, 2),
                            ("SetRXAAGCMode", 3, 4), ("SetRXAAGCHangThreshold", -1, 50)], nblks=(1, 4, 64), make=_in_steps,
                shift=lambda c: synth.shift_freq(0), ncalls={1: 60}),
    "meters_off": _row([USB, AM, FM, USB], meters=False, settle=150),
    "rate_48000": _row([USB, AM, USB, AM], rates=(48000, 48000, 48000)),
    "rate_768000": _row([USB, AM, USB, AM], rates=(768000, 48000, 48000)),
    # a resampler object at either end keeps a phase and a ping-pong of its own on the host: the engine stays on the plain path
    "rate_144000_stays_plain": _row([USB, AM, USB, AM], rates=(144000, 48000, 48000), replays=False),
    "out_96000_stays_plain": _row([USB, AM, USB, AM], rates=(192000, 48000, 96000), replays=False),
}
CASES = [(name, nb) for name, r in ROWS.items() for nb in r["nblks"]]


def _apply_cfg(e, cfg):
    for name, ch, *args in cfg:
        if ch is None:
            getattr(e, name)(*args)
        else:
            getattr(e, name)(ch, *args)


def _engine(qh, row, cfg=None):
    e = qh.RxaEngine(len(row["modes"]), in_rate=row["rates"][0], dsp_rate=row["rates"][1], out_rate=row["rates"][2])
    _apply_cfg(e, row["cfg"] if cfg is None else cfg)
    return e


def _meters(e, nch):
    return [[e.GetRXAMeter(c, mt) for mt in METERS] for c in range(nch)]


def run(qh, row, replay, nblk_per_call, ncalls, x=None):
    """One continuous stream through process_ptr on fixed device buffers (the replay key holds the pointers).
    A tail of _tail(nblk_per_call) blocks then goes through process_host, which never replays: it runs from the flags the replays left
    on the host (ncalls is even, so that a flag the replays forgot to move is on the wrong side by then).
    Returns (outputs [nch, (ncalls * nblk_per_call + tail) * dsp_outsize], meters, graph_launches, band_tile, pll_repairs)."""
    nch = len(row["modes"])
    e = _engine(qh, row)
    try:
        e.set_graph_replay(replay)
        ni, no = nblk_per_call * e.dsp_insize, nblk_per_call * e.dsp_outsize
        tail = _tail(nblk_per_call)
        if x is None:
            x = row["make"](row["modes"], ncalls * ni + tail * e.dsp_insize, fs=float(row["rates"][0]))
        assert ncalls % 2 == 0 and x.shape[1] == ncalls * ni + tail * e.dsp_insize
        dev = torch.device("cuda:0")
        d_in = torch.zeros((nch, ni), dtype=torch.complex128, device=dev)
        d_out = torch.zeros((nch, no), dtype=torch.complex128, device=dev)
        y = np.empty((nch, ncalls * no + tail * e.dsp_outsize), dtype=np.complex128)
        for k in range(ncalls):
            d_in.copy_(torch.from_numpy(np.ascontiguousarray(x[:, k * ni:(k + 1) * ni])))
            torch.cuda.synchronize()
            e.process_ptr(d_in.data_ptr(), ni, d_out.data_ptr(), no, nblk_per_call)
            e.synchronize()
            y[:, k * no:(k + 1) * no] = d_out.cpu().numpy()
        launches = e.graph_launches()
        y[:, ncalls * no:] = e.process_host(np.ascontiguousarray(x[:, ncalls * ni:]))
        return y, _meters(e, nch), launches, e.band_tile(), e.pll_repairs()
    finally:
        e.close()


def _tail(nb):
    """blocks in the closing process_host call: SNBA's repairs leave the chain three blocks after their input, so one block would not
    show a history taken from the wrong side"""
    return max(nb, 8)


def _ncalls(row, nb):
    n = max(12, row["ncalls"].get(nb, 12))
    return n + (n & 1)


# ---- 1. replay == plain, bit for bit -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,nb", CASES, ids=["%s-%d" % c for c in CASES])
def test_replayed_equals_plain(qh, name, nb):
    row = ROWS[name]
    ncalls = _ncalls(row, nb)
    plain, m_plain, l_plain, tile_plain, _ = run(qh, row, False, nb, ncalls)
    rep, m_rep, l_rep, tile_rep, repairs = run(qh, row, True, nb, ncalls)
    print("%s, %d blocks x %d calls: %d graph launches, band tile %d, pll repairs %d, peak %.3e" %
          (name, nb, ncalls, l_rep, tile_rep, repairs, np.abs(plain).max()), flush=True)
    assert l_plain == 0
    if row["replays"]:
        # every live ping-pong flag flips with every call, so a steady stream visits two flag states: the first call runs plain,
        # the next two are captured (and launched), the rest are replays
        assert l_rep >= ncalls - 3, (l_rep, ncalls)
    else:
        assert l_rep == 0
    assert np.all(np.isfinite(plain))
    no = plain.shape[1] * nb // (ncalls * nb + _tail(nb))
    assert np.abs(plain[:, 3 * no:]).max() > 1e-3           # heard in the replayed span
    if name.startswith("nc_"):
        assert all(np.abs(plain[c, 3 * no:]).max() > 1e-3 for c in range(len(row["modes"])))      # the 65536-tap channels too
    if "ssql" in name or name == "amsq":                    # the squelch opens and closes inside the replayed span
        for c in [c for c in range(len(row["modes"])) if name != "ssql_audio_peak_agc" or c < 2]:
            shut = plain[c, 3 * no:] == 0
            opens, closes = int(np.sum(shut[:-1] & ~shut[1:])), int(np.sum(~shut[:-1] & shut[1:]))
            assert opens >= 1 and closes >= 1, (c, opens, closes)
    if "band_tile" in name:
        assert tile_plain == tile_rep == int(name[-4:])
    bad = [k for k in range(ncalls) if not np.array_equal(plain[:, k * no:(k + 1) * no], rep[:, k * no:(k + 1) * no])]
    assert not bad, "calls that differ from the plain engine's: %r" % bad
    assert np.array_equal(plain[:, ncalls * no:], rep[:, ncalls * no:]), "the process_host call behind the replays differs"
    assert m_plain == m_rep


# ---- 2. the replayed engine against the oracle ---------------------------------------------------------------------------------------
def _is_stage(call):
    return call[0].startswith(STAGE_PREFIXES)


def _oracle_channel(oracle, row, c, cfg=None, gain1=None):
    ni = 256 * row["rates"][0] // row["rates"][1]
    o = oracle.WdspChannel(ni, 256, *row["rates"])
    for name, ch, *args in (row["cfg"] if cfg is None else cfg):
        if ch is not None and ch in (c, -1) and not _is_stage((name,)):
            getattr(o, name)(*args)
    if gain1 is not None:
        o.SetRXAPanelGain1(gain1)
    return o


def _restatement(row, c, cfg=None):
    ap, sq = AudioPeakChain(float(row["rates"][1])), Ssql(row["rates"][1])
    for name, ch, *args in (row["cfg"] if cfg is None else cfg):
        if ch in (c, -1) and _is_stage((name,)):
            getattr(sq if name.startswith("SetRXASSQL") else ap, name)(*args)
    return ap, sq


@pytest.mark.parametrize("name", list(ROWS))
def test_replayed_against_oracle(qh, oracle, name):
    row = ROWS[name]
    nch = len(row["modes"])
    ncalls = max(_ncalls(row, 1), row["settle"] + 42)
    ni = 256 * row["rates"][0] // row["rates"][1]
    ncalls += ncalls & 1
    x = row["make"](row["modes"], (ncalls + _tail(1)) * ni, fs=float(row["rates"][0]))
    y, _, launches, _, _ = run(qh, row, True, 1, ncalls, x=x)
    assert launches >= ncalls - 3 if row["replays"] else launches == 0
    ncalls += _tail(1)                                      # (the blocks that went through process_host behind the replays)
    no = y.shape[1] // ncalls
    lo = row["settle"] * no
    staged = any(_is_stage(c) for c in row["cfg"])
    if staged:
        # the stage-off twin, identity panel, plain launches, the same call shapes
        b = _engine(qh, row, [c for c in row["cfg"] if not _is_stage(c)] + [("SetRXAPanelGain1", -1, 1.0)])
        try:
            yb = np.concatenate([b.process_host(np.ascontiguousarray(x[:, k * ni:(k + 1) * ni])) for k in range(ncalls)], axis=1)
        finally:
            b.close()
    for c in (row["oracle_chans"] or range(nch)):
        ref = _oracle_channel(oracle, row, c, gain1=1.0 if staged else None).xrxa(x[c])
        assert np.all(np.isfinite(ref)) and np.abs(ref[lo:]).max() > 1e-3, (c, np.abs(ref[lo:]).max())
        tol = row["tol"]
        if staged:
            err_b = rel_rms(yb[c, lo:], ref[lo:])
            ap, sq = _restatement(row, c)
            want = panel(sq.process(ap.process(yb[c])))
            err = rel_rms(y[c], want)
            print("%s channel %d: against the restatement %.3e, its stage-off twin against the oracle %.3e" % (name, c, err, err_b), flush=True)
            assert err_b < tol, (c, err_b)
            if sq.run:
                op, cl = edges(sq.gain[3 * no:])
                assert op >= 1 and cl >= 1, (c, op, cl)
                assert not np.any(y[c][sq.gain == 0.0])
            assert err < 1e-9, (c, err)
        else:
            err = rel_rms(y[c, lo:], ref[lo:])
            print("%s channel %d: against the oracle %.3e" % (name, c, err), flush=True)
            assert err < tol, (c, err)


# ---- 3. events between replayed calls ----------------------------------------------------------------------------------------------
EVENT_ROWS = ["fm", "sam", "ssql_audio_peak_agc", "nc_8192", "snba"]
NCALLS3 = 40
AT = (8, 21)            # the events arrive before an even and before an odd call: both parities of the ping-pong flags
# What an event costs in replays.  A call through another entry point is itself no replay and leaves the graphs alone: 1.  The getters
# change nothing: 0.  Whatever moves the parameter epoch or drops the graphs costs 3: process_replayed runs one plain call under the
# new key, then captures one graph per flag state, and a steady stream has two states (the captures launch too, so 3 is an upper bound)
SETTERS3 = {"set_ssql_threshold": ("SetRXASSQLThreshold", 0.25), "set_spcw_freq": ("SetRXASPCWFreq", 700.0),
            "set_mpeak_gain": ("SetRXAmpeakFilGain", 0, 1.7), "set_cbl_run": ("SetRXACBLRun", 1), "set_fm_lim_gain": ("SetRXAFMLimGain", 3.0),
            "set_ctcss_freq": ("SetRXACTCSSFreq", 100.0), "set_nc": ("RXASetNC", 4096)}
EVENTS = {"packed": 1, "audio": 1, "host": 1, "getters": 0, "flush": 3, "band_tile": 3 + 3, "replay_off": 3 + 3}
EVENTS.update({k: 3 for k in SETTERS3})


def _quantise24(x):
    """the stream as 24-bit ADC codes (what the wire format carries) and those codes back as doubles: the same values exactly"""
    q = np.clip(np.round(np.stack([x.real, x.imag], axis=-1) * 2 ** 23), -2 ** 23, 2 ** 23 - 1).astype("<i4")
    return q, (q[..., 0] + 1j * q[..., 1]) / 2.0 ** 23


def _scripted(qh, row, x, q, event, replay):
    """NCALLS3 single-block calls with `event` at AT.  Returns (per-call outputs -- complex rows, or the audio bytes of an audio call --,
    meters, graph launches, band tile after every call)."""
    nch = len(row["modes"])
    e = _engine(qh, row)
    outs, tiles = [], []
    try:
        e.set_graph_replay(replay)
        dev = torch.device("cuda:0")
        d_in = torch.zeros((nch, 1024), dtype=torch.complex128, device=dev)
        d_out = torch.zeros((nch, 256), dtype=torch.complex128, device=dev)
        d_pk = torch.zeros((nch, 1024 * 6), dtype=torch.uint8, device=dev)
        afmt = qh.AudioFormat("f32")
        d_aud = torch.zeros((nch, 256 * afmt.frame_bytes), dtype=torch.uint8, device=dev)
        pfmt = qh.IqFormat.le24(1.0 / 2 ** 31)
        for k in range(NCALLS3):
            blk = np.ascontiguousarray(x[:, k * 1024:(k + 1) * 1024])
            how = "ptr"
            for at in AT:
                if event == "band_tile" and k in (at, at + 4):
                    e.set_band_tile(8192 if k == at else 0)
                elif event == "replay_off" and k in (at, at + 3) and replay:
                    e.set_graph_replay(k != at)
                elif k != at:
                    continue
                elif event in ("packed", "audio", "host"):
                    how = event
                elif event == "getters":
                    e.GetRXAMeter(0, 0), e.pll_repairs(), e.agc_repairs()
                elif event == "flush":
                    e.flush()
                elif event in SETTERS3:
                    getattr(e, SETTERS3[event][0])(-1, *SETTERS3[event][1:])
            if how == "host":
                outs.append(e.process_host(blk))
                tiles.append(e.band_tile())
                continue
            if how == "packed" and replay:
                # 3 bytes of I, 3 of Q per sample, little-endian, channel rows back to back; the plain twin takes the same values as doubles
                raw = np.ascontiguousarray(q[:, k * 1024:(k + 1) * 1024].view(np.uint8).reshape(nch, 1024, 2, 4)[..., :3]).reshape(nch, 6144)
                d_pk.copy_(torch.from_numpy(raw))
                torch.cuda.synchronize()
                e.process_packed_ptr(d_pk.data_ptr(), nch * 6144, pfmt, 6144, d_out.data_ptr(), 256, 1)
            else:
                d_in.copy_(torch.from_numpy(blk))
                torch.cuda.synchronize()
                if how == "audio":
                    e.process_audio_ptr(d_in.data_ptr(), 1024, d_aud.data_ptr(), 256 * afmt.frame_bytes, 1, afmt)
                else:
                    e.process_ptr(d_in.data_ptr(), 1024, d_out.data_ptr(), 256, 1)
            e.synchronize()
            outs.append((d_aud if how == "audio" else d_out).cpu().numpy().copy())
            tiles.append(e.band_tile())
        return outs, _meters(e, nch), e.graph_launches(), tiles
    finally:
        e.close()


CASES3 = [(r, ev) for r in EVENT_ROWS for ev in EVENTS]


@pytest.mark.parametrize("name,event", CASES3, ids=["%s-%s" % c for c in CASES3])
def test_events_between_replayed_calls(qh, name, event):
    row = ROWS[name]
    q, x = _quantise24(row["make"](row["modes"], NCALLS3 * 1024))
    plain, m_plain, l_plain, t_plain = _scripted(qh, row, x, q, event, False)
    rep, m_rep, l_rep, t_rep = _scripted(qh, row, x, q, event, True)
    bound = NCALLS3 - 3 - len(AT) * EVENTS[event]
    print("%s / %s: %d graph launches of %d calls (bound %d), band tiles %r" % (name, event, l_rep, NCALLS3, bound, sorted(set(t_rep))), flush=True)
    assert l_plain == 0
    assert l_rep >= bound, (l_rep, bound)
    assert all(np.all(np.isfinite(o)) for o in plain if o.dtype == np.complex128)
    bad = [k for k in range(NCALLS3) if not np.array_equal(plain[k], rep[k])]
    assert not bad, "calls that differ from the plain twin: %r" % bad
    assert t_plain == t_rep, (t_plain, t_rep)
    if event == "band_tile":
        assert 8192 in t_plain
    assert m_plain == m_rep


# ---- 4. a seeded walk over the newer setters ---------------------------------------------------------------------------------------
NCH = 4
GAPS = (0, 1, 2, 3, 5, 8, 13)


def _apply3(rng, targets, fm):
    """One setter of the stages that test_gpu_rxa_fuzz.py's menus predate -- SSQL, the audio peak filters, SNBA, the FM limiter -- or a
    mode change (FM on the one channel that may: one FM filter length per engine).  targets: (object, leading args) pairs."""
    k = int(rng.integers(0, 16 if fm else 13))
    done = []

    def call(name, *args):
        done.append((name,) + args)
        for t, lead in targets:
            getattr(t, name)(*lead, *args)
    if k == 0:
        call("SetRXAMode", int(rng.choice([FM, FM, USB]) if fm else rng.choice([USB, AM, CWU, LSB])))
    elif k == 1:
        call("SetRXASSQLRun", int(rng.integers(0, 2)))
    elif k == 2:
        call("SetRXASSQLThreshold", float(rng.choice([0.1, 0.16, 0.3, 0.5])))
    elif k == 3:
        call("SetRXASSQLTauMute", float(rng.choice([0.0, 0.01, 0.1]))); call("SetRXASSQLTauUnMute", float(rng.choice([0.0, 0.01, 0.1])))
    elif k == 4:
        call("SetRXASPCWRun", int(rng.integers(0, 2)))
    elif k == 5:
        call("SetRXASPCWFreq", float(rng.uniform(400, 1500))); call("SetRXASPCWBandwidth", float(rng.uniform(30, 200)))
    elif k == 6:
        call("SetRXASPCWGain", float(rng.uniform(0.5, 3.0)))
    elif k == 7:
        call("SetRXAmpeakRun", int(rng.integers(0, 2)))
    elif k == 8:
        call("SetRXAmpeakNpeaks", int(rng.integers(1, 3))); call("SetRXAmpeakFilEnable", int(rng.integers(0, 2)), int(rng.integers(0, 2)))
    elif k == 9:
        fil = int(rng.integers(0, 2))
        call("SetRXAmpeakFilFreq", fil, float(rng.uniform(500, 2500))); call("SetRXAmpeakFilBw", fil, float(rng.uniform(40, 150)))
    elif k == 10:
        call("SetRXAmpeakFilGain", int(rng.integers(0, 2)), float(rng.uniform(0.5, 2.5)))
    elif k == 11:
        call("SetRXACBLRun", int(rng.integers(0, 2)))
    elif k == 12:
        call("SetRXASNBARun", int(rng.integers(0, 2)))
    elif k == 13:
        call("SetRXAFMLimRun", int(rng.integers(0, 2))); call("SetRXAFMLimGain", float(rng.uniform(0.0, 20.0)))
    elif k == 14:
        call("SetRXACTCSSFreq", float(rng.choice([67.0, 100.0, 151.4, 250.3]))); call("SetRXACTCSSRun", int(rng.integers(0, 2)))
    else:
        call("SetRXAFMDeviation", float(rng.choice([2500.0, 5000.0])))
    return done


class _Split:
    """a channel's stage setters go to its restatement, every other setter to its stage-off engine and its oracle channel"""

    def __init__(self, stage_off, oracle_channel, ap, sq):
        self.others, self.ap, self.sq = (stage_off, oracle_channel), ap, sq

    def __getattr__(self, name):
        def call(*args):
            if name.startswith("SetRXASSQL"):
                getattr(self.sq, name)(*args)
            elif name.startswith(STAGE_PREFIXES):
                getattr(self.ap, name)(*args)
            else:
                for t, lead in self.others:
                    getattr(t, name)(*lead, *args)
        return call


@pytest.mark.parametrize("seed", list(range(701, 713)))
def test_seeded_walk_over_the_newer_setters_with_graph_replay(qh, oracle, seed):
    rng = np.random.default_rng(seed)
    gaps = [6] + [int(rng.choice(GAPS)) for _ in range(26)]
    nblk = sum(gaps)
    modes = [USB, AM, CWU, USB]
    pbs = [(300.0, 3000.0), (-4000.0, 4000.0), (300.0, 3000.0), (-8000.0, 8000.0)]
    x = synth.make_input_numpy(NCH, nblk * 1024)
    x[1] = synth.make_mode_input_numpy("am", 1, nblk * 1024)
    x[3] = synth.make_mode_input_numpy("fm", 3, nblk * 1024)
    a, p, b = qh.RxaEngine(NCH), qh.RxaEngine(NCH), qh.RxaEngine(NCH)       # replayed, its plain twin, the stage-off engine
    os_ = [oracle.WdspChannel(1024, 256, 192000, 48000, 48000) for _ in range(NCH)]
    aps, sqs = [AudioPeakChain(48000.0) for _ in range(NCH)], [Ssql(48000) for _ in range(NCH)]
    try:
        for c in range(NCH):
            for t, lead in ((a, (c,)), (p, (c,)), (b, (c,)), (os_[c], ())):
                t.SetRXAShiftRun(*lead, 1); t.SetRXAShiftFreq(*lead, synth.shift_freq(c)); t.RXANBPSetRun(*lead, 1)
                t.SetRXAMode(*lead, modes[c]); t.RXASetPassband(*lead, *pbs[c])
            b.SetRXAPanelGain1(c, 1.0); os_[c].SetRXAPanelGain1(1.0)
        a.set_graph_replay(True)
        for e in (a, p, b):
            e.enable_meters(True)
        dev = torch.device("cuda:0")
        d_in = torch.zeros((NCH, 1024), dtype=torch.complex128, device=dev)
        d_out = torch.zeros((NCH, 256), dtype=torch.complex128, device=dev)
        ya, yp, want, yb, rs, log, snba_used = [], [], [], [], [[] for _ in range(NCH)], [], [False] * NCH
        k = 0
        for s, gap in enumerate(gaps):
            for _ in range(gap):
                blk = np.ascontiguousarray(x[:, k * 1024:(k + 1) * 1024])
                for e, ys in ((a, ya), (p, yp)):
                    d_in.copy_(torch.from_numpy(blk))
                    torch.cuda.synchronize()
                    e.process_ptr(d_in.data_ptr(), 1024, d_out.data_ptr(), 256, 1)
                    e.synchronize()
                    ys.append(d_out.cpu().numpy().copy())
                yb.append(b.process_host(blk))
                want.append(np.stack([panel(sqs[c].process(aps[c].process(yb[-1][c]))) for c in range(NCH)]))
                for c in range(NCH):
                    rs[c].append(os_[c].xrxa(blk[c]))
                assert np.array_equal(ya[-1], yp[-1]), "seed %d block %d differs from the plain twin; setters %r" % (seed, k, log)
                k += 1
            c = int(rng.integers(0, NCH))
            done = _apply3(rng, [(a, (c,)), (p, (c,)), (_Split((b, (c,)), (os_[c], ()), aps[c], sqs[c]), ())], fm=(c == 3))
            log.append((k, c, done))
            snba_used[c] = snba_used[c] or any(d[0] == "SetRXASNBARun" and d[1] for d in done)
        assert a.graph_launches() > nblk // 3 and p.graph_launches() == 0
        assert _meters(a, NCH) == _meters(p, NCH)
        ya, want, yb = np.concatenate(ya, axis=1), np.concatenate(want, axis=1), np.concatenate(yb, axis=1)
        for c in range(NCH):
            ref = np.concatenate(rs[c])
            assert np.all(np.isfinite(ref)) and np.all(np.isfinite(ya[c]))
            err, err_b = rel_rms(ya[c], want[c]), rel_rms(yb[c], ref)
            print("seed %d channel %d: against the restatement %.3e, the stage-off engine against the oracle %.3e" % (seed, c, err, err_b), flush=True)
            assert err < 1e-9, (seed, c, err, [l for l in log if l[1] == c])
            assert err_b < (1e-5 if snba_used[c] else 1e-6), (seed, c, err_b, [l for l in log if l[1] == c])
    finally:
        for e in (a, p, b):
            e.close()
