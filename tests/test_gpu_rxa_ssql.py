"""xssql in the batched RXA engine (RXA.c:594) against the restatement (tests/rxa_ssql_ref.py).

Engine A runs the squelch; engine B has the same settings without it and an identity panel, so B's output is the squelch's input (the
mode-0 fixed gain included: a channel with the squelch takes it ahead of it).  The restatement runs on B's output and the default
panel (gain1 4) follows; SSQL's gain is a real scalar on I and Q, so it commutes with the panel.  The inputs are "syllabic": a tone
hopping between about 400 and 1800 Hz every 60-150 ms, on for 1 s and off for 1.5 s in turn, so every case opens and closes the squelch at
least twice.  Samples the restatement mutes are exactly 0; the rest is held to 1e-9 relative RMS, the chain's own bound.  -m gpu."""
import numpy as np
import pytest

from conftest import rel_rms
from quisk_amd import synth
from rxa_audio_peak_ref import panel
from rxa_ssql_ref import DECREASE, INCREASE, Ssql, edges, syllabic

pytestmark = pytest.mark.gpu

FS = 192000
TOL = 1e-9
# ragged calls (blocks of 1024 input samples): a run of short calls through one gate cycle, so ramps straddle call boundaries, and
# one long call of many tiles
CALLS = (3, 1, 17) + (7,) * 54 + (800, 500, 5, 2)


def _engine(qh, nch, modes, dsp_rate=48000):
    e = qh.RxaEngine(nch, dsp_rate=dsp_rate, out_rate=dsp_rate)
    for c in range(nch):
        e.SetRXAShiftRun(c, 1); e.SetRXAShiftFreq(c, synth.shift_freq(c)); e.RXANBPSetRun(c, 1)
        e.SetRXAMode(c, modes[c])
        pb = (-8000.0, 8000.0) if modes[c] == 5 else (-4000.0, 4000.0) if modes[c] in (6, 10) else \
            (-3000.0, -300.0) if modes[c] in (0, 3, 9) else (300.0, 3000.0)
        e.RXASetPassband(c, *pb)
    return e


def _input(modes, n, seed0=0):
    t = np.arange(n) / FS
    x = np.empty((len(modes), n), dtype=np.complex128)
    for c, m in enumerate(modes):
        z = syllabic(n, FS, seed=seed0 + c)
        car = np.exp(-2j * np.pi * ((synth.shift_freq(c) * t) % 1.0))
        if m == 6:                                         # AM: the tone on a carrier
            x[c] = (0.1 + 0.05 * z.real) * car
        elif m == 5:                                       # FM: the tone as +-3 kHz deviation
            x[c] = 0.1 * np.exp(1j * 2 * np.pi * np.cumsum(3000.0 * z.real / 0.3) / FS) * car
        else:
            x[c] = 0.3 * (np.conj(z) if m in (0, 3, 9) else z) * car
    return x


class _Both:
    def __init__(self, e, refs):
        self.e, self.refs = e, refs

    def __getattr__(self, name):
        def call(c, *a):
            getattr(self.e, name)(c, *a)
            getattr(self.refs[c], name)(*a)
        return call


def _run(qh, modes, on, calls=CALLS, dsp_rate=48000, between=None, prep=None):
    """(A's output, the restated output, the restated gain, B's output, [ref state at each call's end]) over the calls"""
    nch = len(modes)
    a, b = _engine(qh, nch, modes, dsp_rate), _engine(qh, nch, modes, dsp_rate)
    if prep:
        prep(a); prep(b)
    b.SetRXAPanelGain1(-1, 1.0)
    refs = [Ssql(dsp_rate) for _ in range(nch)]
    both = _Both(a, refs)
    for c in on:
        both.SetRXASSQLRun(c, 1)
    x = _input(modes, sum(calls) * a.dsp_insize)
    ya, yr, gr, yb, ends = [], [], [], [], []
    pos = 0
    try:
        for k, nb in enumerate(calls):
            if between:
                between(k, a, b, both, refs)
            xa = np.ascontiguousarray(x[:, pos:pos + nb * a.dsp_insize])
            pa, pb = a.process_host(xa), b.process_host(xa)
            ya.append(pa); yb.append(pb)
            out, g = [], []
            for c in range(nch):
                out.append(panel(refs[c].process(pb[c])))
                g.append(refs[c].gain)
            yr.append(np.stack(out)); gr.append(np.stack(g))
            ends.append([r.state for r in refs])
            pos += nb * a.dsp_insize
    finally:
        a.close(); b.close()
    return np.concatenate(ya, 1), np.concatenate(yr, 1), np.concatenate(gr, 1), np.concatenate(yb, 1), ends


def _check(ya, yr, gr, chans, min_edges=2):
    for c in chans:
        op, cl = edges(gr[c])
        assert op >= min_edges and cl >= min_edges, (c, op, cl)
        muted = gr[c] == 0.0
        assert not np.any(ya[c][muted]), (c, int(np.sum(ya[c][muted] != 0)), np.flatnonzero(ya[c][muted] != 0)[:5])
        r = rel_rms(ya[c], yr[c])
        assert r < TOL, (c, r)


def test_every_mode_48k_ragged(qh):
    modes = [1, 0, 4, 6, 5]                                # USB, LSB, CWU, AM, FM
    ya, yr, gr, _, ends = _run(qh, modes, range(5))
    _check(ya, yr, gr, range(5))
    assert any(s in (INCREASE, DECREASE) for row in ends[:-1] for s in row)     # a ramp straddles a call boundary


def test_96k(qh):
    modes = [1, 0, 6]
    calls = (5, 2) + (9,) * 60 + (1500, 3)
    ya, yr, gr, _, ends = _run(qh, modes, range(3), calls=calls, dsp_rate=96000)
    _check(ya, yr, gr, range(3))
    assert any(s in (INCREASE, DECREASE) for row in ends[:-1] for s in row)


def test_setters_run_toggle_and_flush(qh):
    """threshold and taus between calls; run 1 -> 0 -> 1 with the state frozen while off; qh_rxa_flush's partial reset mid-stream"""
    modes = [1, 1, 1, 0]

    def between(k, a, b, s, refs):
        if k == 10:
            s.SetRXASSQLThreshold(0, 0.2); s.SetRXASSQLTauMute(1, 0.3); s.SetRXASSQLTauUnMute(1, 0.05)
            s.SetRXASSQLRun(2, 0)
        elif k == 30:
            s.SetRXASSQLRun(2, 1); s.SetRXASSQLTauUnMute(3, 0.0)
        elif k == 45:
            a.flush(); b.flush()
            for r in refs:
                r.flush()

    ya, yr, gr, yb, _ = _run(qh, modes, range(4), between=between)
    _check(ya, yr, gr, range(4))
    starts = np.cumsum((0,) + CALLS) * 256
    assert np.array_equal(ya[2, starts[10]:starts[30]], panel(yb[2, starts[10]:starts[30]]))    # run 0: as is


def test_with_agc_modes_audio_peak_and_amsq(qh):
    """AGC mode 0 (fixed gain ahead of the squelch) and mode 3; the carrier block and the multi-peak filter ahead of it; AMSQ behind
    the panel"""
    modes = [1, 1, 4, 6]

    def prep(e):
        e.SetRXAAGCMode(0, 0); e.SetRXAAGCFixed(0, 66.0)
        e.SetRXAAGCMode(1, 3)
        e.SetRXACBLRun(2, 1); e.SetRXAmpeakRun(2, 1); e.SetRXAmpeakRun(1, 1)

    def between(k, a, b, s, refs):
        if k == 0:
            a.SetRXAAMSQRun(3, 1)                           # on A only: B's output stays the squelch's input

    ya, yr, gr, _, _ = _run(qh, modes, range(4), prep=prep, between=between, calls=CALLS[:-3] + (200, 5, 2))
    _check(ya, yr, gr, range(3))
    muted = gr[3] == 0.0                                    # AMSQ acts on the squelched output: its muted samples stay 0
    assert np.any(muted) and not np.any(ya[3][muted]) and np.all(np.isfinite(ya[3]))


def test_victim_channel_isolation(qh):
    """SSQL settings of one channel move no other channel's output, bit for bit"""
    modes = [1, 0, 1]
    x = _input(modes, 40 * 1024)
    outs = []
    for k in range(2):
        e = _engine(qh, 3, modes)
        try:
            if k:
                e.SetRXASSQLRun(1, 1); e.SetRXASSQLThreshold(1, 0.3); e.SetRXASSQLTauMute(1, 0.2)
            outs.append(np.concatenate([e.process_host(np.ascontiguousarray(x[:, i * 4096:(i + 1) * 4096])) for i in range(10)], 1))
        finally:
            e.close()
    assert np.array_equal(outs[0][0], outs[1][0]) and np.array_equal(outs[0][2], outs[1][2])
    assert not np.array_equal(outs[0][1], outs[1][1])


def test_graph_replay_matches_eager(qh):
    import torch
    dev = torch.device("cuda:0")
    nch, nblk, ncall = 3, 24, 40
    modes = [1, 0, 6]
    x = _input(modes, ncall * nblk * 1024)
    res = []
    for replay in (False, True):
        e = _engine(qh, nch, modes)
        e.SetRXASSQLRun(-1, 1)
        e.set_graph_replay(replay)
        d_in = torch.zeros((nch, nblk * 1024), dtype=torch.complex128, device=dev)
        d_out = torch.zeros((nch, nblk * 256), dtype=torch.complex128, device=dev)
        ys = []
        try:
            for k in range(ncall):
                if k == 20:
                    e.SetRXASSQLThreshold(1, 0.12); e.SetRXASSQLTauMute(2, 0.15)
                d_in.copy_(torch.from_numpy(np.ascontiguousarray(x[:, k * nblk * 1024:(k + 1) * nblk * 1024])))
                e.process_ptr(d_in.data_ptr(), nblk * 1024, d_out.data_ptr(), nblk * 256, nblk)
                torch.cuda.synchronize()
                ys.append(d_out.cpu().numpy())
            if replay:
                assert e.graph_launches() > 0
        finally:
            e.close()
        res.append(np.concatenate(ys, 1))
    assert np.array_equal(res[0], res[1])
    assert np.any(res[0] == 0) and np.any(res[0] != 0)


def test_untouched_engine_is_bit_identical(qh):
    """SetRXASSQLRun(c, 0) and the other three setters on one engine, none on the other: same bits and device bytes"""
    nch = 3
    modes = [1] * nch
    a, b = _engine(qh, nch, modes), _engine(qh, nch, modes)
    a.SetRXASSQLRun(-1, 0); a.SetRXASSQLThreshold(1, 0.3); a.SetRXASSQLTauMute(-1, 0.2); a.SetRXASSQLTauUnMute(0, 0.05)
    x = synth.make_input_numpy(nch, 10 * 4096)
    try:
        for k in range(10):
            xa = np.ascontiguousarray(x[:, k * 4096:(k + 1) * 4096])
            assert np.array_equal(a.process_host(xa), b.process_host(xa)), k
        assert a.device_bytes() == b.device_bytes()
    finally:
        a.close(); b.close()


def test_refused_values_change_nothing(qh):
    modes = [1, 1]
    a, b = _engine(qh, 2, modes), _engine(qh, 2, modes)
    lib = qh.load()
    for e in (a, b):
        e.SetRXASSQLRun(-1, 1)
    nan, inf = float("nan"), float("inf")
    for bad in (lambda: lib.qh_rxa_SetRXASSQLTauMute(a._h, 0, -0.1), lambda: lib.qh_rxa_SetRXASSQLTauMute(a._h, -1, nan),
                lambda: lib.qh_rxa_SetRXASSQLTauUnMute(a._h, 1, inf), lambda: lib.qh_rxa_SetRXASSQLTauUnMute(a._h, -1, -1e-9),
                lambda: lib.qh_rxa_SetRXASSQLThreshold(a._h, 0, nan), lambda: lib.qh_rxa_SetRXASSQLThreshold(a._h, -1, -inf)):
        assert bad() == -2                                      # QH_ERR_INVALID
    assert lib.qh_rxa_SetRXASSQLTauMute(a._h, 0, 0.0) == 0 and lib.qh_rxa_SetRXASSQLTauMute(b._h, 0, 0.0) == 0
    x = _input(modes, 60 * 4096)
    try:
        for k in range(60):
            xa = np.ascontiguousarray(x[:, k * 4096:(k + 1) * 4096])
            assert np.array_equal(a.process_host(xa), b.process_host(xa)), k
    finally:
        a.close(); b.close()
