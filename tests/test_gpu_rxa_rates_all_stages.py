"""A new dsp_size or dsp_rate with every optional stage in the chain: an engine that has run, rested in silence and then taken the change
against an engine made at the new values with the same setter list.  -m gpu.

test_gpu_rxa_rates.py holds Engine::rebuild to the oracle with the default stages.  A rebuild keeps every setting and drops every note of
pending work (dirty and flush flags, what is on the device): a note that is kept, or a setting that is dropped, shows only on the stage it
belongs to.  So here the stages of test_every_stage_a_mode_allows_at_once (test_gpu_rxa_stage_combinations.py: its setters, values and
signal) are all on, in one engine of three channels at in = dsp = out = 48000, dsp_size 64, default nc:

  USB   fixed AGC gain applied at the AGC's spot (fix_before), EQP (10 bands), CBL + SPCW, SSQL, ANF at position 1, the sender
  AM    fade leveller off (test_gpu_rxa_rates.py says why), AGC mode 1 with hang, AMSQ, EQP (profile), mpeak, SSQL, the sender
  FM    FMSQ, EQP (4 bands), SSQL, EMNR at position 0, the sender

gen0 is off: its phase is carried by design (test_a_new_dsp_size_leaves_gen0_s_phase_running).

Engine A: the setters, two calls of signal (1 and 3 kibisamples), silence as long as test_gpu_rxa_rates.py's after-silence cases use (48
blocks before a new dsp_size, 0.6 s before a new dsp_rate), the change, four calls of signal (1, 3, 9, 1 kibisamples).  Engine B: made at
the new values, the same setters, the same four calls.  Both are this library, so no reference's margins come in: equal state gives equal
bits.  Compared per channel: the output by relative RMS under the gates of test_gpu_rxa_stage_combinations.py, 1e-6, and 1e-4 on the
channel where ANF runs; the sender's rows of the last call likewise (float32 rows: bit-equal or 1e-6).  Device memory: A holds what B holds.

Measured on the MI355X, relative RMS A against B per channel (USB, AM, FM), output | sender rows:
  before this file's refactor   dsp_size 64 -> 128     0 0 0 | 0 0 0
                                dsp_rate 48 k -> 96 k  0 0 2.93e-13 | 0 0 0
  with it                       dsp_size 64 -> 128     0 0 0 | 0 0 0
                                dsp_rate 48 k -> 96 k  0 0 2.93e-13 | 0 0 0
"""
import numpy as np
import pytest

from conftest import rel_rms
from test_gpu_rxa_stage_combinations import AM, CALLS, FM, USB, _base, _input, _neighbour, _stage, case_setup

pytestmark = pytest.mark.gpu

RATE, SIZE = 48000, 64
MODES, STAGES = case_setup("all", ())
NEIGHBOURS = (("anf1",), ("agc1_hang", "amsq"), ("emnr0",))
BEFORE, AFTER = CALLS[:2], CALLS[:4]


def engine(qh, dsp_rate, size):
    e = qh.RxaEngine(3, dsp_size=size, in_rate=RATE, dsp_rate=dsp_rate, out_rate=RATE)
    e.load_emnr_tables()
    for c, m in enumerate(MODES):
        _base(e, c, m)                      # (an FM channel's settings with USB for its mode ...)
        for nb in NEIGHBOURS[c]:
            _neighbour(e, c, m, nb)
        for s in STAGES[c]:
            if s != "fmsq":
                _stage(e, c, m, s)
        if m == FM:                         # (... the engine refuses an FM squelch without its detector)
            e.SetRXAMode(c, FM)
            _stage(e, c, m, "fmsq")
        if m == AM:
            e.SetRXAAMDFadeLevel(c, 0)
        e.SetRXAPreGenRun(c, 0)
    e.set_sender(-1, True)
    return e


def run(e, x, calls):
    """x in calls of so many kibisamples; the output and the last call's sender rows"""
    out, pos = [], 0
    for k in calls:
        out.append(e.process_host(np.ascontiguousarray(x[:, pos:pos + 1024 * k])))
        pos += 1024 * k
    assert pos == x.shape[1]
    return np.concatenate(out, axis=1), np.stack([e.sender_rows_host(c) for c in range(3)])


def measure(qh, change, dsp_rate, size, nsilent):
    """per channel: relative RMS of A against B, output and sender rows; A's and B's device bytes"""
    x1, x2 = _input(MODES, 1024 * sum(BEFORE), RATE), _input(MODES, 1024 * sum(AFTER), RATE)
    a = engine(qh, RATE, SIZE)
    try:
        run(a, x1, BEFORE)
        a.process_host(np.zeros((3, nsilent * SIZE), dtype=np.complex128))
        change(a)
        assert (a.in_rate, a.dsp_rate, a.out_rate, a.dsp_size) == (RATE, dsp_rate, RATE, size)
        ya, sa = run(a, x2, AFTER)
        bytes_a = a.device_bytes()
    finally:
        a.close()
    b = engine(qh, dsp_rate, size)
    try:
        yb, sb = run(b, x2, AFTER)
        bytes_b = b.device_bytes()
    finally:
        b.close()
    assert np.all(np.isfinite(yb)) and sa.shape == sb.shape and sb.shape[1] > 0
    for c in range(3):                      # the case is not an empty one: every channel puts something out, every sender row holds signal
        assert np.abs(yb[c]).max() > 1e-6 and np.abs(sb[c]).max() > 1e-6, (c, np.abs(yb[c]).max(), np.abs(sb[c]).max())
    return [rel_rms(ya[c], yb[c]) for c in range(3)], [rel_rms(sa[c], sb[c]) for c in range(3)], bytes_a, bytes_b


@pytest.mark.parametrize("what", ["dsp_size", "dsp_rate"])
def test_a_change_after_silence_equals_a_fresh_engine_with_every_stage_on(qh, what):
    if what == "dsp_size":
        out, snd, bytes_a, bytes_b = measure(qh, lambda e: e.set_dsp_size(128), RATE, 128, 48)
    else:
        out, snd, bytes_a, bytes_b = measure(qh, lambda e: e.set_dsp_rate(96000), 96000, SIZE, int(0.6 * RATE) // SIZE)
    print("%s: relative RMS A against B, output %s | sender rows %s; device bytes %d / %d"
          % (what, " ".join("%.2e" % v for v in out), " ".join("%.2e" % v for v in snd), bytes_a, bytes_b))
    for c in range(3):
        tol = 1e-4 if any(n.startswith(("anf", "anr")) for n in NEIGHBOURS[c]) else 1e-6
        assert out[c] < tol, (what, c, out)
        assert snd[c] < 1e-6, (what, c, snd)
    assert bytes_a == bytes_b
