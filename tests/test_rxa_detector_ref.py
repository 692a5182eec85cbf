"""The reference of tests/test_gpu_rxa_detector_forms.py checked on the CPU: every chain of tests/rxa_detector_ref.py against the oracle
per sample, the two conditions that make a per-sample gate of the detectors possible, four planted faults that the suite's RMS gates
pass and the bound catches, and the all-zero stream.  Needs no GPU.

Measured here.  E is 1.0e-15 to 4.8e-14 rms(want) for USB, AM and SAM, 2.0e-15 with the CTCSS notch off and 2.9e-13 to 8.4e-13 with it
on for FM (the notch's poles at radius 0.9994 carry the rounding of 1 / 0.0006 samples), so 16 E is at most 1.4e-11 rms(want); T is
4.3e-12 rms(want) for FM, 3e-15 to 1e-14 for a locked SAM loop, 1.1e-10 to 1.8e-10 for SAM-L / SAM-U (the all-pass chains ring on a
tile's deviation) and 1.4e-10 to 2.0e-10 in the cold case, whose loop slips cycles at the tile boundary T is taken at.  With the oracle's oscillator parked and the input turned in long double ahead of it, oracle.WdspChannel is 0.04 to 0.10 of
16 E from the long-double chains at its worst sample, at the detector's own output (HOOK_FMSQ) and at xrxa's; with its own oscillator
(WDSP's recurrence in doubles, shift.c) it needs up to 6.6 times 16 E for the detectors and 413 times for the plain USB channel
(1.2e-11 rms(want), the figure tests/test_rxa_linear_ref.py reports for the linear chain), so that run is held to 1e-9 rms(want) as
there: it pins the composition, the parked one pins the arithmetic.

The planted faults, in the float64 model of FM channel 0 (AM channel 0 for the leveller), against the gates the suite had: relative
RMS against the reference behind 100 settle blocks (tests/test_gpu_tiled_detectors.py; 1e-6, from the first sample and 1e-8 for AM) and
a long call against block calls behind the same settle (1e-9).

    one FM tile started 1e-9 off in omega                               7.7e-14 behind the settle      23 times the bound
    the dc-removal carry at a tile seam without that tile's last sample 1.2e-10                        1.3e8
    the notch's state handed on one sample late at a tile seam          2.3e-10                        4.3e7
    the slow leveller average without the last sample of a call         6.0e-13 over the stream        98
"""
import numpy as np
import pytest

import rxa_detector_ref as D
from conftest import rel_rms

CASES = ([(ch, D.FM_SCHEDULE) for ch in D.FM3] + [(D.chan("fm", 1, ctcss_run=0), D.FM_SCHEDULE)]
         + [(D.chan("fm", 2, ctcss_freq=100.0, deviation=2500.0), D.FM_SCHEDULE)]
         + [(ch, D.AM_SCHEDULE) for ch in D.AM3] + [(D.chan("am", 1), D.AM_SCHEDULE)]
         + [(ch, D.SAM_SCHEDULE) for ch in D.SAM3 + D.SAM3_PLAIN] + [(ch, D.SAM_COLD_SCHEDULE) for ch in D.SAM3_COLD]
         + [(D.chan("usb", 0), D.FM_SCHEDULE)])


def case_id(case):
    ch, sched = case
    return "%s%d-lv%d-sb%d-dev%d-ctcss%d_%g-%dcalls" % (ch.kind, ch.idx, ch.levelfade, ch.sbmode, ch.deviation, ch.ctcss_run, ch.ctcss_freq,
                                                       len(sched))


def _parts(a, b):
    return float(max(np.max(np.abs(a.real - b.real)), np.max(np.abs(a.imag - b.imag))))


@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_the_two_conditions(case):
    """16 E <= 1e-10 rms(want) and 16 E + T <= 1e-9 rms(want): the caps are the issue's; a case that missed one would get another input."""
    ch, sched = case
    E, T, b = D.channel_bound(ch, sched)
    r = D.rms(D.channel_ref(ch)["want"][:b.size])
    print("E %.3g, 16 E %.3g, T %.3g of rms(want)" % (E / r, D.MARGIN * E / r, T / r))
    assert 0.0 < D.MARGIN * E <= 1e-10 * r
    assert D.MARGIN * E + T <= 1e-9 * r
    tiled = any(t for _, _, t in D.tiled_calls(ch.kind, sched))
    assert (T > 0.0) == tiled
    assert float(b.max()) == D.MARGIN * E + T and float(b[0]) == D.MARGIN * E + (T if D.tiled_calls(ch.kind, sched)[0][2] else 0.0)


@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_against_the_oracle_per_sample(oracle, case):
    ch, sched = case
    ref = D.channel_ref(ch)
    n = sum(sched) * D.DSP_SIZE
    want, det_w = ref["want"][:n], ref["det"][:n]
    r = D.rms(want)
    det, out = D.run_oracle(oracle, ch, sched, turned=True)
    assert det.shape == det_w.shape and out.shape == want.shape
    e_det, e_out = _parts(det, det_w), _parts(out, want)
    print("oscillator parked: %.3g of 16 E at the detector's output, %.3g at the chain's" % (e_det / (16 * ref["E_det"]), e_out / (16 * ref["E"])))
    assert e_det <= D.MARGIN * ref["E_det"] and e_out <= D.MARGIN * ref["E"]
    det, out = D.run_oracle(oracle, ch, sched)
    e_out = _parts(out, want)
    print("the oracle's own oscillator: %.3g of 16 E, %.3g of rms(want)" % (e_out / (16 * ref["E"]), e_out / r))
    assert e_out <= 1e-9 * r


FM0, AM0 = D.FM3[0], D.AM3[0]
SEAM = 9 * D.DSP_SIZE + D.FM_EXACT_TILES * D.FM_TILE            # the 5-block call's first tile that starts from a guess
FAULTS = [("omega", FM0, D.FM_SCHEDULE, SEAM), ("dc", FM0, D.FM_SCHEDULE, SEAM - 1), ("notch", FM0, D.FM_SCHEDULE, SEAM - 1),
          ("leveller", AM0, D.AM_SCHEDULE, 116 * D.DSP_SIZE - 1)]


@pytest.mark.parametrize("fault", FAULTS, ids=[f[0] for f in FAULTS])
def test_planted_fault_passes_the_rms_gates_and_fails_the_bound(fault):
    name, ch, sched, idx = fault
    rec = D.case_ref((ch,), sched)
    seams, calls = D.detector_seams((ch,), sched)
    assert idx + 1 in seams or idx in seams
    clean = D.channel_ref(ch)["model"][None]
    D.assert_inside("the model", clean, rec["want"], rec["bound"], seams, calls)
    got = D.detector(ch, False, (name, idx))[1][None]
    settle = 0 if ch.kind == "am" else 100 * D.DSP_SIZE
    old = rel_rms(got[0, settle:], rec["want"][0, settle:].astype(np.complex128))
    long_short = rel_rms(got[0, settle:], clean[0, settle:])
    print("%s: %.3g against the reference, %.3g against the model without the fault" % (name, old, long_short))
    assert old < (1e-8 if ch.kind == "am" else 1e-6) and long_short < 1e-9, "the planted fault is meant to pass the gates the suite had"
    with pytest.raises(AssertionError, match="over bound"):
        D.assert_inside(name, got, rec["want"], rec["bound"], seams, calls)


def test_seams_hold_tiles_segments_and_calls():
    seams, calls = D.detector_seams(D.FM3, D.FM_SCHEDULE)
    assert list(calls[:5]) == [0, 256, 512, 1280, 2304] and set(range(0, 117 * 256, 256)) <= set(seams)
    assert D.seg_groups(3, 66 * 256) == 2 and D.seg_groups(3, 20 * 256) == 1 and D.seg_groups(85, 256 * 256) == 3
    m0 = 30 * 256                                               # the 66-block call: 32 segments over 264 batches of 64
    assert m0 + 64 * (5 * 264 // 32) in seams
    seams, calls = D.detector_seams(D.SAM3, D.SAM_SCHEDULE)
    assert 43 * 256 + 4096 in seams and 4096 not in seams       # SAM tiles in the calls from 32768 samples on only
    assert D.guess_boundaries("sam", D.SAM_SCHEDULE) == (43 * 256 + 3 * 4096, 176 * 256 + 3 * 4096)
    assert D.guess_boundaries("fm", D.FM_SCHEDULE) == (9 * 256 + 1024, 14 * 256 + 1024, 30 * 256 + 1024, 97 * 256 + 1024)


@pytest.mark.parametrize("ch", [D.chan("fm"), D.chan("am"), D.chan("sam"), D.chan("sam", sbmode=1), D.chan("sam", sbmode=2)],
                         ids=["fm", "am", "sam", "sam-l", "sam-u"])
def test_an_all_zero_stream_gives_exactly_zero(ch):
    for T in (D.LD, np.float64):
        det, out = D.chain(ch, np.zeros(3 * D.DSP_SIZE, dtype=D.CLD if T is D.LD else np.complex128), T)
        assert not np.any(det.real) and not np.any(det.imag) and not np.any(out.real) and not np.any(out.imag)
