"""The reference of tests/test_gpu_rxa_linear_forms.py checked on the CPU: the fast long-double form against direct long-double sums,
against the oracle, its bound against the project's stream tolerance, and planted faults that a relative RMS passes and the
per-sample bound catches.  Needs no GPU.

Measured here over the six configurations of rxa_linear_ref.REFERENCE_CASES (with retunes and SetRXAShiftRun toggles between the
calls) and the blocker case: the fast form is within 1.1e-18 to 3.4e-18 rms(want) of the direct sums; oracle.WdspChannel.xrxa is
7e-13 to 5.1e-12 rms(want) from the long-double form at its worst sample (its oscillator is WDSP's recurrence in doubles); the float64
overlap-save model is 1.0e-15 to 2.1e-15 rms(want) from it, 3.7e-15 with the blocker, so that 16 E is 0.016 to 0.034 of the stream
tolerance TOL64 rms(want)."""
import numpy as np
import pytest

import rxa_linear_ref as R
from conftest import rel_rms

CASES = R.REFERENCE_CASES + [R.BLOCKER_CASE]
IDS = [cs.name.replace(" ", "_") for cs in CASES]


def test_long_double_and_the_oscillator_contract():
    R.require_long_double()
    assert R.nco_step(12000.0, 48000) == 2 ** 62 and R.nco_step(-12000.0, 48000) == 3 * 2 ** 62 and R.nco_step(0.0, 192000) == 0
    assert R.nco_step(48000.0 + 12000.0, 48000) == 2 ** 62                     # whole turns drop out
    assert R.nco_step(1.0, 3) == (2 ** 64 - 1) // 3                             # the floor, not the nearest
    assert R.nco_step(-0.0, 48000) == 0 and 0 <= R.nco_step(-1e-300, 48000) < 2 ** 64
    r = R.rotation(np.array([0, 2 ** 62, 2 ** 63, 3 * 2 ** 62, 2 ** 61], dtype=np.uint64))
    want = np.array([1, 1j, -1, -1j, np.sqrt(np.longdouble(0.5)) * (1 + 1j)], dtype=R.CLD)
    assert np.max(np.abs(r - want)) < 2e-19
    cs = R.REFERENCE_CASES[0]
    phase, run = R.nco_phase(cs, 1)
    per_in, blocks, laws = cs.dsp_size * cs.in_rate // cs.dsp_rate, R.call_blocks(cs), R.laws(cs, 1)
    assert blocks == (1, 1, 2, 3, 15, 16, 17, 9, 1) and phase.size == sum(blocks) * per_in
    assert {r for r, _ in laws} == {0, 1} and len({f for _, f in laws}) == 5
    pos, p = 0, 0
    for nb, (r, f) in zip(blocks, laws):                                        # the phase: Python integers, call by call
        assert int(phase[pos]) == p and bool(run[pos]) == bool(r)
        d = R.nco_step(f, cs.in_rate) if r else 0
        assert int(phase[pos + nb * per_in - 1]) == (p + d * (nb * per_in - 1)) % 2 ** 64
        p, pos = (p + d * nb * per_in) % 2 ** 64, pos + nb * per_in


@pytest.mark.parametrize("cs", CASES, ids=IDS)
def test_fast_form_against_direct_long_double_sums(cs):
    """Three windows of 80 outputs: the stream's start, across the call behind the first retune, the stream's end."""
    rec = R.case_ref(cs, 1)
    want, n = rec["want"][0], rec["want"].shape[1]
    worst = 0.0
    for lo in (0, int(rec["retunes"][0]) - 40, n - 80):
        direct = R.chain_direct(cs, 0, rec["x"][0], lo, lo + 80)
        worst = max(worst, float(np.max(np.abs(direct - want[lo:lo + 80]))))
    print("fast form against direct sums: %.3g of rms" % (worst / rec["rms"][0]))
    assert worst <= 1e-17 * rec["rms"][0]


@pytest.mark.parametrize("cs", CASES, ids=IDS)
def test_against_the_oracle_per_sample(oracle, cs):
    """A mistake in the composition (a stage's order, a phase, a gain, the resampler's first phase, a retune's moment) is of order
    one; the oracle's own distance from the long-double form is 7e-13 to 5.1e-12 of rms(want) at its worst sample."""
    rec = R.case_ref(cs, 1)
    got = R.run_oracle(oracle, cs, 0)
    assert got.shape == rec["want"][0].shape
    w = R.assert_inside("oracle, " + cs.name, got[None], rec["want"], 1e-9 * rec["rms"][0], (), rec["calls"])
    print("oracle against the long-double form: %.3g of rms, %s outputs from a call's start" % (w["err"] / rec["rms"][0], w["to_call"]))


@pytest.mark.parametrize("cs", R.REFERENCE_CASES, ids=IDS[:-1])
def test_the_new_bound_is_the_tighter_one(cs):
    rec = R.case_ref(cs, 1)
    assert 0.0 < R.MARGIN * rec["E"][0] < R.TOL64 * rec["rms"][0]
    assert float(np.max(rec["bound"].real)) < R.TOL64 * rec["rms"][0]          # the oscillator's term included


def _caught(name, got, rec, tiles=()):
    assert rel_rms(got, rec["want"]) < 1e-9, "the planted fault is meant to pass the stream gate"
    with pytest.raises(AssertionError, match="over bound"):
        R.assert_inside(name, got, rec["want"], rec["bound"], tiles, rec["calls"])


def test_planted_one_sample_at_every_tile_start():
    cs = R.REFERENCE_CASES[0]
    rec = R.case_ref(cs, 1)
    tiles = rec["tiles"]
    assert 20 < tiles.size < 200
    got = rec["want"].astype(np.complex128)
    R.assert_inside("the reference rounded to doubles", got, rec["want"], rec["bound"])
    got[0, tiles] += 1e-10 * rec["rms"][0]
    _caught("tile starts", got, rec, tiles)


def test_planted_phase_law_one_input_sample_late_behind_a_retune():
    """A retune by 20 microhertz whose new step takes hold one input sample late: from there on the phase is off by the two steps'
    difference, 6.5e-10 rad."""
    cs = R.case("192k usb 2048 fine retune", kind="clean", schedule="fine")
    rec = R.case_ref(cs, 1)
    phase, run = R.nco_phase(cs, 0)
    n0 = sum(rec["sizes"][:4])
    d_old, d_new = (R.nco_step(R.freq_value(0, v), cs.in_rate) for v in (0, 2e-5))
    assert d_old != d_new and int(phase[n0 + 1]) == (int(phase[n0]) + d_new) % 2 ** 64
    late = phase.copy()
    late[n0 + 1:] += np.uint64((d_old - d_new) % 2 ** 64)
    got = R.chain_ld(cs, 0, rec["x"][0], phase=late).astype(np.complex128)[None]
    _caught("late phase law", got, rec)


def test_planted_delay_line_one_sample_short_at_a_call_boundary():
    """nbp0's delay line (nc 8192) handed to the last call without its oldest sample: the last tap's product is missing from that
    call's outputs.  Over nc - 1 outputs of a call in mid-stream the same fault comes to 2e-9 to 7e-9 of the stream's RMS, the size of
    the stream gate itself, which then sees it or not by the call's length; behind the last call's 256 outputs it leaves 6e-10."""
    cs = R.case("192k usb 8192", nc=8192, kind="clean")
    rec = R.case_ref(cs, 1)
    keep = []
    R.chain_ld(cs, 0, rec["x"][0], keep=keep)
    mid, (h, _, _, _) = keep[1], R.stages(cs, 0)[1]
    m0, nc, n = int(rec["calls"][-1]), h.size, rec["want"].shape[1]
    assert nc == 8192 and m0 >= nc and 0 < n - m0 < nc
    lost = h[nc - 1] * mid[m0 - (nc - 1):n - (nc - 1)]      # output m misses h[nc - 1] mid[m - (nc - 1)], m0 <= m < n
    got = rec["want"].copy()
    got[0, m0:] -= R.panel(lost, cs.agc_db)
    _caught("short delay line", got.astype(np.complex128), rec)
