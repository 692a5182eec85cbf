"""The inputs of test_gpu_snba_rates.py and test_gpu_snba_rates_engine.py, vetted on the CPU: the reference must be well conditioned on
each of them, or a comparison against it at 1e-6 says nothing.

xsnba's detector compares against thresholds and its repair inverts a Toeplitz matrix, so the reference itself can turn a last-bit
change of its input into another set of repaired samples (one flipped decision: some 1e-2 relative RMS).  The condition: for each input,
the oracle run on x * (1 + 1e-12 * noise), for eight noise seeds, stays within 1e-7 relative RMS of the oracle on x -- one decade under
the GPU tests' gate, at a perturbation ten times what the engine and the oracle differ by ahead of the blanker.  An input that does
not meet it is replaced by another channel number of `crackle` in snba_rate_cases.py (the AM channel at 192 k / 512 measured 8.9e-7,
which is why that case has none); the gate is not loosened and no samples are excluded.  Not a GPU test."""
import numpy as np
import pytest

from conftest import rel_rms
from snba_rate_cases import AFTER_RATE_CHANGE, CASES, NAMES_CASE, SETTER_CASE, SETTER_EVENTS

SEEDS, EPS, BOUND = 8, 1e-12, 1e-7
INPUTS = dict({name: (c, None) for name, c in CASES.items()},
              **{"setter_" + name: (SETTER_CASE, ev) for name, ev in SETTER_EVENTS.items()},
              after_rate_change=(AFTER_RATE_CHANGE, None), wdsp_names=(NAMES_CASE, None))


@pytest.mark.parametrize("name", sorted(INPUTS))
def test_the_reference_is_well_conditioned_on(oracle, name):
    c, events = INPUTS[name]
    x = c.inputs()
    ref = c.reference(oracle, x, events)
    assert np.all(np.isfinite(ref))
    worst = np.zeros(c.nch)
    for seed in range(SEEDS):
        noise = np.random.default_rng(5000 + seed).standard_normal(x.shape)
        moved = c.reference(oracle, x * (1.0 + EPS * noise), events)
        worst = np.maximum(worst, [rel_rms(moved[ch], ref[ch]) for ch in range(c.nch)])
    print("%s %s: the oracle against itself, worst of %d seeds per channel: %s" % (name, c.rates, SEEDS, ", ".join("%.1e" % w for w in worst)))
    assert worst.max() < BOUND, worst
