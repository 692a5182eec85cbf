"""xsnba at DSP rates of 96, 192 and 384 kHz (ratios 8, 16, 32 to the blanker's 12 kHz internal rate) and at blocks of 2048 and 4096
samples -- the three-pass form of qh_snba.hpp -- against the restatement (oracle/snba_oracle.c in oracle/wdsp_oracle.c's chain), with
two setters in mid-stream.  Inputs and cases: snba_rate_cases.py (vetted on the CPU by test_snba_rate_inputs.py).  The gate is the
project's 1e-6 relative RMS in fp64; every case also shows that the reference with the blanker differs from the same channel
without it, so frames do get repaired.  -m gpu."""
import numpy as np
import pytest

from conftest import rel_rms
from snba_rate_cases import CASES, FM, SAM, SETTER_CASE, SETTER_EVENTS

pytestmark = pytest.mark.gpu

GATE = 1e-6


def _compare(c, y, ref, plain):
    errs = []
    for ch in range(c.nch):
        assert np.all(np.isfinite(ref[ch]))
        # SAM / FM: the loops' lock-in at the start of the stream amplifies last-bit differences (test_gpu_snba_parity.py)
        skip = 64 * 256 if c.modes[ch] in (SAM, FM) else 0
        errs.append(rel_rms(y[ch, skip:], ref[ch, skip:]))
        repaired = rel_rms(ref[ch], plain[ch])
        print("%s channel %d mode %d: rel RMS %.3e (the reference with SNB against without: %.3e)" % (c.rates, ch, c.modes[ch], errs[-1], repaired))
        assert repaired > 1e-3, (ch, repaired)
    assert max(errs) < GATE, errs


@pytest.mark.parametrize("name", sorted(CASES))
def test_snba_matches_the_oracle_at(qh, oracle, name):
    c = CASES[name]
    x = c.inputs()
    e = c.engine(qh)
    y = c.through(e, x)
    e.close()
    assert y.shape == (c.nch, c.nblk * c.outsize)
    _compare(c, y, c.reference(oracle, x), c.reference(oracle, x, snba=0))


@pytest.mark.parametrize("what", sorted(SETTER_EVENTS))
def test_snba_setters_in_mid_stream_at_192k(qh, oracle, what):
    """bandwidth: SetRXASNBAOutputBandwidth on one of two channels (its interpolation taps are designed again and its 140-sample history
    cleared, the other channel's stay); off_on: SetRXASNBARun 0 and 1 again (the state rests while the channel is off the list)"""
    c, ev = SETTER_CASE, SETTER_EVENTS[what]
    x = c.inputs()
    e = c.engine(qh)
    y = c.through(e, x, ev)
    e.close()
    _compare(c, y, c.reference(oracle, x, ev), c.reference(oracle, x, ev if what == "bandwidth" else None, snba=0))
