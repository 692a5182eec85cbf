"""xsender in the batched RXA engine (RXA.c:570): the float rows against np.float32 of the oracle's signal behind nbp0.

The reference is an oracle channel in USB mode with the channel's shift and passband on nbp0, captured at HOOK_FMSQ (rxa_taps_util.
oracle_channel).  The chain agrees with the oracle to the 1e-9 the stage tests use; two doubles that close narrow to floats at most one
ulp apart, and one ulp is at most 2^-23 of the sample: the rows are held to 2^-23 relative RMS.  -m gpu."""
import numpy as np
import pytest

from conftest import rel_rms
from rxa_taps_util import CALLS, MODES, capture, engine, oracle_channel, signal

pytestmark = pytest.mark.gpu
ULP = 2.0 ** -23
TOL = 1e-9


def _run(e, x, calls, chans):
    """(outputs, {ch: sender row}) over the calls"""
    ys, rows, pos = [], {c: [] for c in chans}, 0
    for nb in calls:
        n = nb * e.dsp_insize
        ys.append(e.process_host(np.ascontiguousarray(x[:, pos:pos + n])))
        for c in chans:
            r = e.sender_rows_host(c)
            assert r.size == nb * e.dsp_outsize
            rows[c].append(r)
        pos += n
    return np.concatenate(ys, 1), {c: np.concatenate(v) for c, v in rows.items()}


@pytest.fixture(scope="module")
def x5():
    return signal(MODES, sum(CALLS) * 1024)


@pytest.fixture(scope="module")
def nbp_refs(oracle, x5):
    """nbp0's output of the five channels, as np.complex64"""
    refs = []
    for c, m in enumerate(MODES):
        o = oracle_channel(oracle, c, m, nbp_only=True)
        refs.append(capture(o, oracle.WdspChannel.HOOK_FMSQ, x5[c])[0].astype(np.complex64))
        o.close()
    return refs


def test_one_channel_leaves_the_others_alone(qh, x5, nbp_refs):
    a, b = engine(qh, MODES), engine(qh, MODES)
    try:
        a.set_sender(2, 1)
        ya, rows = _run(a, x5, CALLS, [2])
        yb, _ = _run(b, x5, CALLS, [])
        r = rel_rms(rows[2], nbp_refs[2])
        print("sender row 2 rel rms", r)
        assert r < ULP, r
        for c in range(5):
            d = rel_rms(ya[c], yb[c])
            print("output", c, d)
            assert d < TOL, (c, d)
        with pytest.raises(qh.QuiskHipError):
            a.sender_rows_host(1)                           # its sender is off
    finally:
        a.close(); b.close()


def test_every_mode(qh, x5, nbp_refs):
    e = engine(qh, MODES)
    try:
        e.set_sender(-1, 1)
        _, rows = _run(e, x5, CALLS, range(5))
        for c in range(5):
            r = rel_rms(rows[c], nbp_refs[c])
            print("sender row", c, r)
            assert r < ULP, (c, r)
    finally:
        e.close()


def test_an_engine_that_never_enabled_a_tap(qh, x5):
    """the setters with run 0 on one engine, none on the other: the same bits and the same device bytes"""
    a, b = engine(qh, MODES), engine(qh, MODES)
    try:
        a.set_sender(-1, 0); a.set_siphon(-1, 0)
        pos = 0
        for nb in CALLS:
            xa = np.ascontiguousarray(x5[:, pos:pos + nb * 1024])
            assert np.array_equal(a.process_host(xa), b.process_host(xa)), nb
            pos += nb * 1024
        assert a.device_bytes() == b.device_bytes()
    finally:
        a.close(); b.close()


def test_snba_channel_row_is_nbp0s_output(qh, oracle):
    """bpsnba at position 0 replaces nbp0's output behind the sender's point (RXA.c:570-572)"""
    calls = (3, 1, 17)
    x = signal([1, 1], sum(calls) * 1024, seed=5)
    e = engine(qh, [1, 1])
    o = oracle_channel(oracle, 1, 1, nbp_only=True)
    try:
        e.SetRXASNBARun(1, 1)
        e.set_sender(1, 1)
        _, rows = _run(e, x, calls, [1])
        ref = capture(o, oracle.WdspChannel.HOOK_FMSQ, x[1])[0].astype(np.complex64)
        r = rel_rms(rows[1], ref)
        print("snba channel's sender row", r)
        assert r < ULP, r
    finally:
        e.close(); o.close()


@pytest.mark.parametrize("dsp_size", [64, 2048])
def test_other_block_sizes(qh, oracle, dsp_size):
    calls = (3, 1, 5) if dsp_size == 2048 else (3, 1, 17, 7)
    x = signal([1], sum(calls) * 4 * dsp_size, seed=dsp_size)
    e = engine(qh, [1], dsp_size=dsp_size)
    o = oracle_channel(oracle, 0, 1, dsp_size=dsp_size, nbp_only=True)
    try:
        e.set_sender(0, 1)
        _, rows = _run(e, x, calls, [0])
        ref = capture(o, oracle.WdspChannel.HOOK_FMSQ, x[0])[0].astype(np.complex64)
        r = rel_rms(rows[0], ref)
        print("dsp_size", dsp_size, r)
        assert r < ULP, r
    finally:
        e.close(); o.close()
