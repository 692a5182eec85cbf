"""The FM squelch beside other channels and under launch-sequence replay.  -m gpu.

A channel that turns the squelch on moves no other channel's output by a bit: the stage runs on its own channels' rows with kernels and
buffers of its own, and the forms the engine picks for a call (two streams, stores straight to the caller's rows, fused loads) do not look
at it.  That includes the other FM channel, which shares the de-emphasis tile with the squelched one in both engines: the squelch acts
behind that stage, so the tile's inputs are the same and the partner keeps its bits too (tests/test_gpu_channel_isolation.py bounds FM
partners only where a partner's input differs)."""
import numpy as np
import pytest

from quisk_amd import synth
from test_gpu_rxa_fmsq import FM, USB, _engine, _input

pytestmark = pytest.mark.gpu
AM = 6


def _mixed(qh):
    modes = [USB, AM, FM, FM]
    e = _engine(qh, modes)
    e.RXASetPassband(1, -4000.0, 4000.0)
    return e


def test_turning_it_on_moves_no_other_channel(qh):
    calls = (8, 8, 8, 40, 8, 160, 3)
    x = _input(4, sum(calls) * 1024)
    outs = []
    for k in range(2):
        e = _mixed(qh)
        ys, pos = [], 0
        try:
            for i, nb in enumerate(calls):
                if k and i == 2:
                    e.SetRXAFMSQRun(3, 1); e.SetRXAFMSQThreshold(3, 0.6)
                ys.append(e.process_host(np.ascontiguousarray(x[:, pos:pos + nb * 1024])))
                pos += nb * 1024
        finally:
            e.close()
        outs.append(np.concatenate(ys, 1))
    for c in range(3):
        assert np.array_equal(outs[0][c], outs[1][c]), c
    first = sum(calls[:2]) * 256
    assert np.array_equal(outs[0][3, :first], outs[1][3, :first])
    assert not np.any(outs[1][3, first:first + 4000]) and np.any(outs[0][3, first:first + 4000])        # muted for the ready delay
    assert np.any(outs[1][3, first:])                                                                   # ... and open on the carrier later


def test_setters_without_run_leave_the_engine_as_it_was(qh):
    """every FMSQ setter but Run, and Run 0, on one engine, none on the other: the same bits and the same device bytes"""
    a, b = _mixed(qh), _mixed(qh)
    a.SetRXAFMSQThreshold(-1, 0.4); a.SetRXAFMSQNC(2, 1024); a.SetRXAFMSQNC(3, 4096); a.SetRXAFMSQMP(3, 1); a.SetRXAFMSQRun(-1, 0)
    x = _input(4, 10 * 4096)
    try:
        for k in range(10):
            xa = np.ascontiguousarray(x[:, k * 4096:(k + 1) * 4096])
            assert np.array_equal(a.process_host(xa), b.process_host(xa)), k
        assert a.device_bytes() == b.device_bytes()
        assert a.debug_fmsq(3) is None
    finally:
        a.close(); b.close()


def test_graph_replay_matches_the_plain_path(qh):
    """replayed calls give the plain path's bits, call by call: through the ready delay, an opening, a threshold change and calls in which
    the list of FMSQ channels changes (one more channel, then one fewer)"""
    import torch
    dev = torch.device("cuda:0")
    nch, nblk, ncall = 4, 24, 44
    x = _input(nch, ncall * nblk * 1024, start_on=(3,))
    res, launches = [], 0
    for replay in (False, True):
        e = _mixed(qh)
        e.SetRXAFMSQRun(2, 1)
        e.set_graph_replay(replay)
        d_in = torch.zeros((nch, nblk * 1024), dtype=torch.complex128, device=dev)
        d_out = torch.zeros((nch, nblk * 256), dtype=torch.complex128, device=dev)
        ys = []
        try:
            for k in range(ncall):
                if k == 8:
                    e.SetRXAFMSQRun(3, 1)
                elif k == 20:
                    e.SetRXAFMSQThreshold(2, 0.6)
                elif k == 32:
                    e.SetRXAFMSQRun(2, 0)
                d_in.copy_(torch.from_numpy(np.ascontiguousarray(x[:, k * nblk * 1024:(k + 1) * nblk * 1024])))
                e.process_ptr(d_in.data_ptr(), nblk * 1024, d_out.data_ptr(), nblk * 256, nblk)
                torch.cuda.synchronize()
                ys.append(d_out.cpu().numpy())
            if replay:
                launches = e.graph_launches()
        finally:
            e.close()
        res.append(ys)
    assert launches > 0
    for k in range(ncall):
        assert np.array_equal(res[0][k], res[1][k]), k
    y = np.concatenate(res[0], 1)
    for c in (2, 3):
        assert np.any(y[c] == 0) and np.any(y[c] != 0)
