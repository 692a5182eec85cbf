"""gen0 beside other channels and under launch-sequence replay.  -m gpu.

A channel that runs its generator sends the call to the per-mode path without the two-stream split.  The other channels then get that
form's bits exactly -- the form a sender tap selects too -- and stay within the distance DESIGN.md section 7 records between two forms
(1.9e-14 of the peak, held at 1e-13 here and printed) of the engine that runs neither.  An engine on which no generator runs is the
engine it was: the same bits, the same device bytes.  Replayed from a hipGraph, every mode gives the plain path's bits call by call,
the state's advance on the device included, with settings walked between replays."""
import numpy as np
import pytest

from test_gpu_rxa_eqp import AM, FM, USB, _engine, _input

pytestmark = pytest.mark.gpu
MIXED = [USB, AM, FM, USB]
CALLS = (8, 8, 40, 3)


def _walk(e, x, calls):
    ys, pos = [], 0
    for nb in calls:
        ys.append(e.process_host(np.ascontiguousarray(x[:, pos:pos + nb * e.dsp_insize])))
        pos += nb * e.dsp_insize
    return np.concatenate(ys, 1)


def test_the_other_channels_get_the_per_mode_forms_bits(qh):
    x = _input(MIXED, sum(CALLS) * 1024, 192000.0, True)
    outs = {}
    for what in ("plain", "sender", "gen"):
        e = _engine(qh, MIXED)
        try:
            if what == "sender":
                e.set_sender(3, 1)
            elif what == "gen":
                e.SetRXAPreGenMode(3, 1); e.SetRXAPreGenRun(3, 1)
            outs[what] = _walk(e, x, CALLS)
        finally:
            e.close()
    for c in (0, 1, 2):
        assert np.array_equal(outs["gen"][c], outs["sender"][c]), c
        d = np.abs(outs["gen"][c] - outs["plain"][c]).max() / np.abs(outs["plain"][c]).max()
        print("channel %d: against the engine that runs neither, %.3g of the peak" % (c, d))
        assert d <= 1e-13, (c, d)
    assert not np.array_equal(outs["gen"][3], outs["plain"][3])


@pytest.mark.parametrize("modes", [MIXED, [USB] * 4], ids=["mixed", "linear"])
def test_setters_without_run_leave_the_engine_as_it_was(qh, modes):
    a, b = _engine(qh, modes), _engine(qh, modes)
    x = _input(modes, 6 * 4096, 192000.0, True)
    try:
        a.SetRXAPreGenMode(-1, 0); a.SetRXAPreGenToneMag(0, 0.5); a.SetRXAPreGenToneFreq(1, 700.0); a.SetRXAPreGenNoiseMag(2, 0.1)
        a.SetRXAPreGenSweepMag(3, 0.2); a.SetRXAPreGenSweepFreq(0, -1000.0, 1000.0); a.SetRXAPreGenSweepRate(0, 9000.0); a.set_gen_seed(1, 5)
        a.SetRXAPreGenRun(-1, 0)
        for k in range(6):
            xa = np.ascontiguousarray(x[:, k * 4096:(k + 1) * 4096])
            assert np.array_equal(a.process_host(xa), b.process_host(xa)), k
        assert a.device_bytes() == b.device_bytes()
    finally:
        a.close(); b.close()


def test_graph_replay_matches_the_plain_path(qh):
    """five calls per mode and setting, replayed against plain, bit for bit: tone, two-tone, noise (on two channels), sweep (resetting
    inside the calls), pulse, silence, with a frequency change, a sweep restart, a seed, a flush and a generator switched off between
    replays"""
    import torch
    dev = torch.device("cuda:0")
    nch, nblk = 4, 3
    steps = [lambda e: (e.SetRXAPreGenMode(3, 0), e.SetRXAPreGenMode(1, 2)),
             lambda e: e.SetRXAPreGenToneFreq(3, -1234.5),
             lambda e: e.SetRXAPreGenMode(3, 1),
             lambda e: (e.SetRXAPreGenMode(3, 2), e.SetRXAPreGenNoiseMag(3, 0.3)),
             lambda e: e.set_gen_seed(3, 99),
             lambda e: (e.SetRXAPreGenMode(3, 3), e.SetRXAPreGenSweepFreq(3, -2000.0, 2000.0), e.SetRXAPreGenSweepRate(3, 400000.0)),
             lambda e: e.SetRXAPreGenSweepRate(3, 300000.0),
             lambda e: e.SetRXAPreGenMode(3, 6),
             lambda e: e.flush(),
             lambda e: e.SetRXAPreGenMode(3, 99),
             lambda e: (e.SetRXAPreGenMode(3, 0), e.SetRXAPreGenRun(1, 0))]
    x = _input(MIXED, len(steps) * 5 * nblk * 1024, 192000.0, True)
    res, launches = [], 0
    for replay in (False, True):
        e = _engine(qh, MIXED)
        e.SetRXAPreGenRun(3, 1); e.SetRXAPreGenRun(1, 1)
        e.set_graph_replay(replay)
        d_in = torch.zeros((nch, nblk * 1024), dtype=torch.complex128, device=dev)
        d_out = torch.zeros((nch, nblk * 256), dtype=torch.complex128, device=dev)
        ys = []
        try:
            for k in range(len(steps) * 5):
                if k % 5 == 0:
                    steps[k // 5](e)
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
    for k in range(len(res[0])):
        assert np.array_equal(res[0][k], res[1][k]), k
    assert np.abs(res[0][2][3]).max() > 0.1                      # (the generator's tone reached channel 3's output)
