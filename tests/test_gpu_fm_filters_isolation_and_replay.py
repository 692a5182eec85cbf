"""Engines whose FM channels run different filter designs under launch-sequence replay.  -m gpu.

With graph replay on, block-sized calls of an engine with two designs give the plain path's bits, call by call; a filter setter between
calls drops the captured sequences (qh_rxa_graph_launches stops growing for one call) and the result is still the plain path's."""
import numpy as np
import pytest

from rxa_fm_filters_ref import BAND_B, FM
from test_gpu_rxa_fm_filters import AM, USB, Bank, _input

pytestmark = pytest.mark.gpu
SIZE = 64


def _walk(qh, replay, ncall, nblk, x, setters):
    import torch
    dev = torch.device("cuda:0")
    modes = [FM, FM, FM, USB, AM]
    b = Bank(qh, modes, refs=False)
    e = b.e
    e.SetRXAFMAFFilter(1, *BAND_B)
    e.SetRXAFMNCaud(2, 1024)
    e.set_graph_replay(replay)
    n = nblk * SIZE
    d_in = torch.zeros((len(modes), n), dtype=torch.complex128, device=dev)
    d_out = torch.zeros((len(modes), n), dtype=torch.complex128, device=dev)
    ys, grew = [], []
    try:
        for k in range(ncall):
            if k in setters:
                setters[k](e)
            before = e.graph_launches()
            d_in.copy_(torch.from_numpy(np.ascontiguousarray(x[:, k * n:(k + 1) * n])))
            e.process_ptr(d_in.data_ptr(), n, d_out.data_ptr(), n, nblk)
            torch.cuda.synchronize()
            ys.append(d_out.cpu().numpy())
            grew.append(e.graph_launches() - before)
    finally:
        b.close()
    return ys, grew


def test_replay_gives_the_plain_paths_bits_and_a_setter_drops_the_graphs(qh):
    ncall, nblk = 24, 4
    x = _input(5, calls=(ncall * nblk,))
    setters = {9: lambda e: e.SetRXAFMAFFilter(0, *BAND_B),            # two rows still, channel 0 moves to the other
               15: lambda e: e.SetRXAFMNCde(1, 512),                     # a third de-emphasis row
               20: lambda e: e.SetRXAFMMPaud(2, 0)}                      # the value it has: the graphs go all the same, as for every setter
    plain, _ = _walk(qh, False, ncall, nblk, x, setters)
    replayed, grew = _walk(qh, True, ncall, nblk, x, setters)
    print("graph launches per call: %s" % grew)
    assert sum(grew) > 0
    for k in setters:
        assert grew[k] == 0, (k, grew)
    assert grew[8] > 0 and grew[14] > 0 and grew[19] > 0 and grew[23] > 0, grew
    for k in range(ncall):
        assert np.array_equal(plain[k], replayed[k]), k
