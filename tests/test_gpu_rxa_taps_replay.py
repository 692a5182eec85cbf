"""The sender and the siphon under launch-sequence replay: a replayed hipGraph bakes in its kernels' arguments, so the siphon's write
index has to live and move on the device.  Two engines with both taps on every channel, one replaying, 40 one-block calls through the same
device buffers (16 blocks of 256 fill the ring: it wraps twice while replaying): outputs, sender rows and the whole ring bit for bit after
every call.  -m gpu."""
import numpy as np
import pytest

from rxa_taps_util import MODES, engine, signal

pytestmark = pytest.mark.gpu


def test_replayed_calls_match_the_plain_path_bit_for_bit(qh):
    import torch
    dev = torch.device("cuda:0")
    nch, ncall = len(MODES), 40
    x = signal(MODES, ncall * 1024, seed=2)
    res = []
    for replay in (False, True):
        e = engine(qh, MODES)
        e.set_sender(-1, 1); e.set_siphon(-1, 1)
        e.set_graph_replay(replay)
        d_in = torch.zeros((nch, 1024), dtype=torch.complex128, device=dev)
        d_out = torch.zeros((nch, 256), dtype=torch.complex128, device=dev)
        got = []
        try:
            for k in range(ncall):
                d_in.copy_(torch.from_numpy(np.ascontiguousarray(x[:, k * 1024:(k + 1) * 1024])))
                torch.cuda.synchronize()
                e.process_ptr(d_in.data_ptr(), 1024, d_out.data_ptr(), 256, 1)
                e.synchronize()
                got.append((d_out.cpu().numpy(), np.stack([e.sender_rows_host(c) for c in range(nch)]),
                            np.stack([e.get_sip(c, 4096) for c in range(nch)])))
            if replay:
                assert e.graph_launches() > 0
        finally:
            e.close()
        res.append(got)
    for k, (a, b) in enumerate(zip(*res)):
        for what, u, v in zip(("output", "sender rows", "siphon"), a, b):
            assert np.array_equal(u, v), (k, what)
    assert np.any(res[0][-1][1]) and np.any(res[0][-1][2])
    # the ring has wrapped: its newest 256 samples after call 39 are not where call 15's were, and the index moved on
    assert not np.array_equal(res[1][39][2], res[1][23][2])
