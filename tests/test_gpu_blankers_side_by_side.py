"""WDSP's two noise blankers side by side in one process: they share the detector's kernels (quisk_amd/csrc/qh_blank_det.hpp) and the
banks' host scaffold (qh_bank.hpp: DetBank), so what could newly go wrong is state or scratch of one bank reaching another.  A WdspNoiseBlanker
and two WdspNoiseBlanker2 (modes 0 and 4) work on one caller stream, their calls enqueued back to back cut by cut; after the third cut
the first bank is destroyed and a fresh WdspNoiseBlanker2 takes its rows from there (a free of scratch another bank still used would
show).  Every bank's output must be its restatement's, np.array_equal; as in test_gpu_anb.py and test_gpu_nob.py each restatement first
shows a trigger margin of at least 1e-9 and that triggers and blanks occur -- conditions on the input, not tolerances.  -m gpu."""
import numpy as np
import pytest

import test_gpu_anb
import test_gpu_nob

pytestmark = pytest.mark.gpu

RATE, N = 48000, 20000
CUTS = [0, 4000, 4001, 12345, N]                # the delays are 8 (ANB) and 1227 (NOB) samples; one cut is a single sample
SWAP = 3                                        # the ANB bank leaves after this many cuts
ANB_PRM, NOB_PRM = test_gpu_anb.PARAMS["typical"], test_gpu_nob.PARAMS["typical"]


def test_banks_alternating_on_one_stream_keep_to_themselves(qh):
    import torch
    xa = test_gpu_anb._input(2, N, seed=101)
    xn = test_gpu_nob._input(3, N, seed=102, rate=RATE, name="typical")
    # the restatements, and what they say about the inputs
    ref_a, anbs = test_gpu_anb._reference(RATE, ANB_PRM, xa[:, :CUTS[SWAP]], CUTS[:SWAP + 1])
    test_gpu_anb._check_input(ref_a, anbs, "side by side")
    ref_n = {}
    for mode in (0, 4):
        ref_n[mode], nobs = test_gpu_nob._reference(RATE, mode, NOB_PRM, xn, CUTS)
        test_gpu_nob._check_input(nobs, "typical", "side by side, mode %d" % mode)
    ref_f, fresh = test_gpu_nob._reference(RATE, 0, NOB_PRM, xa[:, CUTS[SWAP]:], [0, N - CUTS[SWAP]])
    for a in fresh:
        print("fresh nob: trigger margin %.3e, %d triggers, %d blanks" % (a.margin, a.triggers, a.blanks))
        assert a.margin >= test_gpu_nob.MARGIN and a.triggers > 0 and a.blanks > 0
    assert anbs[0].delay == 8 and nobs[0].delay == 1227

    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        da, dn = torch.from_numpy(xa).cuda(), torch.from_numpy(xn).cuda()
        oa, on = torch.zeros_like(da), {0: torch.zeros_like(dn), 4: torch.zeros_like(dn)}
        anb = qh.WdspNoiseBlanker(2, RATE, stream=s.cuda_stream, **ANB_PRM)
        nob = {mode: qh.WdspNoiseBlanker2(3, RATE, mode, stream=s.cuda_stream, **NOB_PRM) for mode in (0, 4)}

        def rows(t, a):
            return t.data_ptr() + 16 * a

        for k, (a, b) in enumerate(zip(CUTS[:-1], CUTS[1:])):
            if k == SWAP:
                anb.close()
                anb = qh.WdspNoiseBlanker2(2, RATE, 0, stream=s.cuda_stream, **NOB_PRM)
            anb.process_ptr(rows(da, a), N, rows(oa, a), N, b - a)
            nob[0].process_ptr(rows(dn, a), N, rows(on[0], a), N, b - a)
            nob[4].process_ptr(rows(dn, a), N, rows(on[4], a), N, b - a)
        ya, yn = oa.cpu().numpy(), {mode: on[mode].cpu().numpy() for mode in (0, 4)}
        for bank in (anb, nob[0], nob[4]):
            bank.close()
    assert np.array_equal(ya[:, :CUTS[SWAP]], ref_a)
    assert np.array_equal(ya[:, CUTS[SWAP]:], ref_f)
    for mode in (0, 4):
        assert np.array_equal(yn[mode], ref_n[mode]), mode
