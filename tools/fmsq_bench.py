"""Time of xfmsq (qh_fmsq.hpp) at one GPU's share of BASELINE config 4 (tools/bench_configs.py: 256 channels, mode by c mod 3 = USB / AM /
FM, 2^20 dsp samples per channel and call, fp64).  One JSON line: the whole call with FMSQ off, with FMSQ on in every FM channel, the
difference, and the engine's own front / band / rest split of the on-case (qh_rxa_enable_timing).  For the kernels' own times and counts
run it under `rocprofv3 --kernel-trace --stats -- python tools/fmsq_bench.py` (QH_FQ_ONLY=off / on times one case alone, so that the
off-case's kernel list can be set beside the parent commit's: it must hold nothing new)."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))


def main():
    import torch
    import quisk_amd as qh
    import bench_configs as bc
    dev = torch.device("cuda:0")
    only = os.environ.get("QH_FQ_ONLY", "")
    steps = int(os.environ.get("QH_FQ_STEPS", "5"))
    L = bc.setup_config4(torch, qh, dev)
    sync = lambda: torch.cuda.synchronize(dev)
    r = {"config": "4 (one GPU's share): %d ch x 192 k, %d blocks a call" % (L.nch, L.nblk)}
    fm = [c for c in range(L.nch) if bc.C4_MODES[c % 3] == 5]
    has = hasattr(L.eng, "debug_fmsq")
    if only != "on":
        r["ms_fmsq_off"] = bc.timed(L.step, sync, steps=steps, warmup=2) * 1e3
    if only != "off" and has:
        for c in fm:
            L.eng.SetRXAFMSQRun(c, 1)
        r["ms_fmsq_on"] = bc.timed(L.step, sync, steps=steps, warmup=2) * 1e3
        L.eng.enable_timing(True)
        L.step()
        kt = L.eng.timing_ms()
        L.eng.enable_timing(False)
        r.update(front_ms_on=kt[0], band_ms_on=kt[1], rest_ms_on=kt[2], fm_channels=len(fm),
                 states=sorted({L.eng.debug_fmsq(c)[2] for c in fm}))
        if "ms_fmsq_off" in r:
            r["ms_added"] = r["ms_fmsq_on"] - r["ms_fmsq_off"]
    print(json.dumps(r))
    L.eng.close()


if __name__ == "__main__":
    main()
