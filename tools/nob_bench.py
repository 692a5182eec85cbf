"""Time of WDSP's second noise blanker bank (qh_nob.hip) at the shape tools/anb_bench.py uses: 256 channels, 2^20 samples per channel
and call at 192 kHz, fp64, a typical caller's settings (slew = hangtime = advtime = 1e-4, backtau 0.05, threshold 30), and of qh_anb at
the same shape from the same library in the same process, so that the spread from box to box drops out of the ratio.  One JSON line:
per input (quiet; one 2-sample pulse per 20000 samples) and mode (0 and 4) the mean call with min and max, the same for ANB, the ratio
to ANB and to the traffic floor.  For the kernels' own times run it under
`rocprofv3 --kernel-trace --stats -- python tools/nob_bench.py` (nob_*_kernel, anb_*_kernel, and the detector's det_kernel<0 | 1, ...> and
carry_kernel<...>, one instance per bank's Param and State), one input and mode a run
(QH_NOB_INPUTS=quiet|pulsed, QH_NOB_MODES=0|4), since the statistics are per kernel name; QH_NOB_N and QH_NOB_PULSE_EVERY vary the
samples and the events to show what each kernel's time follows.

One pass over the rows moves 256 x 2^20 x 16 B = 4.29 GB; the floor is one read and one write of the rows, 8.6 GB, 1.07 ms at 8 TB/s.
As built the detector reads the rows twice (det 0 and det 1), the copy reads and writes them once, and the history copy moves
2 x 256 x 50752 x 16 B = 0.42 GB."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from blanker_bench_common import add_pulses, noise, time_calls  # noqa: E402


def _time(bank, x, y, n, steps):
    ms = time_calls(bank, x, y, n, steps)
    return {"mean_ms": sum(ms) / len(ms), "min_ms": min(ms), "max_ms": max(ms)}


def main():
    import torch
    import quisk_amd as qh
    dev = torch.device("cuda:0")
    nch, n = int(os.environ.get("QH_NOB_NCH", "256")), int(os.environ.get("QH_NOB_N", str(1 << 20)))
    steps = int(os.environ.get("QH_NOB_STEPS", "7"))
    every = int(os.environ.get("QH_NOB_PULSE_EVERY", "20000"))
    rate = float(os.environ.get("QH_NOB_RATE", "192000"))
    inputs = os.environ.get("QH_NOB_INPUTS", "quiet,pulsed").split(",")
    modes = [int(m) for m in os.environ.get("QH_NOB_MODES", "0,4").split(",")]
    quiet = noise(torch, dev, nch, n)
    pulsed = add_pulses(torch, quiet.clone(), every)
    y = torch.empty_like(quiet)
    torch.cuda.synchronize(dev)
    one = nch * n * 16
    floor = 2 * one / 8e12 * 1e3
    res = {"nch": nch, "n": n, "rate": rate, "pulse_every": every, "one_pass_GB": one / 1e9, "floor_ms_1r1w_at_8TBps": floor}
    for name, x in (("quiet", quiet), ("pulsed", pulsed)):
        if name not in inputs:
            continue
        anb = qh.WdspNoiseBlanker(nch, rate, tau=1e-4, hangtime=1e-4, advtime=1e-4, backtau=0.05, threshold=30.0)
        res["anb_" + name] = ta = _time(anb, x, y, n, steps)
        anb.close()
        for mode in modes:
            nb = qh.WdspNoiseBlanker2(nch, rate, mode, slewtime=1e-4, hangtime=1e-4, advtime=1e-4, backtau=0.05, threshold=30.0)
            t = _time(nb, x, y, n, steps)
            t["over_anb"] = t["mean_ms"] / ta["mean_ms"]
            t["floor_over_call"] = floor / t["mean_ms"]
            res["nob_%s_mode%d" % (name, mode)] = t
            nb.close()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
