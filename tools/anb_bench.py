"""Time of WDSP's noise blanker bank (qh_anb.hip) at the bench's config-2 shape: 256 channels, 2^20 samples per channel and call at
192 kHz, fp64, a typical caller's settings (tau = hangtime = advtime = 1e-4, backtau 0.05, threshold 30).  One JSON line: the median
call, the traffic floor and the ratio.  For the kernels' own times run it under
`rocprofv3 --kernel-trace --stats -- python tools/anb_bench.py` (anb_*_kernel; the detector's are det_kernel<0 | 1, AnbParam, AnbState>
and carry_kernel<AnbParam, AnbState>).

Input: Gaussian noise whose mean magnitude is the detector's start value 1.0, plus one pulse of 2 samples, 60 times the noise, every
PULSE_EVERY = 20000 samples per channel (9.6 pulses a second at 192 kHz, offset per channel) -- each one a blanking cycle of about 120
samples.  QH_ANB_PULSE_EVERY=0 gives a quiet input (every word takes the copy path).

One pass over the rows moves 256 x 2^20 x 16 B = 4.29 GB.  The algorithm needs the detector to read them once and the apply pass to read
and write them once: 12.9 GB, 1.6 ms at 8 TB/s.  The detector as built reads them twice (det 0 and det 1)."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from blanker_bench_common import add_pulses, noise, time_calls  # noqa: E402


def main():
    import torch
    import quisk_amd as qh
    dev = torch.device("cuda:0")
    nch, n = int(os.environ.get("QH_ANB_NCH", "256")), int(os.environ.get("QH_ANB_N", str(1 << 20)))
    steps, warmup = int(os.environ.get("QH_ANB_STEPS", "7")), 2
    every = int(os.environ.get("QH_ANB_PULSE_EVERY", "20000"))
    rate = float(os.environ.get("QH_ANB_RATE", "192000"))
    x = noise(torch, dev, nch, n)
    if every > 0:
        add_pulses(torch, x, every)
    y = torch.empty_like(x)
    nb = qh.WdspNoiseBlanker(nch, rate, tau=1e-4, hangtime=1e-4, advtime=1e-4, backtau=0.05, threshold=30.0)
    torch.cuda.synchronize(dev)
    ms = time_calls(nb, x, y, n, steps, warmup)
    med = sorted(ms)[len(ms) // 2]
    zeros = int((y[0] == 0).sum().item())
    one = nch * n * 16
    floor = 3 * one / 8e12 * 1e3
    print(json.dumps({"nch": nch, "n": n, "rate": rate, "pulse_every": every, "ms_call": med, "one_pass_GB": one / 1e9,
                      "floor_ms_2r1w_at_8TBps": floor, "floor_over_call": floor / med, "zeros_ch0": zeros}))
    nb.close()


if __name__ == "__main__":
    main()
