"""Time of WDSP's noise blanker bank (qh_anb.hip) at the bench's config-2 shape: 256 channels, 2^20 samples per channel and call at
192 kHz, fp64, a typical caller's settings (tau = hangtime = advtime = 1e-4, backtau 0.05, threshold 30).  One JSON line: the median
call, the traffic floor and the ratio.  For the kernels' own times run it under
`rocprofv3 --kernel-trace --stats -- python tools/anb_bench.py` (anb_*_kernel).

Input: Gaussian noise whose mean magnitude is the detector's start value 1.0, plus one pulse of 2 samples, 60 times the noise, every
PULSE_EVERY = 20000 samples per channel (9.6 pulses a second at 192 kHz, offset per channel) -- each one a blanking cycle of about 120
samples.  QH_ANB_PULSE_EVERY=0 gives a quiet input (every word takes the copy path).

One pass over the rows moves 256 x 2^20 x 16 B = 4.29 GB.  The algorithm needs the detector to read them once and the apply pass to read
and write them once: 12.9 GB, 1.6 ms at 8 TB/s.  The detector as built reads them twice (det 0 and det 1)."""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    import torch
    import quisk_amd as qh
    dev = torch.device("cuda:0")
    nch, n = int(os.environ.get("QH_ANB_NCH", "256")), int(os.environ.get("QH_ANB_N", str(1 << 20)))
    steps, warmup = int(os.environ.get("QH_ANB_STEPS", "7")), 2
    every = int(os.environ.get("QH_ANB_PULSE_EVERY", "20000"))
    rate = float(os.environ.get("QH_ANB_RATE", "192000"))
    gen = torch.Generator(device=dev)
    gen.manual_seed(7)
    x = torch.empty((nch, n), dtype=torch.complex128, device=dev)
    for c in range(nch):
        x[c] = torch.complex(torch.randn(n, dtype=torch.float64, device=dev, generator=gen), torch.randn(n, dtype=torch.float64, device=dev, generator=gen)) * 0.8
        if every > 0:
            p = torch.arange((37 * c) % every + 100, n - 2, every, device=dev)
            x[c, p] += 48.0
            x[c, p + 1] += 48.0
    y = torch.empty_like(x)
    nb = qh.WdspNoiseBlanker(nch, rate, tau=1e-4, hangtime=1e-4, advtime=1e-4, backtau=0.05, threshold=30.0)
    torch.cuda.synchronize(dev)
    for _ in range(warmup):
        nb.process_ptr(x.data_ptr(), n, y.data_ptr(), n, n)
    nb.synchronize()
    ms = []
    for _ in range(steps):
        t0 = time.perf_counter()
        nb.process_ptr(x.data_ptr(), n, y.data_ptr(), n, n)
        nb.synchronize()
        ms.append((time.perf_counter() - t0) * 1e3)
    med = sorted(ms)[len(ms) // 2]
    zeros = int((y[0] == 0).sum().item())
    one = nch * n * 16
    floor = 3 * one / 8e12 * 1e3
    print(json.dumps({"nch": nch, "n": n, "rate": rate, "pulse_every": every, "ms_call": med, "one_pass_GB": one / 1e9,
                      "floor_ms_2r1w_at_8TBps": floor, "floor_over_call": floor / med, "zeros_ch0": zeros}))
    nb.close()


if __name__ == "__main__":
    main()
