"""Cost of xsnba (qh_snba.hpp) by DSP rate and form: 256 USB channels with the blanker on, in = dsp = out rate, dsp_size 1024, one second
of signal per call (tones, noise and some 25 impulses a second per channel, so that frames do get repaired), at dsp_rate 48 k with the
single kernel (form 0) and with the three passes (form 1), and at 96 k, 192 k and 384 k, where only the passes run.

    python tools/bench_snba_rates.py [--out profiles/snba_rates.json] [--no-profile] [--only 48k_form0,...]

Per configuration: the time of a whole call from device events, the median of three turns behind one warm-up call with the spread
(max - min) -- this includes nbp0, bpsnba and bp1 around the blanker --, and, from a run of its own under `rocprofv3 --kernel-trace
--stats` (tracing slows the host: its call time is not used), the split into the blanker's kernels: the decimation pass, the frame
kernel, the interpolation pass and the two small history kernels.  Two things to read off, no gate on either: the frame kernel's time
per second of 12 kHz data should not depend on the rate; and each resampler pass against a device-to-device copy that moves as many
bytes as the pass reads and writes (`copy_ms`)."""
import argparse
import csv
import glob
import json
import os
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

NCH, SIZE, TURNS = 256, 1024, 3
PROFILE_TIMEOUT_S = 180     # the traced run takes some 20 s
CONFIGS = {"48k_form0": (48000, 0), "48k_form1": (48000, 1), "96k": (96000, 0), "192k": (192000, 0), "384k": (384000, 0)}
KERNELS = ("snba_decim_kernel", "snba_interp_kernel", "snba_hist_kernel", "snba_kernel")


def signal(rate, dev):
    """[NCH, one second] complex128 on the device: the USB tones of the tests' `crackle` at 0 Hz carrier, noise, 25 impulses a second"""
    import math
    import torch
    n = rate // SIZE * SIZE
    g = torch.Generator(device=dev)
    g.manual_seed(7)
    t = torch.arange(n, device=dev, dtype=torch.float64) / rate
    x = torch.zeros((NCH, n), dtype=torch.complex128, device=dev)
    for a, f in ((0.08, 700.0), (0.05, 1210.0), (0.03, 2300.0)):
        x += a * torch.exp(2j * math.pi * f * t)[None, :]
    x += 0.01 * torch.view_as_complex(torch.randn((NCH, n, 2), generator=g, device=dev, dtype=torch.float64))
    k = torch.randint(0, n, (NCH, 25), generator=g, device=dev)
    amp = 2.0 + 6.0 * torch.rand((NCH, 25), generator=g, device=dev, dtype=torch.float64)
    torch.view_as_real(x)[:, :, 0].scatter_add_(1, k, amp)
    return x


def run(name, turns):
    import torch
    import quisk_amd as qh
    rate, form = CONFIGS[name]
    dev = torch.device("cuda:0")
    x = signal(rate, dev)
    n = x.shape[1]
    y = torch.zeros_like(x)
    stream = torch.cuda.Stream(dev)
    torch.cuda.synchronize(dev)
    e = qh.RxaEngine(NCH, dsp_size=SIZE, in_rate=rate, dsp_rate=rate, out_rate=rate, stream=stream.cuda_stream)
    e.SetRXAShiftRun(-1, 0); e.RXANBPSetRun(-1, 1); e.SetRXAMode(-1, 1); e.RXASetPassband(-1, 300.0, 3000.0)
    e.SetRXAAGCMode(-1, 0); e.SetRXAAGCFixed(-1, 6.0); e.SetRXASNBARun(-1, 1)
    e.set_snba_form(form)
    nblk = n // SIZE
    e.process_ptr(x.data_ptr(), n, y.data_ptr(), n, nblk)          # warm-up: allocations, designs
    e.synchronize()
    ms = []
    for _ in range(turns):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        e.process_ptr(x.data_ptr(), n, y.data_ptr(), n, nblk)
        e1.record(stream)
        e1.synchronize()
        ms.append(e0.elapsed_time(e1))
    finite = bool(torch.isfinite(torch.view_as_real(y)).all().item())
    nbytes = e.device_bytes()
    e.close()
    res = {"dsp_rate": rate, "form": "three passes" if form == 1 or rate > 48000 else "single kernel", "ms_per_call": sorted(ms)[len(ms) // 2],
           "spread_ms": max(ms) - min(ms), "turns_ms": ms, "finite": finite, "device_bytes": nbytes}
    if res["form"] == "three passes":
        # a copy that moves what a resampler pass moves: it reads the rows at the DSP rate (16 B a sample) and writes 12 kHz rows (8 B), or
        # the other way round; a copy of half that sum reads and writes as much
        moved = NCH * (n * 16 + n * 12000 // rate * 8)
        a = torch.empty(moved // 2, dtype=torch.uint8, device=dev)
        b = torch.empty_like(a)
        with torch.cuda.stream(stream):
            b.copy_(a)
            cs = []
            for _ in range(turns):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(stream); b.copy_(a); e1.record(stream)
                e1.synchronize()
                cs.append(e0.elapsed_time(e1))
        res["pass_bytes_moved"] = moved
        res["copy_ms"] = sorted(cs)[len(cs) // 2]
    return res


def profile(name):
    """this program's --inner run of one configuration under rocprofv3 -> {kernel: {calls, avg_ms}} for the blanker's kernels"""
    with tempfile.TemporaryDirectory() as tmp:
        cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", tmp, "-o", "snba", "--", sys.executable, os.path.abspath(__file__),
               "--inner", name]
        try:
            r = subprocess.run(cmd, capture_output=True, text=True, cwd=tmp, timeout=PROFILE_TIMEOUT_S)
        except subprocess.TimeoutExpired:
            raise RuntimeError("rocprofv3 did not end within %d s" % PROFILE_TIMEOUT_S)
        if r.returncode != 0:
            raise RuntimeError("rocprofv3 failed: %s" % r.stderr[-2000:])
        files = glob.glob(os.path.join(tmp, "**", "*kernel_stats.csv"), recursive=True)
        if not files:
            raise RuntimeError("rocprofv3 left no kernel_stats.csv")
        split = {}
        for row in csv.DictReader(open(files[0])):
            for key in KERNELS:
                if key in row["Name"]:
                    split[key] = {"calls": int(row["Calls"]), "avg_ms": float(row["AverageNs"]) / 1e6, "min_ms": float(row["MinNs"]) / 1e6,
                                  "max_ms": float(row["MaxNs"]) / 1e6}
                    break
        return split


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "snba_rates.json"))
    ap.add_argument("--no-profile", action="store_true")
    ap.add_argument("--only", default="", help="comma-separated configurations (default: all)")
    ap.add_argument("--inner", default="", help="one configuration, one turn, no JSON file: the run rocprofv3 traces")
    a = ap.parse_args()
    if a.inner:
        print(json.dumps(run(a.inner, 1)))
        return
    names = [s for s in a.only.split(",") if s] or list(CONFIGS)
    res = {"shape": {"nch": NCH, "dsp_size": SIZE, "seconds_per_call": 1, "mode": "USB, nbp0 + bpsnba + bp1 around the blanker, fixed AGC",
                     "turns": TURNS, "warmup_calls": 1}, "configs": {}}
    for name in names:
        c = run(name, TURNS)
        if not a.no_profile:
            c["kernels_rocprofv3"] = k = profile(name)
            if "snba_kernel" in k and c["form"] == "three passes":      # (the single kernel has both resamplers inside: no frame time)
                c["frame_kernel_ms_per_second_of_12k"] = k["snba_kernel"]["avg_ms"]
            for key, tag in (("snba_decim_kernel", "decim_over_copy"), ("snba_interp_kernel", "interp_over_copy")):
                if key in k and "copy_ms" in c:
                    c[tag] = k[key]["avg_ms"] / c["copy_ms"]
        res["configs"][name] = c
        print(name, json.dumps(c), flush=True)
    if "48k_form0" in res["configs"] and "48k_form1" in res["configs"]:
        res["form1_over_form0_at_48k"] = res["configs"]["48k_form1"]["ms_per_call"] / res["configs"]["48k_form0"]["ms_per_call"]
    res["source"] = ("tools/bench_snba_rates.py: device events around one call of one second, median of %d turns; kernel split from rocprofv3 "
                     "--kernel-trace --stats in a run of its own per configuration" % TURNS)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
