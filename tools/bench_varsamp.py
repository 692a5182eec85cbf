"""Time of WDSP's variable-ratio resampler bank (qh_varsamp.hip) at the shape of an audio back end behind a many-channel receiver: 256
channels, 48 k -> 48 k, R = 1024 (rsize 140, one shared h of 1.1 MB), 4096 samples per channel and call, varmode 1, and a var that steps
around 1.0003 from call to call the way rmatch's control loop moves it (a few parts per million a call, another phase per channel).

    python tools/bench_varsamp.py [--out profiles/varsamp_bank.json] [--no-profile]

The call time comes from device events around 50 calls on one stream behind 10 warm-up calls, five such windows, the median; with the
profile (a second run of this program under `rocprofv3 --kernel-trace --stats`, tracing slows the host, so its call time is not used) the
JSON also carries the split of a call into the walk kernel, one lane per channel and serial in the samples, and the filter kernel.
Arithmetic the filter needs per output sample: rsize x (a 2-flop interpolation + two fused multiply-adds) = 6 rsize flop."""
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

NCH, IN_RATE, OUT_RATE, R, N = 256, 48000, 48000, 1024, 4096
WARMUP, CALLS, WINDOWS = 10, 50, 5


def var_of_call(k, nch):
    import numpy as np
    return 1.0003 + 4e-6 * np.sin(0.37 * k + 0.1 * np.arange(nch))


def run(windows):
    import torch
    import quisk_amd as qh
    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev)
    g.manual_seed(1)
    x = torch.view_as_complex(torch.randn((NCH, N, 2), generator=g, device=dev, dtype=torch.float64).contiguous())
    stream = torch.cuda.Stream(dev)                     # (the null stream would make the bank open one of its own)
    torch.cuda.synchronize(dev)
    vs = qh.WdspVarResampler(NCH, IN_RATE, OUT_RATE, R=R, varmode=1, stream=stream.cuda_stream)
    mo = max(vs.max_out(N, var_of_call(k, NCH)) for k in range(WARMUP + windows * CALLS)) + 64
    y = torch.zeros((NCH, mo), dtype=torch.complex128, device=dev)
    cnt = torch.zeros(NCH, dtype=torch.int32, device=dev)
    k = 0
    for _ in range(WARMUP):
        vs.process_ptr(x.data_ptr(), N, y.data_ptr(), mo, N, var_of_call(k, NCH), cnt.data_ptr())
        k += 1
    torch.cuda.synchronize(dev)
    ms, outs = [], []
    for _ in range(windows):
        vars_ = [var_of_call(k + j, NCH) for j in range(CALLS)]
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        for v in vars_:
            vs.process_ptr(x.data_ptr(), N, y.data_ptr(), mo, N, v, cnt.data_ptr())
        e1.record(stream)
        e1.synchronize()
        k += CALLS
        ms.append(e0.elapsed_time(e1) / CALLS)
        outs.append(int(cnt.sum().item()))              # the last call's; every call makes N var samples a channel within one
    torch.cuda.synchronize(dev)
    finite = bool(torch.isfinite(torch.view_as_real(y[:, :int(cnt.min().item())])).all().item())
    vs.close()
    med = sorted(ms)[len(ms) // 2]
    out = outs[len(outs) // 2]
    return {"ms_per_call": med, "ms_per_call_windows": ms, "outputs_per_call": out, "M_output_samples_per_s": out / med / 1e3,
            "filter_GFLOP_per_call": 6.0 * vs_rsize() * out / 1e9, "finite": finite}


def vs_rsize():
    return int(140.0 * max(IN_RATE, OUT_RATE) / min(IN_RATE, OUT_RATE))


def profile():
    """this program's --inner run under rocprofv3 -> {kernel: {calls, avg_us}} for the bank's two kernels"""
    with tempfile.TemporaryDirectory() as tmp:
        cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", tmp, "-o", "vs", "--", sys.executable, os.path.abspath(__file__), "--inner"]
        r = subprocess.run(cmd, capture_output=True, text=True, cwd=tmp)
        if r.returncode != 0:
            raise RuntimeError("rocprofv3 failed: %s" % r.stderr[-2000:])
        files = glob.glob(os.path.join(tmp, "**", "*kernel_stats.csv"), recursive=True)
        if not files:
            raise RuntimeError("rocprofv3 left no kernel_stats.csv")
        split = {}
        for row in csv.DictReader(open(files[0])):
            for key in ("varsamp_walk_kernel", "varsamp_filter_kernel"):
                if key in row["Name"]:
                    split[key] = {"calls": int(row["Calls"]), "avg_us": float(row["AverageNs"]) / 1e3, "min_us": float(row["MinNs"]) / 1e3,
                                  "max_us": float(row["MaxNs"]) / 1e3}
        return split


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "varsamp_bank.json"))
    ap.add_argument("--no-profile", action="store_true")
    ap.add_argument("--inner", action="store_true", help="one window, no JSON file: the run rocprofv3 traces")
    a = ap.parse_args()
    if a.inner:
        print(json.dumps(run(1)))
        return
    res = {"shape": {"nch": NCH, "in_rate": IN_RATE, "out_rate": OUT_RATE, "R": R, "rsize": vs_rsize(), "n_per_call": N, "varmode": 1,
                     "var": "1.0003 + 4e-6 sin(0.37 call + 0.1 ch)", "warmup_calls": WARMUP, "calls_per_window": CALLS, "windows": WINDOWS}}
    res.update(run(WINDOWS))
    if not a.no_profile:
        res["kernels_rocprofv3"] = profile()
        k = res["kernels_rocprofv3"]
        if len(k) == 2:
            res["walk_over_filter"] = k["varsamp_walk_kernel"]["avg_us"] / k["varsamp_filter_kernel"]["avg_us"]
    res["source"] = "tools/bench_varsamp.py: device events around %d calls, median of %d windows; kernel split from rocprofv3 --kernel-trace --stats in a run of its own" % (CALLS, WINDOWS)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
