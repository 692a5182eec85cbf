"""Time of WDSP's diversity combiner bank (qh_div.hip) against a device-to-device copy that moves the same bytes.

    python tools/bench_div.py [--out profiles/div_bank.json]

Two shapes, both mixing (output == nr) with random rotate factors: 256 groups x nr 2 x 65 536 samples (two antennas, many receivers) and
32 groups x nr 8 x 65 536 samples (the widest group).  A call reads nr rows and writes one per group: (nr + 1) 16 n ngroups bytes, the
algorithmic bytes.  The yardstick is a hipMemcpyAsync device-to-device that moves as many: half of them read and half written, so its
size is half the algorithmic bytes.  Both are timed in the same run on the same stream: device events around 50 calls behind 10 warm-up
calls, five such windows, the median.  The kernel is a pure stream, so whatever it falls short of the copy is the finding to explain."""
import argparse
import ctypes as C
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = [(256, 2, 65536), (32, 8, 65536)]
WARMUP, CALLS, WINDOWS = 10, 50, 5
D2D = 3                                                 # hipMemcpyDeviceToDevice


def hip_runtime():
    """the HIP runtime this process has already loaded (PyTorch's own copy: quisk_amd/lib.py)"""
    for line in open("/proc/self/maps"):
        path = line.split()[-1]
        if "libamdhip64" in os.path.basename(path):
            rt = C.CDLL(path)
            rt.hipMemcpyAsync.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p]
            return rt
    raise RuntimeError("no HIP runtime is loaded")


def windows(torch, stream, call):
    for _ in range(WARMUP):
        call()
    stream.synchronize()
    ms = []
    for _ in range(WINDOWS):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        for _ in range(CALLS):
            call()
        e1.record(stream)
        e1.synchronize()
        ms.append(e0.elapsed_time(e1) / CALLS)
    return sorted(ms)[len(ms) // 2], ms


def run_shape(torch, qh, rt, ngroups, nr, n):
    import numpy as np
    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev)
    g.manual_seed(1)
    x = torch.view_as_complex(torch.randn((ngroups, nr, n, 2), generator=g, device=dev, dtype=torch.float64).contiguous())
    y = torch.zeros((ngroups, n), dtype=torch.complex128, device=dev)
    stream = torch.cuda.Stream(dev)                     # (the null stream would make the bank open one of its own)
    torch.cuda.synchronize(dev)
    div = qh.WdspDiversity(ngroups, nr, stream=stream.cuda_stream)
    rng = np.random.default_rng(2)
    for grp in range(ngroups):
        div.set_rotate(rng.uniform(-1, 1, nr), rng.uniform(-1, 1, nr), grp)
    div.set_output(nr)
    bytes_alg = (nr + 1) * 16 * n * ngroups
    ms, ms_all = windows(torch, stream, lambda: div.process_ptr(x.data_ptr(), n, nr * n, y.data_ptr(), n, n))
    finite = bool(torch.isfinite(torch.view_as_real(y)).all().item())
    # one receiver of one group against the sum made here, as a check that the timed call is the real one
    want = sum(complex(div.get(0)["irotate"][i], div.get(0)["qrotate"][i]) * x[0, i, :8].cpu().numpy() for i in range(nr))
    close = bool(np.allclose(y[0, :8].cpu().numpy(), want, rtol=1e-12, atol=1e-12))
    div.close()
    half = bytes_alg // 2
    src = torch.empty(half, dtype=torch.uint8, device=dev)
    dst = torch.empty(half, dtype=torch.uint8, device=dev)
    src.copy_(torch.view_as_real(x).reshape(-1).view(torch.uint8)[:half])         # (random data, like the kernel's)
    torch.cuda.synchronize(dev)

    def copy():
        if rt.hipMemcpyAsync(dst.data_ptr(), src.data_ptr(), half, D2D, stream.cuda_stream) != 0:
            raise RuntimeError("hipMemcpyAsync failed")
    cms, cms_all = windows(torch, stream, copy)
    torch.cuda.synchronize(dev)
    return {"ngroups": ngroups, "nr": nr, "n": n, "algorithmic_bytes": bytes_alg, "ms_per_call": ms, "ms_per_call_windows": ms_all,
            "GB_per_s": bytes_alg / ms / 1e6, "copy_bytes_read_plus_written": 2 * half, "copy_ms": cms, "copy_ms_windows": cms_all,
            "copy_GB_per_s": 2 * half / cms / 1e6, "time_over_copy": ms / cms, "finite": finite, "matches_a_host_sum": close}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "div_bank.json"))
    a = ap.parse_args()
    import torch
    import quisk_amd as qh
    qh.load()
    rt = hip_runtime()
    res = {"shapes": [run_shape(torch, qh, rt, *s) for s in SHAPES],
           "source": "tools/bench_div.py: device events around %d calls behind %d warm-up calls, median of %d windows; the copy is a hipMemcpyAsync "
                     "device-to-device of half the algorithmic bytes (as many bytes moved), same run, same stream" % (CALLS, WARMUP, WINDOWS)}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
