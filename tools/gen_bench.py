"""What gen0 costs at one GPU's share of BASELINE config 2 (256 channels, USB, 2^20 dsp samples per channel and call, fp64: bench.py's
settings).  One process, the cases in turn on one engine: no generator running (the linear path, what the parent commit runs: the A/B
case), the per-mode path forced by a siphon tap with no generator running, then gen0 running in every channel in modes 0, 1, 2, 3, 6
and 99 with the same tap on.  Per case the wall time of each of `steps` calls and the engine's own event timing (qh_rxa_enable_timing:
front / band / rest, ms) of one call.  One JSON line.

The generating kernel's own time does not come out of those (the signal it writes changes what the stages behind it cost): run this
program under `rocprofv3 --kernel-trace --output-format csv` and hand the kernel trace to `gen_bench.py --trace <kernel_trace.csv>`,
which prints gen_kernel's time per mode (every case launches it ten times, in the order above; the median of the last eight) and its
share of the HBM roofline at 16 B per sample stored against bench.py's 8 TB/s."""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
HBM_PEAK_GBPS = 8000.0          # bench.py's


MODES = ((0, "tone"), (1, "two-tone"), (2, "noise"), (3, "sweep (defaults)"), (6, "pulse"), (99, "silence"))
PER_CASE = 10                   # launches of gen_kernel per case: 2 warm-up calls, `steps` = 5, 3 with event timing


def trace(path, nch=256, n=1 << 20):
    import csv
    rows = [r for r in csv.DictReader(open(path)) if "gen_kernel" in r["Kernel_Name"]]
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    assert len(rows) == PER_CASE * len(MODES), len(rows)
    out = []
    for k, (mode, name) in enumerate(MODES):
        ms = sorted((int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e6 for r in rows[k * PER_CASE + 2:(k + 1) * PER_CASE])
        med = 0.5 * (ms[3] + ms[4])
        gbps = nch * n * 16 / (med * 1e-3) / 1e9
        out.append({"mode": mode, "name": name, "gen_kernel_ms": round(med, 4), "min_ms": round(ms[0], 4), "max_ms": round(ms[-1], 4),
                    "store_gbps": round(gbps, 1), "hbm_roofline_share": round(gbps / HBM_PEAK_GBPS, 3)})
    print(json.dumps({"gen_kernel": out}))


def main():
    if len(sys.argv) > 2 and sys.argv[1] == "--trace":
        return trace(sys.argv[2])
    import torch
    import quisk_amd as qh
    from quisk_amd import synth
    nch, nblk = int(os.environ.get("QH_GEN_NCH", "256")), int(os.environ.get("QH_GEN_NBLK", "4096"))
    steps = 5
    dev = torch.device("cuda:0")
    n_in, n_out = nblk * 1024, nblk * 256
    e = qh.RxaEngine(nch)
    e.SetRXAShiftRun(-1, 1)
    for c in range(nch):
        e.SetRXAShiftFreq(c, synth.shift_freq(c))
    e.RXANBPSetRun(-1, 1); e.SetRXAMode(-1, 1); e.RXASetPassband(-1, 300.0, 3000.0)
    e.SetRXAAGCMode(-1, 0); e.SetRXAAGCFixed(-1, 0.0)
    x = synth.make_input_torch(nch, n_in, dev, fs=192000.0)
    y = torch.empty((nch, n_out), dtype=torch.complex128, device=dev)

    def sync():
        e.synchronize()
        torch.cuda.synchronize(dev)

    def case(name):
        step = lambda: e.process_ptr(x.data_ptr(), n_in, y.data_ptr(), n_out, nblk)
        for _ in range(2):
            step()
        sync()
        walls = []
        for _ in range(steps):
            t0 = time.perf_counter()
            step()
            sync()
            walls.append(round((time.perf_counter() - t0) * 1e3, 3))
        e.enable_timing(True)
        evs = []
        for _ in range(3):
            step()
            evs.append(e.timing_ms())
        e.enable_timing(False)
        sync()
        ev = sorted(evs, key=lambda v: v[0])[1]                 # the median first segment of three
        return {"case": name, "wall_ms_per_call": walls, "event_ms": [round(v, 3) for v in ev], "device_bytes": e.device_bytes()}

    out = [case("no generator running (linear path)")]
    e.set_siphon(-1, 1)
    out.append(case("no generator running, siphon on (per-mode path)"))
    e.SetRXAPreGenRun(-1, 1)
    for mode, name in MODES:
        e.SetRXAPreGenMode(-1, mode)
        out.append(case("gen0 mode %d (%s) in every channel, siphon on" % (mode, name)))
    print(json.dumps({"config": "2 (one GPU's share): %d ch x 192 k, %d blocks a call" % (nch, nblk), "cases": out}))
    e.close()


if __name__ == "__main__":
    main()
