"""Time of the RXA chain with the LMS notch (xanf) or EMNR on: nch channels x nblk DSP blocks per call.  The LMS recurrence is
sequential per channel (one wavefront each), so the figure of merit is samples/s per channel and channels in flight.
python tools/lms_bench.py [nch] [nblk] [--taps T[,T...]] [--delay D] [--lms-only]

--taps / --delay: the ANF's settings (default 64 / 16, the one-tap-per-lane form; more than 64 taps or a delay outside 1..64 takes
the long form, lms_long_kernel).  A list of tap counts gives one result line each.  --lms-only leaves the EMNR and SNBA runs out."""
import argparse
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import quisk_amd as qh
from quisk_amd import synth

ap = argparse.ArgumentParser()
ap.add_argument("nch", nargs="?", type=int, default=256)
ap.add_argument("nblk", nargs="?", type=int, default=256)
ap.add_argument("--taps", default="64")
ap.add_argument("--delay", type=int, default=16)
ap.add_argument("--lms-only", action="store_true")
args = ap.parse_args()
nch, nblk = args.nch, args.nblk
dev = torch.device("cuda:0")
x = synth.make_input_torch(nch, nblk * 1024, dev) if hasattr(synth, "make_input_torch") else torch.from_numpy(synth.make_input_numpy(nch, nblk * 1024)).to(dev)
y = torch.empty((nch, nblk * 256), dtype=torch.complex128, device=dev)
# clocks per sample are stated at the device's top engine clock (where torch does not report one: the MI355X's 2400 MHz); the clock a
# kernel really ran at is lower and differs from card to card, so the figure is an upper bound on the cycles, not a count of them
mhz = getattr(torch.cuda.get_device_properties(0), "clock_rate", 2400e3) / 1e3


def run(name, taps=64):
    e = qh.RxaEngine(nch)
    for c in range(nch):
        e.SetRXAMode(c, 1); e.RXASetPassband(c, 300.0, 3000.0); e.SetRXAAGCMode(c, 0)
    if name == "anf":
        if (taps, args.delay) != (64, 16):
            e.SetRXAANFVals(-1, taps, args.delay, 1e-4, 0.1)
        e.SetRXAANFRun(-1, 1)
    if name == "emnr":
        e.load_emnr_tables()
        e.SetRXAEMNRRun(-1, 1)
    if name == "snba":
        e.SetRXASNBARun(-1, 1)
    e.enable_timing(True)
    torch.cuda.synchronize()
    for _ in range(2):
        e.process_ptr(x.data_ptr(), x.shape[1], y.data_ptr(), y.shape[1], nblk)
    e.synchronize()
    t0 = time.perf_counter()
    for _ in range(3):
        e.process_ptr(x.data_ptr(), x.shape[1], y.data_ptr(), y.shape[1], nblk)
    e.synchronize()
    ms = (time.perf_counter() - t0) / 3 * 1e3
    e.close()
    return ms


mid = nblk * 256
res = {"plain": run("plain")}
for taps in [int(t) for t in args.taps.split(",")]:
    res["anf"] = run("anf", taps)
    lms_ms = res["anf"] - res["plain"]
    out = {"nch": nch, "nblk": nblk, "taps": taps, "delay": args.delay, "ms_plain": round(res["plain"], 3), "ms_with_anf": round(res["anf"], 3),
           "lms_and_bp1_ms": round(lms_ms, 3),
           "lms_Msamp_per_s_per_channel": round(mid / lms_ms / 1e3, 3),
           "lms_x_realtime_at_48k": round(mid / lms_ms * 1e3 / 48000.0, 1),
           "lms_clocks_per_sample_at_%d_MHz" % round(mhz): round(lms_ms * 1e-3 * mhz * 1e6 / mid),
           "chain_Gsamp_per_s_with_anf": round(nch * nblk * 1024 / res["anf"] / 1e6, 2)}
    if not args.lms_only and "emnr" not in res:
        res["emnr"], res["snba"] = run("emnr"), run("snba")
    if not args.lms_only:
        out.update({"ms_with_emnr": round(res["emnr"], 3), "emnr_and_bp1_ms": round(res["emnr"] - res["plain"], 3),
                    "emnr_frames_per_s": round(nch * nblk / 4 / (res["emnr"] - res["plain"]) * 1e3, 0),
                    "chain_Gsamp_per_s_with_emnr": round(nch * nblk * 1024 / res["emnr"] / 1e6, 2),
                    "ms_with_snba": round(res["snba"], 3), "snba_bpsnba_bp1_ms": round(res["snba"] - res["plain"], 3),
                    "snba_frames_per_s": round(nch * nblk / (res["snba"] - res["plain"]) * 1e3, 0),
                    "snba_x_realtime_per_channel": round(nblk * 256 / 48000.0 / ((res["snba"] - res["plain"]) * 1e-3), 1),
                    "chain_Gsamp_per_s_with_snba": round(nch * nblk * 1024 / res["snba"] / 1e6, 2)})
    print(json.dumps(out), flush=True)
