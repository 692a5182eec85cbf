"""What distinct FM filter designs cost an RXA engine: 256 FM channels, 65 536 samples per channel and call (dsp_size 64, 48 k / 48 k /
48 k, AGC mode 0), with 1, 2, 16 and 256 distinct audio bands among the channels (SetRXAFMAFFilter), channel c taking band c mod R so
that every design has 256 / R channels and pairs form wherever two channels share one.

    python tools/bench_fm_filters.py [--out profiles/fm_filters_bank.json]

Every design count runs in a process of its own under a time limit (a child that faults or hangs ends the run).  Per count the JSON
holds: the wall time of the first process call, which designs the rows on the host; the time per call (wall clock around CALLS
synchronised calls behind WARMUP calls, three turns, median and spread); the engine's own stage times of one call (qh_rxa_timing: front,
the fircore tiles of all stages together, everything else -- the engine does not time its kernels one by one); the design rows on the
device and the device bytes.  A last run has one design and ONE channel with a minimum-phase de-emphasis filter (SetRXAFMMPde): its
complex taps switch the paired tile, and the dc removal fused into it, off for the whole stage -- what that costs the other 255."""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

NCH, N, SIZE, RATE = 256, 65536, 64, 48000
DESIGNS = (1, 2, 16, 256)
WARMUP, CALLS, TURNS = 2, 8, 3
LIMIT_S = 240


def child(R, mp_one=False):
    import numpy as np
    import torch
    import quisk_amd as qh
    dev = torch.device("cuda:0")
    e = qh.RxaEngine(NCH, dsp_size=SIZE, in_rate=RATE, dsp_rate=RATE, out_rate=RATE)
    e.SetRXAMode(-1, 5)
    e.RXASetPassband(-1, -8000.0, 8000.0)
    e.SetRXAAGCMode(-1, 0)
    e.SetRXAAGCFixed(-1, 0.0)
    for c in range(NCH):
        r = c % R
        e.SetRXAFMAFFilter(c, 300.0 - 0.5 * r, 3000.0 + 4.0 * r)
    if mp_one:
        e.SetRXAFMMPde(0, 1)
    t = np.arange(N) / RATE
    ph = 2.0 * np.pi * np.cumsum(3000.0 * np.sin(2.0 * np.pi * 1000.0 * t)) / RATE
    x = torch.from_numpy(np.ascontiguousarray(np.broadcast_to(0.3 * np.exp(1j * ph), (NCH, N)))).to(dev)
    y = torch.zeros((NCH, N), dtype=torch.complex128, device=dev)
    nblk = N // SIZE
    torch.cuda.synchronize(dev)

    def call():
        e.process_ptr(x.data_ptr(), N, y.data_ptr(), N, nblk)

    t0 = time.perf_counter()
    call()
    e.synchronize()
    first = time.perf_counter() - t0
    t0 = time.perf_counter()
    call()
    e.synchronize()
    second = time.perf_counter() - t0
    turns = []
    for _ in range(TURNS):
        for _ in range(WARMUP):
            call()
        e.synchronize()
        t0 = time.perf_counter()
        for _ in range(CALLS):
            call()
        e.synchronize()
        turns.append((time.perf_counter() - t0) * 1e3 / CALLS)
    e.enable_timing(True)
    call()
    e.synchronize()
    stages = e.timing_ms()
    e.enable_timing(False)
    rows = e.debug_fm_rows()
    s = sorted(turns)
    res = {"designs": R, "one_minimum_phase_channel": bool(mp_one), "first_call_wall_ms": first * 1e3, "second_call_wall_ms": second * 1e3, "host_design_ms": (first - second) * 1e3,
           "ms_per_call_turns": turns, "ms_per_call": s[len(s) // 2], "spread_ms": s[-1] - s[0],
           "stage_ms_front_tiles_rest": stages, "de_rows": rows[0], "aud_rows": rows[1], "rows_designed": rows[2],
           "device_bytes": e.device_bytes(), "finite": bool(torch.isfinite(torch.view_as_real(y)).all().item())}
    e.close()
    print("RESULT " + json.dumps(res))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fm_filters_bank.json"))
    ap.add_argument("--child", type=int, default=0)
    ap.add_argument("--mp-one", action="store_true")
    a = ap.parse_args()
    if a.child:
        child(a.child, a.mp_one)
        return
    runs = []
    for R, mp in [(R, False) for R in DESIGNS] + [(1, True)]:
        p = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", str(R)] + (["--mp-one"] if mp else []), capture_output=True, text=True,
                           timeout=LIMIT_S)
        if p.returncode != 0:
            sys.stderr.write(p.stdout[-2000:] + p.stderr[-2000:])
            raise SystemExit("designs %d: the child ended with status %d; nothing more is started" % (R, p.returncode))
        runs.append(json.loads([ln for ln in p.stdout.splitlines() if ln.startswith("RESULT ")][-1][7:]))
    base = runs[0]["ms_per_call"]
    for r in runs:
        r["over_one_design"] = r["ms_per_call"] / base
    res = {"shape": {"nch": NCH, "n_per_call": N, "dsp_size": SIZE, "rate": RATE, "warmup_calls": WARMUP, "calls_per_turn": CALLS, "turns": TURNS},
           "runs": runs,
           "source": "tools/bench_fm_filters.py: wall clock around %d synchronised calls behind %d warm-up calls, %d turns, median and spread "
                     "(max - min); one process per design count" % (CALLS, WARMUP, TURNS)}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
