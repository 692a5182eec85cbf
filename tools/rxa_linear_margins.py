"""How far inside its per-sample bound the engine's linear RXA chain runs, case by case and tile form by tile form.

    python tools/rxa_linear_margins.py [--out profiles/rxa_linear_margins.json]

Runs every case of tests/test_gpu_rxa_linear_forms.py once on the GPU and writes, for every case and form: E (the largest per-sample
error of the float64 overlap-save model, tests/rxa_linear_ref.py chain_model64) over rms(want), the kernel's largest error over E and
over the bound, where that sample sits (channel, index, distance to the nearest tile start, call start and retune, in output samples)
and, once per case, how far oracle.WdspChannel.xrxa is from the long-double form at its worst sample of channel 0, over rms(want).
The bounds are the tests' own; nothing here decides a tolerance."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "rxa_linear_margins.json"))
    args = ap.parse_args()
    try:
        import torch  # noqa: F401  -- before libquiskhip: one HIP runtime per process (quisk_amd/lib.py)
    except ImportError:
        pass
    import numpy as np
    import quisk_amd as qh
    import rxa_linear_ref as R
    import test_gpu_rxa_linear_forms as T
    from oracle import pyoracle

    qh.load()
    pyoracle.build()
    res = {"what": "per case and form of tests/test_gpu_rxa_linear_forms.py: E over rms(want) (the largest over the channels), the "
                   "kernel's largest |got - want| over E and over the per-sample bound 16 E + 2 pi 2^-64 n_in |want|, and that "
                   "sample's distance to the nearest tile start, call start and retune, in output samples; oracle_over_rms: "
                   "oracle.WdspChannel.xrxa against the long-double form at its worst sample of channel 0",
           "runs": {}}
    oracle_of = {}
    for run in T.RUNS:
        cs, nch, form, meters, replay = run
        rec = R.case_ref(cs, nch, form, meters)
        info = {}
        y = R.run_engine(qh, cs, nch, form, meters, replay, info)
        w = R.margins(y, rec)
        if cs not in oracle_of:
            o, want = R.run_oracle(pyoracle, cs, 0), rec["want"][0]
            oracle_of[cs] = float(max(np.max(np.abs(o.real - want.real)), np.max(np.abs(o.imag - want.imag)))) / rec["rms"][0]
        res["runs"][T.run_id(run)] = {
            "E_over_rms": max(E / r for E, r in zip(rec["E"], rec["rms"])), "kernel_err_over_E": w["err_over_E"],
            "err_over_bound": w["ratio"], "channel": w["channel"], "index": w["index"], "part": w.get("part"),
            "to_tile": w["to_seam"], "to_call": w["to_call"], "to_retune": w["to_retune"], "oracle_over_rms": oracle_of[cs],
            "bound": "max(16 E, TOL64 rms(want))" if T.run_id(run) in T.EXCEPTIONS else "16 E + 2 pi 2^-64 n_in |want|",
            "outputs": int(rec["want"].shape[1]), "calls_in_blocks": list(rec["blocks"]), "graph_launches": info["graph_launches"]}
        print(T.run_id(run), "%.3g of the bound, %.3g E" % (w["ratio"], w["err_over_E"]), flush=True)
    over = [v["kernel_err_over_E"] for v in res["runs"].values()]
    res["range"] = {"kernel_err_over_E": [min(over), max(over)],
                    "err_over_bound_max": max(v["err_over_bound"] for v in res["runs"].values()),
                    "E_over_rms": [min(v["E_over_rms"] for v in res["runs"].values()), max(v["E_over_rms"] for v in res["runs"].values())],
                    "oracle_over_rms": [min(oracle_of.values()), max(oracle_of.values())]}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1, sort_keys=True)
        f.write("\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
