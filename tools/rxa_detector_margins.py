"""How far inside their per-sample bound the engine's AM, SAM and FM detectors run, form by form.

    python tools/rxa_detector_margins.py [--out profiles/rxa_detector_margins.json]

Runs every case of tests/test_gpu_rxa_detector_forms.py once on the GPU and writes, for every case and channel: E (the largest
per-sample error of the float64 model of tests/rxa_detector_ref.py against the long-double chains) and T (what a tile accepted at 1e-12
can do to the chain's output) over rms(want), the kernel's largest error over E and over its bound 16 E (+ T from the first tiled call
on; channels in the tests' EXCEPTIONS are marked, their figures are against the same 16 E), where that sample sits (index behind the switch, distance to the nearest tile or segment start and call start, in output samples),
and once per case the count of tiles the verify pass re-ran.  The bounds are the tests' own; nothing here decides a tolerance."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "rxa_detector_margins.json"))
    args = ap.parse_args()
    try:
        import torch  # noqa: F401  -- before libquiskhip: one HIP runtime per process (quisk_amd/lib.py)
    except ImportError:
        pass
    import quisk_amd as qh
    import rxa_detector_ref as D
    import test_gpu_rxa_detector_forms as T

    qh.load()
    res = {"what": "per case of tests/test_gpu_rxa_detector_forms.py and per channel: E and T over rms(want), the kernel's largest "
                   "|got - want| over E and over the per-sample bound (16 E, + T from the first tiled call on), that sample's index "
                   "behind the switch and its distance to the nearest tile or segment start and call start; per case the tiles the "
                   "verify pass re-ran",
           "runs": {}}
    import time
    for run in T.RUNS:
        name, chans, sched, forms, meters = run
        t0 = time.time()
        if forms is None:
            os.environ.pop("QH_DBG_FORMS", None)
        else:
            os.environ["QH_DBG_FORMS"] = str(forms)             # read when the engine is made
        rec = D.case_ref(tuple(chans), tuple(sched))
        seams, calls = D.detector_seams(chans, sched)
        info = {}
        t1 = time.time()
        y = D.run_engine(qh, chans, sched, meters, info)
        print("    reference %.1f s, engine %.1f s" % (t1 - t0, time.time() - t1), flush=True)
        rows = []
        for c, ch in enumerate(chans):
            one = {k: (v[c:c + 1] if k in ("want", "bound") else [v[c]] if k in ("E", "T", "rms") else v) for k, v in rec.items()}
            w = D.margins(y[c:c + 1], one, seams, calls)
            rows.append({"kind": ch.kind, "E_over_rms": rec["E"][c] / rec["rms"][c], "T_over_rms": rec["T"][c] / rec["rms"][c],
                         "rms": rec["rms"][c], "err_over_bound": w["ratio"], "err_over_E": w["err_over_E"], "index": w["index"],
                         "part": w.get("part"), "to_seam": w["to_seam"], "to_call": w["to_call"],
                         "excepted": bool(T.excepted(name, ch)), "err_over_rms": w["err"] / rec["rms"][c]})
        worst = max(rows, key=lambda r: r["err_over_bound"])
        res["runs"][name] = {"QH_DBG_FORMS": forms, "meters": bool(meters), "calls_in_blocks": list(sched), "pll_repairs": int(info["pll_repairs"]),
                             "err_over_bound_max": worst["err_over_bound"], "channels": rows}
        print(name, "%.3g of the bound (%s), %.3g E; repairs %d"
              % (worst["err_over_bound"], worst["kind"], max(r["err_over_E"] for r in rows), info["pll_repairs"]), flush=True)
        for r in rows:
            print("    %-4s err/bound %.3g  err/E %.3g  index %d  to seam %s  to call %s" % (r["kind"], r["err_over_bound"], r["err_over_E"], r["index"], r["to_seam"], r["to_call"]), flush=True)
    os.environ.pop("QH_DBG_FORMS", None)
    allrows = [r for v in res["runs"].values() for r in v["channels"]]
    res["range"] = {"err_over_bound_max": max(r["err_over_bound"] for r in allrows),
                    "err_over_E": [min(r["err_over_E"] for r in allrows), max(r["err_over_E"] for r in allrows)],
                    "E_over_rms": [min(r["E_over_rms"] for r in allrows), max(r["E_over_rms"] for r in allrows)],
                    "T_over_rms_max": max(r["T_over_rms"] for r in allrows)}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1, sort_keys=True)
        f.write("\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
