"""How far inside their per-sample bounds the three stand-alone filter banks run, case by case.

    python tools/filter_forms_margins.py [--out profiles/filter_forms_margins.json]

Runs every case of tests/test_gpu_fir_forms.py, tests/test_gpu_polyphase_forms.py and tests/test_gpu_hbcascade_forms.py once per sample
type on the GPU and writes, for every case and type: the largest error over bound, where that sample sits (channel, index, distance to
the nearest tile / block / segment start and to the nearest call boundary) and, for FirBank in fp32, E (the largest per-sample error of
the complex64 overlap-save model, tests/filter_forms_ref.py os_model) and the kernel's own largest error, both over rms(want).  The
bounds are the tests' own; nothing here decides a tolerance."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def entry(w, **more):
    e = {"err_over_bound": w["ratio"], "channel": w["channel"], "index": w["index"], "part": w.get("part"),
         "to_seam": w["to_seam"], "to_call": w["to_call"]}
    e.update(more)
    return e


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "filter_forms_margins.json"))
    args = ap.parse_args()
    try:
        import torch  # noqa: F401  -- before libquiskhip: one HIP runtime per process (quisk_amd/lib.py)
    except ImportError:
        pass
    import numpy as np
    import quisk_amd as qh
    import filter_forms_ref as R
    import test_gpu_fir_forms as tf
    import test_gpu_hbcascade_forms as th
    import test_gpu_polyphase_forms as tp

    qh.load()
    types = ((R.F64, "f64"), (R.F32, "f32"))
    res = {"what": "largest |got - want| over the per-sample bound of the tests, per case and sample type; to_seam / to_call: distance "
                   "of that sample to the nearest tile (FirBank), 256-output block (RationalFir) or segment (HalfBandCascade) start and "
                   "to the nearest call boundary, in output samples",
           "fir": {}, "polyphase": {}, "hbcascade": {}}
    for case in tf.CASES:
        for dtype, tname in types:
            for kind in ("noise", "impulses"):
                rec = R.fir_case(case, kind, dtype)
                y, _ = R.run_calls(qh.FirBank(3, rec["taps"], case[1], dtype=dtype), rec["x"], rec["sizes"])
                bound = tf.bound_of(case, kind, dtype, rec)
                e = entry(R.worst_sample(y, rec["want"], bound, rec["tiles"], rec["calls"]),
                          geometry=dict(zip(("fold", "pick", "P", "Lf", "per_tile"), rec["geometry"])), samples=int(rec["x"].shape[1]))
                if dtype == R.F32:
                    g = y.astype(np.complex128)
                    worst = float(np.max(np.maximum(np.abs(g.real - rec["want"].real), np.abs(g.imag - rec["want"].imag))))
                    e.update(E_over_rms=rec["E"] / rec["rms"], kernel_err_over_rms=worst / rec["rms"], kernel_err_over_E=worst / rec["E"],
                             bound="TOL32 rms(want)" if (case, kind) in tf.F32_EXCEPTIONS else "16 E")
                res["fir"]["%s %s %s" % (R.fir_case_id(case), tname, kind)] = e
                print("fir", R.fir_case_id(case), tname, kind, "%.3g" % e["err_over_bound"], flush=True)
    for case in tp.CASES:
        for dtype, tname in types:
            rec = R.rat_case(case, dtype)
            y, _ = R.run_calls(qh.RationalFir(3, rec["taps"], case[0], case[1], dtype=dtype), rec["x"], rec["sizes"])
            e = entry(R.worst_sample(y, rec["want"], rec["bound"], rec["blocks"], rec["calls"]), K=rec["K"])
            res["polyphase"]["%s %s" % (R.rat_case_id(case), tname)] = e
            print("polyphase", R.rat_case_id(case), tname, "%.3g" % e["err_over_bound"], flush=True)
    for case in th.CASES:
        for dtype, tname in types:
            rec = R.hbc_case(case[0], dtype, case[1])
            y, _ = R.run_calls(qh.HalfBandCascade(rec["nch"], case[0], dtype=dtype), rec["x"], rec["sizes"])
            e = entry(R.worst_sample(y, rec["want"], rec["B"], rec["segs"], rec["calls"]),
                      B_over_rms=float(np.median(np.concatenate([rec["B"].real, rec["B"].imag], axis=None))) / rec["rms"])
            if dtype == R.F64:
                e["err_over_TOL64_rms"] = R.worst_sample(y, rec["want"], R.TOL64 * rec["rms"], rec["segs"], rec["calls"])["ratio"]
            res["hbcascade"]["%s %s" % (th.hbc_case_id(case), tname)] = e
            print("hbcascade", th.hbc_case_id(case), tname, "%.3g" % e["err_over_bound"], flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1, sort_keys=True)
        f.write("\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
