"""Time of WDSP's fixed-ratio resampler bank (qh_resample.hip) at the shape of an audio back end behind a many-channel receiver: 256
channels, 65 536 input samples per channel and call, complex fp64 at 48 k -> 44.1 k, 44.1 k -> 48 k, 192 k -> 48 k and 48 k -> 96 k, and
real floats at 48 k -> 44.1 k.

    python tools/bench_resample.py [--out profiles/resample_bank.json]

Every shape is timed three ways, taken in turn three times in one process:
  bank   qh_resample_process;
  rat    qh_rat_process (qh_polyphase.hip) on the same taps and ratio -- the only way to run such a ratio before the bank; complex only;
  copy   a device-to-device copy of as many bytes as the bank reads and writes (input rows + output rows).
A turn of a leg is device events around CALLS calls on one stream behind WARMUP calls.  Per leg the JSON holds the three turns, their
median and their spread (max - min); per shape whether the bank's median stays within rat's plus the larger spread, and the ratio.
Where the first tile shape of a design is a choice (L >= 16), the bank is also timed with the other choices (QH_RESAMPLE_G).
Arithmetic per output sample: cpp fused multiply-adds per component, 4 cpp flop complex and 2 cpp flop real."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

NCH, N = 256, 65536
SHAPES = [("c64", 48000, 44100), ("c64", 44100, 48000), ("c64", 192000, 48000), ("c64", 48000, 96000), ("r32", 48000, 44100)]
WARMUP, CALLS, TURNS = 3, 20, 3
G_CHOICES = (2, 4, 8, 16)


def timed(stream, call):
    import torch
    for _ in range(WARMUP):
        call()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(stream)
    for _ in range(CALLS):
        call()
    e1.record(stream)
    e1.synchronize()
    return e0.elapsed_time(e1) / CALLS


def leg(turns):
    s = sorted(turns)
    return {"ms_per_call_turns": turns, "ms_per_call": s[len(s) // 2], "spread_ms": s[-1] - s[0]}


def shape(dtype, in_rate, out_rate, n=N, nch=NCH):
    import numpy as np
    import torch
    import quisk_amd as qh
    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev)
    g.manual_seed(1)
    cplx = dtype == "c64"
    if cplx:
        x = torch.view_as_complex(torch.randn((nch, n, 2), generator=g, device=dev, dtype=torch.float64).contiguous())
    else:
        x = torch.randn((nch, n), generator=g, device=dev, dtype=torch.float32)
    tdt, es = (torch.complex128, 16) if cplx else (torch.float32, 4)
    stream = torch.cuda.Stream(dev)
    torch.cuda.synchronize(dev)

    def bank_with(G):
        if G is None:
            os.environ.pop("QH_RESAMPLE_G", None)
        else:
            os.environ["QH_RESAMPLE_G"] = str(G)
        b = qh.WdspResampler(nch, in_rate, out_rate, dtype=dtype, stream=stream.cuda_stream)
        os.environ.pop("QH_RESAMPLE_G", None)
        return b

    bank = bank_with(None)
    L, M, cpp = bank.L(), bank.M(), bank.cpp()
    mo = bank.max_out(n)
    y = torch.zeros((nch, mo), dtype=tdt, device=dev)
    legs = {"bank": lambda: bank.process_ptr(x.data_ptr(), n, y.data_ptr(), mo, n)}
    out_per_call = int(bank.out_count(n))
    res = {"dtype": dtype, "in_rate": in_rate, "out_rate": out_rate, "L": L, "M": M, "cpp": cpp, "outputs_per_channel_and_call": out_per_call}
    rat = yr = None
    if cplx:
        nat = np.ascontiguousarray(bank.taps().T).reshape(-1) / L        # time order; qh_rat multiplies by interp
        rat = qh.RationalFir(nch, nat, L, M, stream=stream.cuda_stream)
        yr = torch.zeros((nch, mo + 1), dtype=tdt, device=dev)
        legs["rat"] = lambda: rat.process_ptr(x.data_ptr(), n, n, yr.data_ptr(), mo + 1)
    nbytes = nch * (n + out_per_call) * es
    src = torch.zeros(nbytes, dtype=torch.uint8, device=dev)
    dst = torch.zeros(nbytes, dtype=torch.uint8, device=dev)

    def copy():
        with torch.cuda.stream(stream):
            dst.copy_(src, non_blocking=True)

    legs["copy"] = copy
    variants = {}
    if L >= 16:
        for G in G_CHOICES:
            vb = bank_with(G)
            variants[G] = vb
            legs["bank_G%d" % G] = (lambda vb=vb: vb.process_ptr(x.data_ptr(), n, y.data_ptr(), mo, n))
    torch.cuda.synchronize(dev)
    turns = {k: [] for k in legs}
    for _ in range(TURNS):
        for k, call in legs.items():
            turns[k].append(timed(stream, call))
    torch.cuda.synchronize(dev)
    res["legs"] = {k: leg(v) for k, v in turns.items()}
    res["copy_bytes"] = nbytes
    b = res["legs"]["bank"]
    res["bank_Gsamples_out_per_s"] = nch * out_per_call / b["ms_per_call"] / 1e6
    res["bank_GFLOP_per_s"] = (4 if cplx else 2) * cpp * nch * out_per_call / b["ms_per_call"] / 1e6
    if cplx:
        # the same stream through both: the first call of a fresh pair, so that the phases agree
        b2, r2 = bank_with(None), qh.RationalFir(nch, nat, L, M, stream=stream.cuda_stream)
        y.zero_(); yr.zero_()
        torch.cuda.synchronize(dev)
        c = b2.process_ptr(x.data_ptr(), n, y.data_ptr(), mo, n)
        nr = r2.process_ptr(x.data_ptr(), n, n, yr.data_ptr(), mo + 1)
        torch.cuda.synchronize(dev)
        k = int(min(c.min(), nr))
        res["rat_count"], res["bank_count"] = int(nr), int(c[0])
        res["max_abs_diff_bank_rat"] = float((y[:, :k] - yr[:, :k]).abs().max().item())
        res["max_abs_bank"] = float(y[:, :k].abs().max().item())
        r = res["legs"]["rat"]
        spread = max(b["spread_ms"], r["spread_ms"])
        res["rat_over_bank"] = r["ms_per_call"] / b["ms_per_call"]
        res["bank_not_above_rat_by_more_than_the_spread"] = bool(b["ms_per_call"] <= r["ms_per_call"] + spread)
        b2.close(); r2.close(); rat.close()
    res["finite"] = bool(torch.isfinite(torch.view_as_real(y) if cplx else y).all().item())
    for vb in variants.values():
        vb.close()
    bank.close()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "resample_bank.json"))
    a = ap.parse_args()
    res = {"shape": {"nch": NCH, "n_per_call": N, "warmup_calls": WARMUP, "calls_per_turn": CALLS, "turns": TURNS},
           "shapes": [shape(*s) for s in SHAPES],
           "source": "tools/bench_resample.py: device events around %d calls behind %d warm-up calls; the legs of a shape taken in turn %d times in one "
                     "process; median and spread (max - min) of the turns" % (CALLS, WARMUP, TURNS)}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
