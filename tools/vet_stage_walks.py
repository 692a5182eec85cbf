#!/usr/bin/env python3
"""Vet the seeds of tests/test_gpu_rxa_fuzz_stages.py on the CPU (no GPU needed): per seed, the composed reference's margins (squelch
threshold crossings, tail counts), each channel's reference against its twin fed 1e-13 relative noise, which of the new stages ran, and
how many close/open cycles each squelch made.  A seed is rejected when a margin fails (a crossing closer than 1e-6, a tail count closer
than 1e-3 to an integer) or a twin distance exceeds a tenth of the channel's tolerance.  Prints REJECTED, TABLE and SHARES in the form the
test file holds them, and compares with what it holds.

    python tools/vet_stage_walks.py [--jobs N] [--family plain|replay|wide] [seed ...]
"""
import argparse
import os
import sys
from multiprocessing import Pool

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]


def vet(job):
    family, seed = job
    import numpy as np
    import test_gpu_rxa_fuzz_stages as T
    w = T.walk(seed, family, twin=True)
    why = []
    for c, r in enumerate(w["refs"]):
        if not r.margins_ok():
            why.append("channel %d margins %s" % (c, ", ".join("%s %.1e" % kv for kv in r.margins().items() if np.isfinite(kv[1]))))
        if w["twin_dist"][c] > 0.1 * w["tol"][c]:
            why.append("channel %d twin %.1e against tolerance %.0e" % (c, w["twin_dist"][c], w["tol"][c]))
    margins = {k: min(r.margins()[k] for r in w["refs"]) for k in w["refs"][0].margins()}
    return family, seed, T.facts(w), why, margins, w["twin_dist"], w["tol"], w["nblk"]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--jobs", type=int, default=min(8, os.cpu_count() or 1))
    ap.add_argument("--family")
    ap.add_argument("seeds", nargs="*", type=int)
    a = ap.parse_args()
    import test_gpu_rxa_fuzz_stages as T
    jobs = [(f, s) for f, t in T.TRIED.items() for s in t if (not a.family or f == a.family) and (not a.seeds or s in a.seeds)]
    with Pool(a.jobs) as pool:
        res = pool.map(vet, jobs, chunksize=1)
    table, rejected = {}, {}
    for family, seed, facts, why, margins, twin, tol, nblk in res:
        print("%-6s %6d (%3d blocks): margins %s\n    twin %s of tolerance %s\n    ran %s; SSQL cycles %r, FMSQ cycles %d; two stages live on channels %r%s" % (
            family, seed, nblk, ", ".join("%s %.1e" % kv for kv in margins.items()), ["%.1e" % v for v in twin], ["%.0e" % v for v in tol],
            "+".join(facts[0]) or "none", facts[1], facts[2], facts[3], "\n    REJECTED: " + "; ".join(why) if why else ""))
        if why:
            rejected[seed] = "; ".join(why)
        else:
            table[seed] = facts
    n = len(table)
    shares = {st: sum(st in f[0] for f in table.values()) for st in T.STAGES}
    shares.update(ssql_cycle=sum(any(f[1]) for f in table.values()), fmsq_cycle=sum(f[2] > 0 for f in table.values()),
                  two_live=sum(bool(f[3]) for f in table.values()), walks=n, tried=len(res), replaced=len(rejected))
    print("\nREJECTED = {")
    for s, w in sorted(rejected.items()):
        print("    %d: %r," % (s, w))
    print("}\nTABLE = {")
    for s, f in sorted(table.items()):
        print("    %d: %r," % (s, f))
    print("}\nSHARES = %r" % (shares,))
    if not a.seeds and not a.family:
        same = table == T.TABLE and set(rejected) == set(T.REJECTED) and shares == T.SHARES
        print("\nthe test file holds %s" % ("the same" if same else "something else: update REJECTED, TABLE and SHARES there"))
        return 0 if same else 1
    return 0


if __name__ == "__main__":
    sys.exit(main())
