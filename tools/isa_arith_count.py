#!/usr/bin/env python3
"""Static fp64 arithmetic census of kernels of qh_engine.hip, from a gfx950 cross-compile (no GPU needed).

    tools/isa_arith_count.py [--asm FILE.s] [--keep FILE.s] [--json] PATTERN [PATTERN ...]

Every PATTERN is a regular expression searched in the demangled kernel names, e.g.
    'osfir_kernel<double, 4096, 1, false, false, false, false, false, false, 0, false, false>'   the band tile, meters off
    'osfir_kernel<double, 4096, 4, .*true, 0, false, false>'                                     front tiles of fold 4 (POLY)
For each kernel that matches: v_add_f64, v_mul_f64 and v_fma_f64 + v_fmac_f64 instructions in its code (static: both sides of
a branch count), all VALU instructions, and the VGPRs, scratch bytes and code length the compiler reports beside the code.
Without --asm the unit is compiled with the flags of quisk_amd/build.py (-O3 -std=c++17) to assembly first, which takes minutes.
"""
import argparse
import collections
import json
import os
import re
import shutil
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def compile_asm(out, source="qh_engine.hip"):
    from quisk_amd import build as qbuild
    cmd = [qbuild._hipcc(), "--offload-arch=gfx950", "-O3", "-std=c++17", "-x", "hip", "--cuda-device-only", "-S",
           source if os.path.exists(source) else os.path.join(qbuild.CSRC, source), "-o", out]
    subprocess.run(cmd, check=True)
    return out


def demangle(names):
    for tool in ("/opt/rocm/llvm/bin/llvm-cxxfilt", shutil.which("llvm-cxxfilt"), shutil.which("c++filt")):
        if tool and os.path.exists(tool):
            out = subprocess.run([tool], input="\n".join(names) + "\n", capture_output=True, text=True, check=True).stdout.split("\n")
            return dict(zip(names, out))
    return {n: n for n in names}


def kernels(asm_text):
    """{mangled name: (instruction mnemonics, {NumVgprs, ScratchSize, codeLenInByte, Occupancy})} of every kernel (.amdhsa_kernel)."""
    names = re.findall(r"^\s*\.amdhsa_kernel\s+(\S+)", asm_text, re.M)
    res = {}
    for name in names:
        m = re.search(r"^%s:.*?$" % re.escape(name), asm_text, re.M)
        end = asm_text.find("\n.Lfunc_end", m.end())
        ins = []
        for line in asm_text[m.end():end].split("\n"):
            t = line.strip()
            if not line.startswith("\t") or not t or t[0] in ".;":
                continue
            ins.append(t.split()[0])
        tail = asm_text[end:asm_text.find(".amdhsa_kernel", end)]
        info = {}
        for key in ("NumVgprs", "ScratchSize", "codeLenInByte", "Occupancy"):
            k = re.search(r";\s*%s:?\s*=?\s*(\d+)" % key, tail)
            info[key] = int(k.group(1)) if k else None
        res[name] = (ins, info)
    return res


def census(ins):
    c = collections.Counter(re.sub(r"_e(32|64)$", "", i) for i in ins)      # v_fmac_f64_e32 and v_fmac_f64_e64 are one instruction
    row = {"v_add_f64": c["v_add_f64"], "v_mul_f64": c["v_mul_f64"], "v_fma_f64": c["v_fma_f64"] + c["v_fmac_f64"]}
    row["fp64"] = row["v_add_f64"] + row["v_mul_f64"] + row["v_fma_f64"]
    row["valu"] = sum(v for k, v in c.items() if k.startswith("v_"))
    return row


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("patterns", nargs="+")
    ap.add_argument("--asm", help="assembly made earlier (hipcc --cuda-device-only -S)")
    ap.add_argument("--keep", help="keep the assembly this run compiles in this file")
    ap.add_argument("--source", default="qh_engine.hip", help="a unit of quisk_amd/csrc, or a path (tools/ubench/dft16_count.hip)")
    ap.add_argument("--json", action="store_true")
    a = ap.parse_args()
    if a.asm:
        text = open(a.asm).read()
    else:
        with tempfile.TemporaryDirectory() as d:
            path = a.keep or os.path.join(d, "unit.s")
            text = open(compile_asm(path, a.source)).read()
    ks = kernels(text)
    dem = demangle(list(ks))
    rows, missed = [], 0
    for pat in a.patterns:
        hits = [n for n in ks if re.search(pat, dem[n])]
        if not hits:
            print("no kernel matches %r" % pat, file=sys.stderr)
            missed = 1
        for n in hits:
            ins, info = ks[n]
            rows.append(dict(kernel=dem[n], **census(ins), vgprs=info["NumVgprs"], scratch_bytes=info["ScratchSize"],
                             code_bytes=info["codeLenInByte"], occupancy=info["Occupancy"]))
    if a.json:
        print(json.dumps(rows, indent=1))
    else:
        for r in rows:
            print(r["kernel"])
            print("  v_add_f64 %d  v_mul_f64 %d  v_fma/fmac_f64 %d  fp64 total %d  VALU %d  VGPRs %s  scratch %s B  code %s B  waves/SIMD %s" % (
                r["v_add_f64"], r["v_mul_f64"], r["v_fma_f64"], r["fp64"], r["valu"], r["vgprs"], r["scratch_bytes"], r["code_bytes"],
                r["occupancy"]))
    return missed


if __name__ == "__main__":
    sys.exit(main())
