"""Builds quisk_amd/lib/libquiskhip.so with hipcc for gfx950 (cross-compiles without a GPU)."""
import os
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "csrc")
LIBDIR = os.path.join(HERE, "lib")
LIB = os.path.join(LIBDIR, "libquiskhip.so")
SOURCES = ["qh_engine.hip", "qh_engine_params.hip", "qh_rxa_api.hip", "qh_fir.hip", "qh_pan.hip", "qh_qrx.hip", "qh_hbcascade.hip", "qh_polyphase.hip", "qh_ingest.hip", "qh_qagc.hip", "qh_nb.hip", "qh_anb.hip", "qh_nob.hip", "qh_varsamp.hip", "qh_resample.hip", "qh_div.hip", "qh_analyzer.hip", "qh_wdsp_compat.cpp", "qh_wdsp_ext.cpp", "qh_quisk_compat.cpp", "qh_quisk_rx_compat.cpp", "qh_qps.hip", "qh_design.cpp"]
HEADERS = sorted(f for f in os.listdir(CSRC) if f.endswith((".hpp", ".h"))) + [os.path.join("..", "..", "include", "quiskhip.h")]


def _hipcc():
    for c in (os.environ.get("HIPCC"), "/opt/rocm/bin/hipcc", "hipcc"):
        if c and (os.path.isabs(c) and os.path.exists(c) or not os.path.isabs(c)):
            return c
    raise RuntimeError("hipcc not found")


def needs_build():
    if not os.path.exists(LIB):
        return True
    t = os.path.getmtime(LIB)
    return any(os.path.getmtime(os.path.join(CSRC, f)) > t for f in SOURCES + HEADERS) or os.path.getmtime(EMNR_NPZ) > t


def _export_map(path, extra=()):
    """Linker version script: the C ABI of include/quiskhip.h and nothing else.  The library is loaded into other programs' processes
    (Quisk's Python, anything that links filter.o's names): kernels' host stubs, C++ helpers and file-scope state stay local."""
    import re
    src = open(os.path.join(HERE, "..", "include", "quiskhip.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    names = sorted(set(n for n in re.findall(r"\b([A-Za-z_][A-Za-z0-9_]*)\s*\([^;{}]*\)\s*;", src) if n != "defined"))
    text = "{\n  global:\n" + "".join("    %s;\n" % n for n in names + list(extra)) + "  local: *;\n};\n"
    try:
        if open(path).read() == text:
            return path
    except OSError:
        pass
    os.makedirs(os.path.dirname(path), exist_ok=True)
    with open(path, "w") as f:
        f.write(text)
    return path


def _deps(src):
    """Headers a source includes (transitively, by name), so that a header edit rebuilds only the units that see it."""
    seen, todo = set(), [os.path.join(CSRC, src)]
    while todo:
        f = todo.pop()
        try:
            text = open(f).read()
        except OSError:
            continue
        for line in text.splitlines():
            line = line.strip()
            if line.startswith('#include "'):
                h = os.path.normpath(os.path.join(os.path.dirname(f), line.split('"')[1]))
                if h not in seen:
                    seen.add(h)
                    todo.append(h)
    return seen


EMNR_NPZ = os.path.join(HERE, "data", "wdsp_emnr_tables.npz")


def _emnr_tables_source(path):
    """WDSP's EMNR falls back to tables compiled into it when its data files `calculus` / `zetaHat.bin` are not in the working
    directory (wdsp/emnr.c:207-225, 317-328): the library does the same with the tables of quisk_amd/data/wdsp_emnr_tables.npz (those
    files' numbers, tools/extract_wdsp_emnr_tables.py) written out as a C++ source of 64-bit words -- generated here, compiled like the
    other units, never committed.  Read with zipfile / struct: building does not need numpy."""
    try:
        if os.path.getmtime(path) >= max(os.path.getmtime(EMNR_NPZ), os.path.getmtime(os.path.abspath(__file__))):
            return path
    except OSError:
        pass
    import struct
    import zipfile

    def raw(z, name):
        b = z.read(name + ".npy")
        assert b[:6] == b"\x93NUMPY", name
        hlen = struct.unpack("<H", b[8:10])[0] if b[6] == 1 else struct.unpack("<I", b[8:12])[0]
        off = (10 if b[6] == 1 else 12) + hlen
        return b[off:]

    with zipfile.ZipFile(EMNR_NPZ) as z:
        gg, ggs, zeta = (struct.unpack("<%dQ" % (len(r) // 8), r) for r in (raw(z, "GG"), raw(z, "GGS"), raw(z, "zeta_hat")))
        valid = struct.unpack("<3600i", raw(z, "zeta_valid"))
        rng = struct.unpack("<4Q", raw(z, "zeta_range"))
        dims = struct.unpack("<2i", raw(z, "zeta_dims"))
    assert len(gg) == 241 * 241 and len(ggs) == 241 * 241 and len(zeta) == 3600 and dims == (60, 60)
    # the compiled-in zetaHat of the reference holds 0 where the file holds its "no value" mark -1e300 (zetahat.c; cells flagged -1);
    # neither is ever read (getZeta, emnr.c:878-882, returns early for flags <= 0)
    mark = struct.unpack("<Q", struct.pack("<d", -1e300))[0]
    zeta = tuple(0 if w == mark else w for w in zeta)

    def words(name, vals, typ="unsigned long long", fmt="0x%016xull"):
        lines = ["extern const %s %s[%d] = {" % (typ, name, len(vals))]
        for i in range(0, len(vals), 6):
            lines.append("    " + ", ".join(fmt % v for v in vals[i:i + 6]) + ",")
        lines.append("};")
        return "\n".join(lines)

    text = "\n".join([
        "// GENERATED by quisk_amd/build.py from quisk_amd/data/wdsp_emnr_tables.npz: the bit patterns of the doubles (see qh_emnr_tables.hpp)",
        "namespace qh {",
        words("kEmnrDefaultGG", gg), words("kEmnrDefaultGGS", ggs), words("kEmnrDefaultZeta", zeta), words("kEmnrDefaultRange", rng),
        words("kEmnrDefaultValid", valid, "int", "%d"),
        "}", ""])
    os.makedirs(os.path.dirname(path), exist_ok=True)
    with open(path, "w") as f:
        f.write(text)
    return path


def build(force=False, verbose=False, defines=(), out=None, jobs=None):
    """One object per source under quisk_amd/lib/obj (rebuilt when the source or a header it includes is newer), then the
    link.  defines/out: experiment builds (tools/ab_bench.py) with -D overrides into another file, compiled in one go;
    QH_HIPCC_FLAGS in the environment adds compiler flags to such builds (scheduler strategies and the like)."""
    target = out or LIB
    base = [_hipcc(), "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-Wall", "-x", "hip"]
    extra = ["-D" + d for d in defines] + os.environ.get("QH_HIPCC_FLAGS", "").split()
    if extra and not out:
        # (the shipped library is kept when it is newer than its sources, whatever it was compiled with: an experiment build that
        # overwrote or silently reused it would measure the wrong thing)
        raise ValueError("quisk_amd.build: -D overrides / QH_HIPCC_FLAGS make an experiment build: pass out=<another file> (tools/ab_bench.py)")
    os.makedirs(os.path.dirname(target), exist_ok=True)
    if out:
        vmap = _export_map(os.path.join(os.path.dirname(target), "quiskhip.map"), extra=["qh_dbg_*"])      # (experiment builds may add probes)
        gen = _emnr_tables_source(os.path.join(os.path.dirname(target), "qh_emnr_tables_gen.cpp"))
        cmd = base + ["-shared", "-Wl,--version-script=" + vmap, "-o", target] + extra + [os.path.join(CSRC, f) for f in SOURCES] + [gen]
        if verbose:
            print(" ".join(cmd), file=sys.stderr)
        subprocess.run(cmd, check=True)
        return target
    objdir = os.path.join(LIBDIR, "obj")
    stamp_file = os.path.join(objdir, "build.stamp")
    if not force and not needs_build():          # the library that travelled with the snapshot is current: nothing to do, nothing started
        return LIB
    # Something will be compiled: what were the objects that are kept compiled with?  Another compiler, ROCm release or flag set makes
    # all of them stale.  (Asked only here -- a process that merely loads a current library must not start a compiler driver.)
    import hashlib
    try:
        ver = subprocess.run([base[0], "--version"], capture_output=True, text=True).stdout
    except OSError:
        ver = ""
    stamp = hashlib.sha256(("\n".join(base[1:] + extra) + "\n" + ver).encode()).hexdigest()
    try:
        if open(stamp_file).read().strip() != stamp:
            force = True
    except OSError:
        if os.path.isdir(objdir):
            force = True
    os.makedirs(objdir, exist_ok=True)
    base = base + extra
    todo, objs = [], []
    gen = _emnr_tables_source(os.path.join(objdir, "qh_emnr_tables_gen.cpp"))
    for src in SOURCES + [gen]:
        obj = os.path.join(objdir, os.path.basename(src) + ".o")
        objs.append(obj)
        stale = force or not os.path.exists(obj)
        if not stale:
            t = os.path.getmtime(obj)
            stale = any(os.path.getmtime(f) > t for f in [os.path.join(CSRC, src)] + [d for d in _deps(src) if os.path.exists(d)])
        if stale:
            todo.append((src, obj))
    hdr = os.path.join(HERE, "..", "include", "quiskhip.h")
    if not todo and os.path.exists(LIB) and all(os.path.getmtime(o) <= os.path.getmtime(LIB) for o in objs + [hdr]):
        return LIB
    jobs = jobs or min(4, os.cpu_count() or 1)
    running = []

    def reap(block):
        for pr, src in list(running):
            if block or pr.poll() is not None:
                if pr.wait() != 0:
                    for other, _ in running:
                        if other is not pr:
                            other.kill()
                    raise subprocess.CalledProcessError(pr.returncode, src)
                running.remove((pr, src))
                if block:
                    return

    for src, obj in todo:
        while len(running) >= jobs:
            reap(True)
        cmd = base + ["-c", os.path.join(CSRC, src), "-o", obj]
        if verbose:
            print(" ".join(cmd), file=sys.stderr)
        running.append((subprocess.Popen(cmd), src))
    while running:
        reap(True)
    vmap = _export_map(os.path.join(objdir, "quiskhip.map"))
    cmd = [_hipcc(), "--offload-arch=gfx950", "-shared", "-fPIC", "-Wl,--version-script=" + vmap, "-o", LIB] + objs
    if verbose:
        print(" ".join(cmd), file=sys.stderr)
    subprocess.run(cmd, check=True)
    with open(stamp_file, "w") as fh:
        fh.write(stamp + "\n")
    return LIB


if __name__ == "__main__":
    print(build(force="--force" in sys.argv, verbose=True))
