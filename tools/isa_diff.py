#!/usr/bin/env python3
"""Compare the gfx950 device assembly that two csrc directories compile to.  Needs no GPU.

    python tools/isa_diff.py <csrc A> <csrc B> [--jobs N] [--keep DIR] [--only pb_force.hip ...]

Each directory is a particlerobotsimulations_amd/csrc of a checkout (the Makefile's include paths are relative to
it), typically A = a `git worktree` of the parent commit and B = the working tree.  Every .hip that reaches
pb_device.hpp or pb_sweep.hpp through its quoted includes is compiled with that directory's own DEVFLAGS (asked of
its Makefile, `make -pn`) plus --offload-device-only -S.  Lines that define or name the __hip_cuid_<hash> symbol (a
hash of the source text) are dropped; the rest is compared per file and per kernel symbol.  For a kernel that
differs the report gives, for both sides, the registers, LDS and scratch of its metadata and its instruction count.
Exit status: 0 if every file is identical, 1 if not.
"""
import argparse
import concurrent.futures
import os
import re
import subprocess
import sys
import tempfile

SHARED = ("pb_device.hpp", "pb_sweep.hpp")
META_KEYS = (".vgpr_count", ".sgpr_count", ".group_segment_fixed_size", ".private_segment_fixed_size")


def make_vars(csrc):
    """HIPCC and DEVFLAGS as the directory's Makefile expands them."""
    db = subprocess.run(["make", "-pn", "-C", csrc], text=True, capture_output=True).stdout
    out = {}
    for name in ("HIPCC", "DEVFLAGS"):
        m = re.search(r"^%s\s*:?=\s*(.*)$" % name, db, re.M)
        if not m:
            sys.exit(f"isa_diff: {csrc}/Makefile defines no {name}")
        out[name] = m.group(1).strip()
    return out


def reaches_shared(csrc, name, seen=None):
    seen = set() if seen is None else seen
    if name in SHARED:
        return True
    path = os.path.join(csrc, name)
    if name in seen or not os.path.isfile(path):
        return False
    seen.add(name)
    with open(path, errors="replace") as fh:
        incs = re.findall(r'^\s*#\s*include\s+"([^"]+)"', fh.read(), re.M)
    return any(reaches_shared(csrc, i, seen) for i in incs)


def sources(csrc):
    return sorted(f for f in os.listdir(csrc) if f.endswith(".hip") and reaches_shared(csrc, f))


def compile_asm(csrc, mk, src, out):
    cmd = [mk["HIPCC"]] + mk["DEVFLAGS"].split() + ["--offload-device-only", "-S", src, "-o", out]
    r = subprocess.run(cmd, cwd=csrc, text=True, capture_output=True)
    if r.returncode != 0:
        sys.exit(f"isa_diff: {' '.join(cmd)} (in {csrc}) failed:\n{r.stderr}")
    with open(out) as fh:
        return [l.rstrip("\n") for l in fh if "__hip_cuid_" not in l]


def split_kernels(lines):
    """{kernel symbol: {"text": [body + .amdhsa_kernel block], "meta": {...}}}, and the lines outside any kernel."""
    kernels, rest = {}, []
    names = [m.group(1) for l in lines for m in [re.match(r"\s*\.amdhsa_kernel\s+(\S+)", l)] if m]
    want = set(names)
    cur = None
    for l in lines:
        m = re.match(r"(\S+):\s*(;.*)?$", l)
        if cur is None and m and m.group(1) in want and "text" not in kernels.get(m.group(1), {}):
            cur = m.group(1)
            kernels[cur] = {"text": [], "meta": {}}
        if cur is None:
            m = re.match(r"\s*\.amdhsa_kernel\s+(\S+)", l)
            if m and m.group(1) in kernels:
                cur = "desc:" + m.group(1)
        if cur is None:
            rest.append(l)
            continue
        kernels[cur.split(":", 1)[-1]]["text"].append(l)
        if cur.startswith("desc:"):
            if l.strip() == ".end_amdhsa_kernel":
                cur = None
        elif re.match(r"\.Lfunc_end\d+:", l):
            cur = None
    # the metadata note (YAML): registers, LDS and scratch per kernel
    sym, block = None, {}
    for l in rest:
        s = l.strip().lstrip("- ").strip()
        key, _, val = s.partition(":")
        if key in META_KEYS or key == ".symbol":
            block[key] = val.strip().strip("'")
        if key == ".wavefront_size":  # last key of a kernel's entry
            sym = block.get(".symbol", "").removesuffix(".kd")
            if sym in kernels:
                kernels[sym]["meta"] = {k: block.get(k, "?") for k in META_KEYS}
            block = {}
    return kernels, rest


def instructions(text):
    n = 0
    for l in text:
        s = l.strip()
        if s == ".end_amdhsa_kernel" or s.startswith(".amdhsa_"):
            continue
        if s and not s.startswith((".", ";")) and not s.endswith(":") and not re.match(r"\S+:\s*;", s):
            n += 1
    return n


def demangle(sym):
    for tool in ("/opt/rocm/lib/llvm/bin/llvm-cxxfilt", "c++filt"):
        try:
            full = subprocess.check_output([tool, sym], text=True, stderr=subprocess.DEVNULL).strip()
            # "void (anonymous namespace)::k<...>(arguments)" -> "k<...>"
            return re.sub(r"^void |\(anonymous namespace\)::", "", re.sub(r"\((?!anonymous).*$", "", full))
        except Exception:
            pass
    return sym


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("a")
    ap.add_argument("b")
    ap.add_argument("--jobs", type=int, default=min(8, os.cpu_count() or 1))
    ap.add_argument("--keep", help="keep the filtered assembly here (A/<file>.s, B/<file>.s)")
    ap.add_argument("--only", nargs="*", help="compare these .hip files only")
    args = ap.parse_args()
    dirs = {"A": os.path.abspath(args.a), "B": os.path.abspath(args.b)}
    mk = {k: make_vars(d) for k, d in dirs.items()}
    files = sorted(set(sources(dirs["A"])) | set(sources(dirs["B"])))
    if args.only:
        files = [f for f in files if f in args.only]
    missing = [f"{k}:{f}" for f in files for k, d in dirs.items() if not os.path.isfile(os.path.join(d, f))]
    if missing:
        sys.exit("isa_diff: not in both directories: " + ", ".join(missing))

    asm = {}
    with tempfile.TemporaryDirectory() as td, concurrent.futures.ThreadPoolExecutor(args.jobs) as pool:
        jobs = {(k, f): pool.submit(compile_asm, dirs[k], mk[k], f, os.path.join(td, f"{k}_{f}.s"))
                for f in files for k in dirs}
        for key, job in jobs.items():
            asm[key] = job.result()
    if args.keep:
        for (k, f), lines in asm.items():
            os.makedirs(os.path.join(args.keep, k), exist_ok=True)
            with open(os.path.join(args.keep, k, f + ".s"), "w") as fh:
                fh.write("\n".join(lines) + "\n")

    print(f"A: {dirs['A']}\nB: {dirs['B']}")
    roots = {k: os.path.dirname(os.path.dirname(d)) for k, d in dirs.items()}  # (include paths are absolute)
    if any(mk["A"][v].replace(roots["A"], "") != mk["B"][v].replace(roots["B"], "") for v in mk["A"]):
        print("note: the two Makefiles give different HIPCC / DEVFLAGS")
    print(f"{'file':<18} {'lines':>7} {'kernels':>8} {'identical':>10}  whole file")
    all_same = True
    for f in files:
        ka, ra = split_kernels(asm["A", f])
        kb, rb = split_kernels(asm["B", f])
        names = sorted(set(ka) | set(kb))
        differ = [n for n in names if ka.get(n, {}).get("text") != kb.get(n, {}).get("text")]
        same = asm["A", f] == asm["B", f]
        all_same = all_same and same
        print(f"{f:<18} {len(asm['B', f]):>7} {len(names):>8} {len(names) - len(differ):>10}  "
              f"{'identical' if same else 'DIFFERENT'}")
        if not same and not differ:
            print("    (the kernels are identical; the difference is outside them: symbol tables, metadata, device functions)")
        for n in differ:
            print(f"    differs: {demangle(n)}")
            for side, ks in (("A", ka), ("B", kb)):
                if n not in ks:
                    print(f"      {side}: absent")
                    continue
                meta = ks[n]["meta"]
                print(f"      {side}: " + ", ".join(f"{k} {meta.get(k, '?')}" for k in META_KEYS) +
                      f", instructions {instructions(ks[n]['text'])}")
    print("RESULT: " + ("every file identical (__hip_cuid_* aside)" if all_same else "assembly differs"))
    return 0 if all_same else 1


if __name__ == "__main__":
    sys.exit(main())
