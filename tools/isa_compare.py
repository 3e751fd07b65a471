#!/usr/bin/env python3
"""Compare the gfx950 device code of two source trees kernel by kernel (development tool; no GPU needed).

    tools/isa_compare.py <tree A> <tree B> [--jobs N] [--work DIR]

Each tree (a checkout, or `git archive <commit> | tar -x -C <dir>`) has every gsdr_amd/csrc/*.hip compiled to device
assembly with the Makefile's flags: once as the product build, and fir.hip and iir.hip once more with
-DGSDR_TUNING_PROBES (the `probes` target). A kernel is its instruction stream from its label to its end marker plus
the `.amdhsa_*` lines of its descriptor; comments are dropped, and block-label numbers and the kernel's own name are
normalised. Kernels pair by name first; what is left over pairs by normalised body (a renamed instantiation whose
code did not change). Prints, per build, what paired and every kernel left without an identical counterpart; exits
non-zero if the product builds differ. Assembly already under <work>/<a|b>_<build>/ is reused, not compiled again.
"""
import argparse
import collections
import concurrent.futures
import glob
import hashlib
import os
import re
import subprocess
import sys

HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
FLAGS = ["-O3", "-std=c++17", "-fPIC", "-ffp-contract=off", "--offload-arch=gfx950", "-fvisibility=hidden",
         "-fvisibility-inlines-hidden", "-Wno-unused-function", "-munsafe-fp-atomics"]
PROBE_UNITS = ("fir", "iir")


def compile_unit(tree, unit, out, probes):
    if os.path.exists(out):
        return
    cmd = [HIPCC, *FLAGS, f"-I{tree}/include", f"-I{tree}/gsdr_amd/csrc", "--cuda-device-only", "-S",
           f"{tree}/gsdr_amd/csrc/{unit}.hip", "-o", out + ".tmp"]
    if probes:
        cmd.insert(1, "-DGSDR_TUNING_PROBES")
    r = subprocess.run(cmd, capture_output=True, text=True)
    if r.returncode != 0:
        sys.exit(f"{' '.join(cmd)}\n{r.stderr}")
    os.rename(out + ".tmp", out)


def kernels(path):
    """{kernel symbol: normalised text} of one device assembly file."""
    lines = open(path).read().splitlines()
    body, desc = {}, {}
    i = 0
    while i < len(lines):
        m = re.match(r"(\w+):\s*(;.*)?$", lines[i])
        if m and i > 0 and any(f"@function" in l and m.group(1) in l for l in lines[max(0, i - 6):i]):
            name, j, text = m.group(1), i + 1, []
            while j < len(lines) and not lines[j].startswith(".Lfunc_end"):
                text.append(lines[j])
                j += 1
            body[name] = text
            i = j
        m = re.match(r"\s*\.amdhsa_kernel\s+(\w+)", lines[i]) if i < len(lines) else None
        if m:
            j, text = i + 1, []
            while not lines[j].strip().startswith(".end_amdhsa_kernel"):
                text.append(lines[j])
                j += 1
            desc[m.group(1)] = text
            i = j
        i += 1
    out = {}
    for name, text in body.items():
        norm = []
        for l in text + desc.get(name, []):
            l = l.split(";")[0].replace(name, "KERNEL").strip()
            l = re.sub(r"\.LBB\d+_", ".LBB_", l)
            if l:
                norm.append(l)
        out[name] = "\n".join(norm)
    return out


def demangle(names):
    r = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True).stdout.splitlines()
    return [n.replace("HIP_vector_type<float, 2u>", "f2").replace("gsdr::", "") for n in r]


def name_distance(wa, wb):
    """how many words (identifiers, numbers) of two demangled names have no partner in the other"""
    return sum(((wa - wb) + (wb - wa)).values())


def compare(dir_a, dir_b, label):
    only_a, only_b, changed, by_name, by_body = [], [], [], 0, 0
    units = sorted({os.path.basename(p) for d in (dir_a, dir_b) for p in glob.glob(f"{d}/*.s")})
    for u in units:
        ka = kernels(f"{dir_a}/{u}") if os.path.exists(f"{dir_a}/{u}") else {}
        kb = kernels(f"{dir_b}/{u}") if os.path.exists(f"{dir_b}/{u}") else {}
        same = [n for n in ka if kb.get(n) == ka[n]]
        diff = [n for n in ka if n in kb and kb[n] != ka[n]]
        rest_a = {n: t for n, t in ka.items() if n not in kb}
        rest_b = {n: t for n, t in kb.items() if n not in ka}
        # Renamed: a name in one tree only, the same code. Where several kernels share their code (a switch that changes
        # nothing on one staging path), the closest names pair first, so what stays unpaired is what the other tree lacks.
        names = sorted({*rest_a, *rest_b})
        words = {n: collections.Counter(re.findall(r"\w+", d)) for n, d in zip(names, demangle(names))}
        cand = [(name_distance(words[n], words[m]), n, m) for n, t in rest_a.items() for m, s in rest_b.items() if s == t]
        renamed = 0
        for _, n, m in sorted(cand):
            if n in rest_a and m in rest_b:
                renamed += 1
                del rest_a[n], rest_b[m]
        by_name += len(same)
        by_body += renamed
        changed += [(u, n, "") for n in diff]
        only_a += [(u, n, "") for n in rest_a]
        # (a kernel only in B whose code another kernel of B's unit has too is a second instantiation of the same code)
        only_b += [(u, n, "  [code identical to another kernel of this unit]" if list(kb.values()).count(t) > 1 else "")
                   for n, t in rest_b.items()]
        print(f"  {label:8s} {u[:-2]:12s} A {len(ka):4d} kernels, B {len(kb):4d}: identical {len(same):4d} by name + "
              f"{renamed:4d} renamed")
    print(f"{label}: {by_name} identical by name, {by_body} renamed with identical code, {len(changed)} same name but "
          f"different code, {len(only_a)} only in A, {len(only_b)} only in B")
    for title, rows in (("same name, different code", changed), ("only in A", only_a), ("only in B", only_b)):
        if rows:
            print(f"  {title}:")
            for (u, _, note), d in zip(rows, demangle([n for _, n, _ in rows])):
                print(f"    {u[:-2]}: {d}{note}")
    return not (changed or only_a or only_b)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("tree_a")
    ap.add_argument("tree_b")
    ap.add_argument("--jobs", type=int, default=min(8, os.cpu_count() or 1))
    ap.add_argument("--work", default="build/isa_compare")
    a = ap.parse_args()
    jobs = []
    for side, tree in (("a", a.tree_a), ("b", a.tree_b)):
        tree = os.path.abspath(tree)
        units = sorted(os.path.basename(p)[:-4] for p in glob.glob(f"{tree}/gsdr_amd/csrc/*.hip"))
        for build in ("product", "probes"):
            d = f"{a.work}/{side}_{build}"
            os.makedirs(d, exist_ok=True)
            jobs += [(tree, u, f"{d}/{u}.s", build == "probes") for u in units if build == "product" or u in PROBE_UNITS]
    with concurrent.futures.ThreadPoolExecutor(a.jobs) as ex:
        for f in [ex.submit(compile_unit, *j) for j in jobs]:
            f.result()
    same = compare(f"{a.work}/a_product", f"{a.work}/b_product", "product")
    compare(f"{a.work}/a_probes", f"{a.work}/b_probes", "probes")
    sys.exit(0 if same else 1)


if __name__ == "__main__":
    main()
