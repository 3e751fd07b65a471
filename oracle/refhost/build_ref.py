#!/usr/bin/env python3
"""Build the reference-run libraries oracle/_ref/libref_{contract,nocontract}.so -- TEST INFRASTRUCTURE ONLY.

The reference (kernrj/gsdr) is CUDA, but the kernels named in KERNELS below are one-thread-per-element functions
that g++ compiles for the host once the CUDA headers supply the types and shim.h defines the function-space
keywords away. This script

  1. cuts the text of each named kernel out of the reference's sources into oracle/_ref/extract/<file>.inc
     (from the `__global__` line naming it, with a `template <...>` line just above, to its closing brace),
  2. writes the empty gsdr/gsdr_export.h the reference's CMake would generate, and
  3. compiles driver.cpp around them twice: -ffp-contract=fast -mfma (nvcc contracts by default) and
     -ffp-contract=off,

and records what it used (file hashes, flags) in oracle/_ref/manifest.json. Everything it writes stays under
oracle/_ref/, which git ignores: nothing cut or compiled from the reference is ever committed.

GSDR_REFERENCE_DIR names the reference checkout (default /root/reference). The CUDA headers are the ones the
triton package bundles, found without importing it. Where either is missing the script says so in one line
and succeeds without building anything, so `make all` stays green on machines that have neither.
"""
from __future__ import annotations

import hashlib
import importlib.util
import json
import os
import re
import shutil
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(os.path.dirname(HERE), "_ref")
REFERENCE = os.environ.get("GSDR_REFERENCE_DIR", "/root/reference")

# reference source file -> the __global__ functions taken from it
KERNELS = {
    "fir.cu": ["k_Fir", "k_FirDecimate"],
    "quad_demod.cu": ["k_quadFmDemod", "k_quadAmDemod"],
    "magnitude.cu": ["k_Magnitude", "k_Abs"],
    "add_const.cu": ["k_AddConst", "k_AddToMagnitude"],
    "multiply.cu": ["k_Multiply"],
    "trig.cu": ["k_ComplexCosine", "k_RealCosine"],
    "conversion.cu": ["k_int8ToFloat"],
    "qpsk.cu": ["k_QpskModulateTemplated", "k_QpskModulate", "k_QpskModulate4x"],
    "qpsk256.cu": ["k_InitQpsk256Rectangular", "k_InitQpsk256Circular", "k_Qpsk256Modulate", "k_Qpsk256Modulate4x"],
}
# headers of the reference that driver.cpp includes from its tree (operators, zero<T>())
HEADERS = ["src/cuComplexOperatorOverloads.cuh", "include/gsdr/cuda_util.h"]

COMMON = ["-std=c++14", "-O2", "-fPIC", "-shared", "-fno-fast-math", "-w"]
BUILDS = {
    "contract": ["-ffp-contract=fast", "-mfma"],
    "nocontract": ["-ffp-contract=off", "-mfma"],
}


def lib_path(build: str) -> str:
    return os.path.join(OUT, f"libref_{build}.so")


def sha256(path: str) -> str:
    with open(path, "rb") as f:
        return hashlib.sha256(f.read()).hexdigest()


def cuda_include_dir() -> str | None:
    spec = importlib.util.find_spec("triton")
    for root in (spec.submodule_search_locations or []) if spec else []:
        inc = os.path.join(root, "backends", "nvidia", "include")
        if os.path.exists(os.path.join(inc, "cuComplex.h")) and os.path.exists(os.path.join(inc, "cuda_runtime.h")):
            return inc
    return None


def cut_kernel(lines: list[str], name: str, where: str) -> str:
    """The text of `__global__ ... name(...) { ... }` with its template line, found by pattern and brace depth."""
    head = re.compile(r"\b__global__\b.*\b" + re.escape(name) + r"\s*\(")
    starts = [i for i, ln in enumerate(lines) if head.search(ln) and not ln.lstrip().startswith("template __global__")]
    if len(starts) != 1:
        raise SystemExit(f"refhost: {where}: expected one definition of {name}, found {len(starts)}")
    first = starts[0]
    if first > 0 and lines[first - 1].lstrip().startswith("template"):
        first -= 1
    depth, opened = 0, False
    for last in range(starts[0], len(lines)):
        code = lines[last].split("//", 1)[0]
        if not opened and ";" in code and "{" not in code:
            raise SystemExit(f"refhost: {where}: {name} is a declaration, not a definition")
        depth += code.count("{") - code.count("}")
        opened = opened or "{" in code
        if opened and depth == 0:
            return "".join(lines[first:last + 1])
    raise SystemExit(f"refhost: {where}: unbalanced braces after {name}")


def reference_hashes() -> dict[str, str]:
    files = [os.path.join("src", f) for f in KERNELS] + HEADERS
    return {f: sha256(os.path.join(REFERENCE, f)) for f in sorted(files)}


def main() -> int:
    missing = [f for f in [os.path.join("src", f) for f in KERNELS] + HEADERS
               if not os.access(os.path.join(REFERENCE, f), os.R_OK)]
    if missing:
        print(f"refhost: no reference at {REFERENCE} ({missing[0]} unreadable): reference-run libraries not built")
        return 0
    inc = cuda_include_dir()
    if inc is None:
        print("refhost: no CUDA headers (triton's backends/nvidia/include): reference-run libraries not built")
        return 0
    cxx = os.environ.get("CXX", "g++")
    if shutil.which(cxx) is None:
        print(f"refhost: no {cxx}: reference-run libraries not built")
        return 0

    manifest = {
        "reference_sha256": reference_hashes(),
        "recipe_sha256": {f: sha256(os.path.join(HERE, f)) for f in ("build_ref.py", "driver.cpp", "shim.h")},
        "kernels": KERNELS,
        "compiler": subprocess.run([cxx, "--version"], capture_output=True, text=True).stdout.splitlines()[0],
        "flags": {b: " ".join(COMMON + f) for b, f in BUILDS.items()},
    }
    stamp = os.path.join(OUT, "manifest.json")
    if os.path.exists(stamp) and all(os.path.exists(lib_path(b)) for b in BUILDS):
        with open(stamp) as f:
            if json.load(f) == manifest:
                return 0  # up to date

    extract = os.path.join(OUT, "extract")
    os.makedirs(extract, exist_ok=True)
    os.makedirs(os.path.join(OUT, "gsdr"), exist_ok=True)
    for src, names in KERNELS.items():
        with open(os.path.join(REFERENCE, "src", src)) as f:
            lines = f.readlines()
        with open(os.path.join(extract, os.path.splitext(src)[0] + ".inc"), "w") as f:
            f.write("\n".join(cut_kernel(lines, n, src) for n in names))
    with open(os.path.join(OUT, "gsdr", "gsdr_export.h"), "w") as f:
        f.write("#ifndef GSDR_PUBLIC\n#define GSDR_PUBLIC\n#endif\n")
    if os.path.exists(stamp):
        os.remove(stamp)
    includes = ["-I" + HERE, "-I" + OUT, "-I" + os.path.join(REFERENCE, "src"),
                "-I" + os.path.join(REFERENCE, "include"), "-isystem", inc]
    for build, flags in BUILDS.items():
        cmd = [cxx] + COMMON + flags + includes + [os.path.join(HERE, "driver.cpp"), "-o", lib_path(build), "-lm"]
        subprocess.run(cmd, check=True)
    with open(stamp, "w") as f:
        json.dump(manifest, f, indent=1, sort_keys=True)
    print(f"refhost: built {', '.join(os.path.basename(lib_path(b)) for b in BUILDS)} from {REFERENCE}")
    return 0


if __name__ == "__main__":
    sys.exit(main())
