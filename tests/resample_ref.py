"""Reference for the rational resampler's tests (gsdrxResampleFF / FC, gsdr_ext.h); a helper, not a test module.

    s(m) = q + m M,  i0 = (L - s mod L) mod L,  n0 = (s + i0) / L,
    output[m] = sum_{p >= 0, i0 + p L < T} h[i0 + p L] x[n0 + p]

in float64 with exact int64 indices, vectorised over p. test_resample_host.py ties it to the project's oracle
(oracle.fir over the zero-stuffed input)."""
import os
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "gsdr_amd", "csrc")


def inputs_for(L, M, q, T, N):
    """floor((q + (N - 1) M + T - 1) / L) + 1 input samples (exact Python integers); 0 for N == 0."""
    if N == 0:
        return 0
    extent = q + (N - 1) * M + T
    return (extent - 1) // L + 1 if extent > 0 else 0


def _windows(L, M, T, q, m):
    """(i0, n0) of outputs m (an int64 array)."""
    s = np.int64(q) + m * np.int64(M)
    i0 = (L - s % L) % L
    return i0, (s + i0) // L


def _accumulate(h, x, L, M, q, N, m0, chunk):
    """Yields (lo, hi, taps, samples, valid) a block of outputs: taps / samples of shape (hi - lo, P)."""
    T = h.size
    P = -(-T // L) if T else 0
    p = np.arange(P, dtype=np.int64)
    chunk = max(1, min(chunk, (1 << 22) // max(P, 1)))  # blocks of at most 4 M products
    for lo in range(m0, m0 + N, chunk):
        hi = min(lo + chunk, m0 + N)
        i0, n0 = _windows(L, M, T, q, np.arange(lo, hi, dtype=np.int64))
        ti = i0[:, None] + p[None, :] * L
        valid = ti < T
        xi = np.where(valid, n0[:, None] + p[None, :], 0)
        v = x[xi].astype(np.complex128 if np.iscomplexobj(x) else np.float64)  # (gathered first: x may be large)
        yield lo - m0, hi - m0, np.where(valid, h[np.where(valid, ti, 0)], 0), np.where(valid, v, 0), valid


def resample_ref(h, x, L, M, q=0, N=None, m0=0, chunk=1 << 15):
    """Outputs m0 .. m0 + N of the stream (x, q), float64 / complex128. Only the products of the definition are formed
    (a non-finite sample outside them does not spread); an empty window gives 0."""
    h = np.asarray(h, np.float64)
    x = np.asarray(x)
    if N is None:
        room = x.size * L - q - h.size
        N = room // M + 1 - m0 if room >= 0 else 0
    out = np.zeros(N, np.complex128 if np.iscomplexobj(x) else np.float64)
    if h.size == 0:
        return out
    for lo, hi, t, v, valid in _accumulate(h, x, L, M, q, N, m0, chunk):
        with np.errstate(invalid="ignore"):
            # real taps: the components apart (a complex product would turn Inf + 1j into Inf + NaN j)
            out.real[lo:hi] = np.sum(np.where(valid, t * v.real, 0), axis=1)
            if np.iscomplexobj(out):
                out.imag[lo:hi] = np.sum(np.where(valid, t * v.imag, 0), axis=1)
    return out


def resample_bound(h, x, L, M, q=0, N=None, m0=0, chunk=1 << 15):
    """S_m = sum |h| |x| over the same products."""
    h = np.abs(np.asarray(h, np.float64))
    x = np.abs(np.asarray(x))   # exact enough for a bound: |x| of float32 / complex64 samples in their own precision
    return resample_ref(h, x, L, M, q, N, m0, chunk)


def zero_stuff(x, L):
    """u[j] = x[j / L] where L divides j, else 0."""
    u = np.zeros(x.size * L, x.dtype)
    u[::L] = x
    return u


def continuation(phase0, m0, L, M):
    """(input offset, phase) of the call whose first output is output m0 of the stream that starts with phase0."""
    U = phase0 + m0 * M
    return U // L, U % L


PLAN_PROGRAM = r"""
#include <cinttypes>
#include <cstdio>

#include "resample_plan.hpp"

int main() {
  uint64_t L, M, T, sample, n;
  while (std::scanf("%" SCNu64 " %" SCNu64 " %" SCNu64 " %" SCNu64 " %" SCNu64, &L, &M, &T, &sample, &n) == 5) {
    gsdr::resample::Plan p{};
    const bool ok = gsdr::resample::plan(L, M, T, (size_t)sample, n, &p);
    std::printf("{\"ok\":%d,\"route\":%d,\"wg\":%u,\"kt\":%u,\"span\":%u,\"lds_bytes\":%u,\"blocks\":%" PRIu64 "}\n",
                ok ? 1 : 0, p.route, p.wg, p.kt, p.span, p.lds_bytes, p.blocks);
  }
  return 0;
}
"""


def build_plan_program(directory, extra_flags=()):
    """Compiles the library's launch plan (gsdr_amd/csrc/resample_plan.hpp, HIP-free) into a host program in
    `directory`; returns run(cases) -> one dict a case (L, M, T, sample bytes, outputs), in order."""
    import json

    src = os.path.join(str(directory), "resample_plan.cpp")
    exe = os.path.join(str(directory), "resample_plan" + ("_" + "".join(c for c in "".join(extra_flags) if c.isalnum())
                                                          if extra_flags else ""))
    with open(src, "w") as f:
        f.write(PLAN_PROGRAM)
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", *extra_flags, "-I" + CSRC, src, "-o", exe],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]

    def run(cases):
        text = "".join("%d %d %d %d %d\n" % tuple(c) for c in cases)
        out = subprocess.run([exe], input=text, capture_output=True, text=True)
        assert out.returncode == 0 and out.stderr == "", (out.returncode, out.stderr[-3000:])
        lines = out.stdout.splitlines()
        assert len(lines) == len(cases)
        return [json.loads(line) for line in lines]

    return run
