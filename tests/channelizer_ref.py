"""Reference for the channelizer's tests (gsdrxChannelizer, gsdr_ext.h); a helper, not a test module.

    n(m, i) = n0 + m D + i,
    output[c, m] = sum_{i < T} h[i] x[m D + i] exp(-j 2 pi ((c n(m, i)) mod M) / M)

evaluated term by term in float64 / complex128 with exact integer phases: no branch sums, no DFT, no rotation.
test_channelizer_host.py ties it to the project's oracle (oracle.chain_fir with fs = M, tune = 0, chan = c)."""
import os
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "gsdr_amd", "csrc")


def int8_to_float(x8):
    """gsdrInt8ToNormFloat on interleaved int8 I/Q, as complex64: max(-1, v / 127) a component, in float32."""
    f = np.maximum(np.float32(-1.0), x8.astype(np.float32) / np.float32(127.0))
    return np.ascontiguousarray(f).view(np.complex64)


def phasors(M):
    """exp(-j 2 pi k / M), k in [0, M), the multiples of a quarter turn exact."""
    k = np.arange(M)
    t = np.exp(-2j * np.pi * k / M)
    for q, v in ((0, 1), (1, -1j), (2, -1), (3, 1j)):
        if (q * M) % 4 == 0:
            t[q * M // 4] = v
    return t


def _blocks(x, T, D, N, m0, per_output):
    """Yields (lo, hi, m, windows): windows[a, i] = x[(m0 + lo + a) D + i], blocks of at most 2^22 / per_output rows."""
    i = np.arange(T, dtype=np.int64)
    chunk = max(1, (1 << 22) // max(per_output, 1))
    for lo in range(0, N, chunk):
        hi = min(lo + chunk, N)
        m = np.arange(m0 + lo, m0 + hi, dtype=np.int64)
        yield lo, hi, m, x[m[:, None] * D + i[None, :]]


def channelizer_ref(h, x, M, D, n0, N, m0=0):
    """Output times m0 .. m0 + N of the stream (x, n0): an (M, N) complex128 array. The real taps are applied a
    component at a time (h x formed as two real products), then the phasor of each term."""
    h = np.asarray(h, np.float64)
    x = np.asarray(x)
    T = h.size
    out = np.zeros((M, N), np.complex128)
    if T == 0 or N == 0:
        return out
    table = phasors(M)
    c = np.arange(M, dtype=np.int64)
    i = np.arange(T, dtype=np.int64)
    r_base = int(n0) % M   # Python integers: n0 may exceed 63 bits
    for lo, hi, m, w in _blocks(x, T, D, N, m0, T * M):
        w = w.astype(np.complex128)
        tr, ti = h[None, :] * w.real, h[None, :] * w.imag
        r = (r_base + (m[:, None] * D + i[None, :]) % M) % M            # n(m, i) mod M
        p = table[(c[:, None, None] * r[None, :, :]) % M]              # (M, rows, T)
        with np.errstate(invalid="ignore", over="ignore"):
            out.real[:, lo:hi] = np.sum(tr[None] * p.real - ti[None] * p.imag, axis=2)
            out.imag[:, lo:hi] = np.sum(tr[None] * p.imag + ti[None] * p.real, axis=2)
    return out


def channelizer_bound(h, x, D, N, m0=0):
    """S_m = sum_i |h_i| |x_{m D + i}|, the same for every channel of output time m."""
    h = np.abs(np.asarray(h, np.float64))
    x = np.asarray(x)
    s = np.zeros(N, np.float64)
    if h.size == 0:
        return s
    for lo, hi, _, w in _blocks(x, h.size, D, N, m0, h.size):
        s[lo:hi] = np.abs(w.astype(np.complex128)) @ h
    return s


PLAN_PROGRAM = r"""
#include <cinttypes>
#include <cstdio>

#include "channelizer_plan.hpp"

int main() {
  using namespace gsdr::channelizer;
  uint64_t M, D, T, n;
  while (std::scanf("%" SCNu64 " %" SCNu64 " %" SCNu64 " %" SCNu64, &M, &D, &T, &n) == 4) {
    Plan p{};
    uint64_t need = 0;
    const bool fits = extents(M, D, T, n, &need);
    const bool ok = plan(M, D, T, n, &p);
    std::printf("{\"ok\":%d,\"fits\":%d,\"valid\":%d,\"route\":%d,\"wg\":%u,\"kt\":%u,\"span\":%u,\"lds_bytes\":%u,"
                "\"blocks\":%" PRIu64 ",\"pad\":%u}\n",
                ok ? 1 : 0, fits ? 1 : 0, valid_channels(M) ? 1 : 0, p.route, p.wg, p.kt, p.span, p.lds_bytes, p.blocks,
                row_pad((uint32_t)D));
  }
  return 0;
}
"""


def build_plan_program(directory, extra_flags=()):
    """Compiles the library's launch plan (gsdr_amd/csrc/channelizer_plan.hpp, HIP-free) into a host program in
    `directory`; returns run(cases) -> one dict a case (M, D, T, output times), in order."""
    import json

    src = os.path.join(str(directory), "channelizer_plan.cpp")
    exe = os.path.join(str(directory), "channelizer_plan" +
                       ("_" + "".join(c for c in "".join(extra_flags) if c.isalnum()) if extra_flags else ""))
    with open(src, "w") as f:
        f.write(PLAN_PROGRAM)
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", *extra_flags, "-I" + CSRC, src, "-o", exe],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]

    def run(cases):
        text = "".join("%d %d %d %d\n" % tuple(c) for c in cases)
        out = subprocess.run([exe], input=text, capture_output=True, text=True)
        assert out.returncode == 0 and out.stderr == "", (out.returncode, out.stderr[-3000:])
        lines = out.stdout.splitlines()
        assert len(lines) == len(cases)
        return [json.loads(line) for line in lines]

    return run
