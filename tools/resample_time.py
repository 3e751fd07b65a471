"""Call time of gsdrxResampleFF / FC at three shapes (development tool):
  (a) FF 24 / 125, 769 taps, 2^26 input samples  (250 kHz -> 48 kHz class)
  (b) FC  5 /   6, 121 taps, 2^26 input samples
  (c) FC  4 /   1,  65 taps, 2^24 input samples  (4x interpolation)
each against two yardsticks taken in the same run:
  copy      -- a device-to-device copy that moves the call's input plus output bytes (reads half of them, writes half);
  stuff+fir -- (b), (c): what the library offered before the resampler, ops.fir(taps, zero_stuffed, decimation=M) on
               a zero-stuffed buffer built beforehand; only the FIR call is timed.
Section 5's conventions: the buffer sets rotate and together exceed the 256 MB Infinity Cache, so every call streams
from HBM; an untimed settle phase precedes the rounds; the legs alternate within a round; HIP events around `reps`
calls a leg; min and median over the rounds.

    python tools/resample_time.py [--rounds 7] [--reps 10] [--settle 2.0] [--out FILE]
"""
import argparse
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from gsdr_amd import ops  # noqa: E402
from gsdr_amd.signals import lowpass_taps  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--rounds", type=int, default=7)
ap.add_argument("--reps", type=int, default=10)
ap.add_argument("--settle", type=float, default=2.0, help="seconds of untimed calls before the rounds of a shape")
ap.add_argument("--shapes", default="abc")
ap.add_argument("--out", default=None, help="also write the table to this file")
opt = ap.parse_args()

CACHE = 256 << 20
SHAPES = {
    "a": ("FF 24/125 T=769", torch.float32, 24, 125, 769, 1 << 26, False),
    "b": ("FC 5/6 T=121", torch.complex64, 5, 6, 121, 1 << 26, True),
    "c": ("FC 4/1 T=65", torch.complex64, 4, 1, 65, 1 << 24, True),
}
dev = torch.device("cuda", 0)
lines = []


def say(text):
    print(text, flush=True)
    lines.append(text)


def timed(fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for k in range(reps):
        fn(k)
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps * 1e3  # microseconds a call


def run_shape(key):
    label, dtype, L, M, T, n_in, stuffed_leg = SHAPES[key]
    size = 8 if dtype.is_complex else 4
    N = (n_in * L - T) // M + 1
    assert ops.resample_inputs_for(L, M, 0, T, N) <= n_in
    bytes_call = (n_in + N) * size
    sets = max(2, -(-2 * CACHE // bytes_call))  # the rotation covers at least twice the cache
    g = torch.Generator(device=dev).manual_seed(7)
    taps = torch.from_numpy(lowpass_taps(T, 0.4 / max(L, M)) * L).to(dev)
    xs = [(torch.rand(n_in * (size // 4), device=dev, generator=g) * 2 - 1).view(dtype) for _ in range(sets)]
    ys = [torch.empty(N, dtype=dtype, device=dev) for _ in range(sets)]
    # the copy yardstick: (n_in + N) / 2 elements read and as many written, the resampler's traffic
    cs = [torch.rand((n_in + N) // 2 * (size // 4), device=dev, generator=g).view(dtype) for _ in range(2 * sets)]
    cd = [torch.empty((n_in + N) // 2, dtype=dtype, device=dev) for _ in range(2 * sets)]
    legs = [("resample", lambda k: ops.resample(taps, xs[k % sets], L, M, 0, N, out=ys[k % sets])),
            ("copy", lambda k: cd[k % (2 * sets)].copy_(cs[k % (2 * sets)]))]
    us = []
    if stuffed_leg:
        for x in xs[:max(2, -(-2 * CACHE // (n_in * L * size)))]:
            u = torch.zeros(n_in * L, dtype=dtype, device=dev)
            u[::L] = x
            us.append(u)
        legs.append(("stuff+fir", lambda k: ops.fir(taps, us[k % len(us)], M, N, out=ys[k % sets])))
        # the two routes compute the same thing
        a = ops.resample(taps, xs[0], L, M, 0, N)
        b = ops.fir(taps, us[0], M, N)
        torch.cuda.synchronize()
        diff = (a - b).abs().max().item()
        assert diff <= 1e-4 * L, diff
    t_end = time.time() + opt.settle
    k = 0
    while time.time() < t_end:  # untimed: clocks and caches settle on this shape's own work
        for _, fn in legs:
            fn(k)
        torch.cuda.synchronize()
        k += 1
    times = {name: [] for name, _ in legs}
    for _ in range(opt.rounds):
        for name, fn in legs:
            times[name].append(timed(fn, opt.reps))
    say("(%s) %s: %d inputs -> %d outputs, %.1f MB in + out a call, %d buffer sets" %
        (key, label, n_in, N, bytes_call / 1e6, sets))
    med = {}
    for name, _ in legs:
        v = times[name]
        med[name] = statistics.median(v)
        say("    %-10s min %9.1f us  median %9.1f us  (%.2f TB/s of the resampler's in + out bytes at the median; "
            "rounds: %s)" % (name, min(v), med[name], bytes_call / med[name] / 1e6, " ".join("%.0f" % t for t in v)))
    say("    resample moves its bytes at %.2f of the copy's rate" % (med["copy"] / med["resample"]))
    if stuffed_leg:
        say("    stuff+fir / resample = %.2f (must be > 1)" % (med["stuff+fir"] / med["resample"]))
    del xs, ys, cs, cd, us, legs
    torch.cuda.empty_cache()
    return med


results = {key: run_shape(key) for key in opt.shapes}
ok = all(r["stuff+fir"] > r["resample"] for r in results.values() if "stuff+fir" in r)
say("timing condition (resample faster than stuff+fir on (b) and (c)): %s" % ("met" if ok else "NOT met"))
if opt.out:
    os.makedirs(os.path.dirname(os.path.abspath(opt.out)), exist_ok=True)
    with open(opt.out, "w") as f:
        f.write("\n".join(lines) + "\n")
sys.exit(0 if ok else 1)
