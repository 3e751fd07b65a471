"""Call time of gsdrxChannelizer at four shapes (development tool), each on 2^26 input
samples:
  (a) CF32, M = 16, D =  8, T = 127
  (b) CF32, M = 16, D = 16, T = 128
  (c) CF32, M = 64, D = 64, T = 512
  (d) CS8,  M = 16, D =  8, T = 127
each against yardsticks taken in the same run:
  copy  -- a device-to-device copy that moves the call's input plus output bytes (reads half of them, writes half);
  multi -- (a), (d): what the library offered before the channelizer for the same 16 rows, ops.xlating_fir_multi
           with the channel frequencies c fs / 16 at D = 8.
Section 5's conventions: the buffer sets rotate and together exceed twice the 256 MB Infinity Cache, so every call
streams from HBM; an untimed settle phase precedes the rounds; the legs alternate within a round; HIP events around
`reps` calls a leg; min and median over the rounds.

    python tools/channelizer_time.py [--rounds 7] [--reps 5] [--settle 1.0] [--shapes abcd] [--out FILE]
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
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--settle", type=float, default=1.0, help="seconds of untimed calls before the rounds of a shape")
ap.add_argument("--shapes", default="abcd")
ap.add_argument("--inputs", type=int, default=1 << 26, help="input samples a call")
ap.add_argument("--out", default=None, help="also write the table to this file")
opt = ap.parse_args()

CACHE = 256 << 20
SHAPES = {
    "a": ("CF32 M=16 D=8 T=127", torch.complex64, 16, 8, 127, True),
    "b": ("CF32 M=16 D=16 T=128", torch.complex64, 16, 16, 128, False),
    "c": ("CF32 M=64 D=64 T=512", torch.complex64, 64, 64, 512, False),
    "d": ("CS8 M=16 D=8 T=127", torch.int8, 16, 8, 127, True),
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


def make_input(dtype, n, g):
    if dtype == torch.int8:
        return torch.randint(-128, 128, (2 * n,), dtype=torch.int8, device=dev, generator=g)
    return (torch.rand(2 * n, device=dev, generator=g) * 2 - 1).view(torch.complex64)


def run_shape(key):
    label, dtype, M, D, T, multi_leg = SHAPES[key]
    n_in = opt.inputs
    in_bytes = n_in * (2 if dtype == torch.int8 else 8)
    N = (n_in - T) // D + 1
    out_bytes = M * N * 8
    bytes_call = in_bytes + out_bytes
    sets = max(2, -(-2 * CACHE // bytes_call))  # the rotation covers at least twice the cache
    g = torch.Generator(device=dev).manual_seed(7)
    taps = torch.from_numpy(lowpass_taps(T, 0.4 / M)).to(dev)
    xs = [make_input(dtype, n_in, g) for _ in range(sets)]
    ys = [torch.empty((M, N), dtype=torch.complex64, device=dev) for _ in range(sets)]
    # the copy yardstick: half the call's bytes read and as many written
    cs = [torch.rand(bytes_call // 8, device=dev, generator=g) for _ in range(sets)]
    cd = [torch.empty(bytes_call // 8, dtype=torch.float32, device=dev) for _ in range(sets)]
    legs = [("channelizer", lambda k: ops.channelizer(xs[k % sets], taps, M, D, 0, N, out=ys[k % sets])),
            ("copy", lambda k: cd[k % sets].copy_(cs[k % sets]))]
    if multi_leg:
        chans = [float(c) for c in range(M)]   # fs = M: channel c at c fs / M
        zs = [torch.empty((M, N), dtype=torch.complex64, device=dev) for _ in range(sets)]
        legs.append(("multi", lambda k: ops.xlating_fir_multi(xs[k % sets], taps, float(M), 0.0, chans, D, 0, N,
                                                              out=zs[k % sets])))
        # the two routes compute the same thing
        legs[0][1](0)
        legs[2][1](0)
        torch.cuda.synchronize()
        diff = (ys[0] - zs[0]).abs().max().item()
        assert diff <= 1e-4, diff
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
    say("(%s) %s: %d inputs -> %d x %d outputs, %.1f MB in + out a call, %d buffer sets" %
        (key, label, n_in, M, N, bytes_call / 1e6, sets))
    med = {}
    for name, _ in legs:
        v = times[name]
        med[name] = statistics.median(v)
        say("    %-11s min %9.1f us  median %9.1f us  (%.2f TB/s of the channelizer's in + out bytes at the median; "
            "rounds: %s)" % (name, min(v), med[name], bytes_call / med[name] / 1e6, " ".join("%.0f" % t for t in v)))
    say("    channelizer moves its bytes at %.2f of the copy's rate" % (med["copy"] / med["channelizer"]))
    if multi_leg:
        say("    multi / channelizer = %.2f (must be > 1)" % (med["multi"] / med["channelizer"]))
    del xs, ys, cs, cd, legs
    torch.cuda.empty_cache()
    return med


results = {key: run_shape(key) for key in opt.shapes}
ok = all(r["multi"] > r["channelizer"] for r in results.values() if "multi" in r)
say("timing condition (channelizer faster than xlating_fir_multi on (a) and (d)): %s" % ("met" if ok else "NOT met"))
if opt.out:
    os.makedirs(os.path.dirname(os.path.abspath(opt.out)), exist_ok=True)
    with open(opt.out, "w") as f:
        f.write("\n".join(lines) + "\n")
sys.exit(0 if ok else 1)
