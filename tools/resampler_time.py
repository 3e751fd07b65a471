"""Call time of gsdrxResamplerProcess against the one-shot call it replaces (development tool),
for (a) FF 24 / 125, 769 taps and (b) FC 5 / 6, 121 taps, at chunks of 2^20 and 2^16 input samples:
  stream  -- gsdrxResamplerProcess, one call a chunk of a continuing stream;
  by hand -- gsdrxResampleFF / FC on the same chunk with the overlap already in place (the chunks lie back to back in
             one buffer, so the previous chunk's tail is the overlap): what callers did before, without their paste
             copy, so a floor for what they paid. The one-shot kernels are the resampler's own.
Both legs go straight through the C ABI with arguments prepared beforehand, so a call's host cost is one ctypes call.
The method of tools/resample_time.py: the chunk slots rotate and together exceed twice the 256 MB Infinity Cache;
an untimed settle phase precedes the rounds; the legs alternate; HIP events around one pass over the slots; a round's
figure is the median of its passes, a leg's the median over the rounds.

Condition, at 2^20: stream median <= by-hand median + margin, margin = the by-hand leg's own spread over the rounds
(max - min of its round medians), at least 5 % of its median. The 2^16 rows are launch-bound and carry no bar.

    python tools/resampler_time.py [--rounds 7] [--passes 5] [--settle 1.0] [--out FILE]
"""
import argparse
import ctypes
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from gsdr_amd import ops  # noqa: E402
from gsdr_amd.abi import check, lib  # noqa: E402
from gsdr_amd.signals import lowpass_taps  # noqa: E402
from gsdr_amd.stream import Resampler  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--rounds", type=int, default=7)
ap.add_argument("--passes", type=int, default=5, help="timed passes over the slots a leg and round")
ap.add_argument("--settle", type=float, default=1.0, help="seconds of untimed calls before the rounds of a row")
ap.add_argument("--out", default=None, help="also write the table to this file")
opt = ap.parse_args()

CACHE = 256 << 20
SHAPES = [("(a) FF 24/125 T=769", torch.float32, 24, 125, 769), ("(b) FC 5/6 T=121", torch.complex64, 5, 6, 121)]
CHUNKS = [1 << 20, 1 << 16]
dev = torch.device("cuda", 0)
lines = []


def say(text):
    print(text, flush=True)
    lines.append(text)


def total_outputs(L, M, T, S):
    return (S * L - T) // M + 1 if S * L >= T else 0


def timed(fn, calls):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / calls * 1e3  # microseconds a call


def run_row(label, dtype, L, M, T, C):
    size = 8 if dtype.is_complex else 4
    w = -(-T // L)
    cap = C * L // M + 2                              # outputs a call writes at most
    slots = max(2, -(-2 * CACHE // ((C + cap) * size)))  # the rotation covers at least twice the cache
    taps = torch.from_numpy(lowpass_taps(T, 0.4 / max(L, M)) * L).to(dev)
    g = torch.Generator(device=dev).manual_seed(7)
    # slot j's chunk is x[w + j C, w + (j + 1) C): the w samples in front of it are the by-hand leg's overlap
    x = (torch.rand((w + slots * C) * (size // 4), device=dev, generator=g) * 2 - 1).view(dtype)
    y = torch.empty(slots * cap, dtype=dtype, device=dev)
    stream = torch.cuda.current_stream(dev).cuda_stream
    one_shot = lib.gsdrxResampleFC if dtype.is_complex else lib.gsdrxResampleFF
    r = Resampler(taps, L, M, 0, complex_samples=dtype.is_complex)
    written = ctypes.c_size_t(0)

    def stream_pass():
        for j in range(slots):
            check("gsdrxResamplerProcess", lib.gsdrxResamplerProcess(
                r._h, x.data_ptr() + (w + j * C) * size, C, y.data_ptr() + j * cap * size, cap, ctypes.byref(written),
                stream))

    # the by-hand leg's calls: call k of a stream of C-sample chunks (k >= 1: a call with an overlap), in slot k mod slots
    by_hand = []
    for k in range(1, slots + 1):
        S, m = k * C, total_outputs(L, M, T, k * C)
        n = total_outputs(L, M, T, S + C) - m
        first, q = (m * M) // L, (m * M) % L
        assert -w <= first - S <= 0 and ops.resample_inputs_for(L, M, q, T, n) <= S + C - first and n <= cap
        j = k % slots
        by_hand.append((L, M, q, taps.data_ptr(), T, x.data_ptr() + (w + j * C + first - S) * size,
                        y.data_ptr() + j * cap * size, n, 0, stream))

    def by_hand_pass():
        for args in by_hand:
            check("gsdrxResample", one_shot(*args))

    # the two legs compute the same thing: call 1 of a fresh stream over slots 0 and 1, bit for bit
    stream_pass()
    torch.cuda.synchronize()
    n1 = by_hand[0][7]
    a = y[cap:cap + n1].clone()
    check("gsdrxResample", one_shot(*by_hand[0]))
    torch.cuda.synchronize()
    assert torch.equal(torch.view_as_real(a) if dtype.is_complex else a,
                       torch.view_as_real(y[cap:cap + n1]) if dtype.is_complex else y[cap:cap + n1])
    legs = [("stream", stream_pass), ("by hand", by_hand_pass)]
    t_end = time.time() + opt.settle
    while time.time() < t_end:  # untimed: clocks and caches settle on this row's own work
        for _, fn in legs:
            fn()
        torch.cuda.synchronize()
    rounds = {name: [] for name, _ in legs}
    for _ in range(opt.rounds):
        for name, fn in legs:
            rounds[name].append(statistics.median(timed(fn, slots) for _ in range(opt.passes)))
    torch.cuda.synchronize()
    r.close()
    med = {name: statistics.median(v) for name, v in rounds.items()}
    say("%s, chunks of %d samples (%d slots, <= %d outputs a call):" % (label, C, slots, cap))
    for name, _ in legs:
        say("    %-8s median %8.2f us a call  (round medians: %s)" %
            (name, med[name], " ".join("%.2f" % t for t in rounds[name])))
    spread = max(rounds["by hand"]) - min(rounds["by hand"])
    margin = max(spread, 0.05 * med["by hand"])
    ok = med["stream"] <= med["by hand"] + margin
    say("    stream - by hand = %+.2f us; margin %.2f us (by-hand spread %.2f us, 5 %% of its median %.2f us)" %
        (med["stream"] - med["by hand"], margin, spread, 0.05 * med["by hand"]))
    del x, y
    torch.cuda.empty_cache()
    return ok


verdict = True
for label, dtype, L, M, T in SHAPES:
    for C in CHUNKS:
        ok = run_row(label, dtype, L, M, T, C)
        if C == 1 << 20:
            say("    condition (stream <= by hand + margin): %s" % ("met" if ok else "NOT met"))
            verdict = verdict and ok
        else:
            say("    (launch-bound: reported without a bar)")
say("timing condition at 2^20 on both shapes: %s" % ("met" if verdict else "NOT met"))
if opt.out:
    os.makedirs(os.path.dirname(os.path.abspath(opt.out)), exist_ok=True)
    with open(opt.out, "w") as f:
        f.write("\n".join(lines) + "\n")
sys.exit(0 if verdict else 1)
