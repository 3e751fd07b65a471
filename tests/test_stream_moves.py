"""CPU: where the bytes of a streaming call go (the move lists of gsdr_amd/csrc/stream_plan.hpp, HIP-free), compiled
into a small host program under the address and undefined-behaviour sanitizers and replayed on a model of the four
buffers. The model holds each buffer as an array of absolute sample indices (sample n of the stream is the number n);
the spare and the seam buffer are poisoned before each call, the call's segments are applied in a random order, and
then: the spare holds exactly the next history, the seam buffer exactly what the seam outputs read, every segment lies
inside the capacity the objects allocate and inside the valid part of its source, and no two ranges overlap. The spare
becomes the next call's history, so a sequence checks the ping-pong as well.

The shapes are test_resampler_plan.py's (both end phases) and test_stream_plan.py's (decimation, window) list as
L = 1; the chunk sequences are generated as those tests generate them."""
import json
import os
import random
import subprocess

import numpy as np
import pytest

from resample_ref import CSRC
from test_resampler_plan import SHAPES, chunk_sizes, first, need

STREAM_SHAPES = [(1, 1), (1, 63), (4, 127), (4, 131), (3, 200), (8, 8), (16, 5), (5, 1)]   # test_stream_plan.py's
SEQUENCES, CHUNKS = 12, 30
HIST, SPARE, SEAM, CHUNK = range(4)
POISON = -1

PROGRAM = r"""
#include <cinttypes>
#include <cstdio>
#include <initializer_list>

#include "stream_plan.hpp"

int main() {
  uint64_t L, M, T, q, S, m, c;
  while (std::scanf("%" SCNu64 " %" SCNu64 " %" SCNu64 " %" SCNu64 " %" SCNu64 " %" SCNu64 " %" SCNu64, &L, &M, &T, &q,
                    &S, &m, &c) == 7) {
    gsdr::StreamPlan p;
    const bool ok = gsdr::stream_plan(L, M, T, q, S, m, c, &p);
    gsdr::StreamMoves next, seam;
    if (ok) gsdr::stream_next_history(p, c, &next);
    if (ok) gsdr::stream_seam(p, &seam);
    std::printf("{\"ok\":%d,\"outputs\":%" PRIu64 ",\"seam\":%" PRIu64 ",\"hist\":%" PRIu64 ",\"hist_after\":%" PRIu64
                ",\"first\":%" PRIu64 ",\"first_after\":%" PRIu64 ",\"lead\":%" PRIu64 ",\"head\":%" PRIu64
                ",\"main_off\":%" PRId64 ",\"caps\":[%" PRIu64 ",%" PRIu64 ",%" PRIu64 "],\"segs\":[",
                ok ? 1 : 0, p.outputs, p.seam, p.hist, p.hist_after, p.first, p.first_after, p.lead, p.head, p.main_off,
                gsdr::stream_hist_capacity(L, T), gsdr::stream_hist_capacity(L, T), gsdr::stream_seam_capacity(L, T));
    int k = 0;
    for (const gsdr::StreamMoves* mv : {&next, &seam}) {
      for (int i = 0; i < mv->n; ++i, ++k) {
        const gsdr::StreamMoves::Seg& g = mv->seg[i];
        std::printf("%s[%d,%" PRIu64 ",%d,%" PRIu64 ",%" PRIu64 "]", k ? "," : "", (int)g.dst, g.dst_off, (int)g.src,
                    g.src_off, g.count);
      }
    }
    std::printf("]}\n");
  }
  return 0;
}
"""


@pytest.fixture(scope="module")
def moves(tmp_path_factory):
    """run(cases) -> one dict a case (L, M, T, q, consumed, next output, chunk), in order."""
    d = tmp_path_factory.mktemp("stream_moves")
    src, exe = os.path.join(str(d), "stream_moves.cpp"), os.path.join(str(d), "stream_moves")
    with open(src, "w") as f:
        f.write(PROGRAM)
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-fsanitize=undefined,address",
                        "-fno-sanitize-recover=undefined", "-I" + CSRC, src, "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]

    def run(cases):
        text = "".join("%d %d %d %d %d %d %d\n" % tuple(c) for c in cases)
        out = subprocess.run([exe], input=text, capture_output=True, text=True)
        assert out.returncode == 0 and out.stderr == "", (out.returncode, out.stderr[-3000:])
        lines = out.stdout.splitlines()
        assert len(lines) == len(cases)
        return [json.loads(line) for line in lines]

    return run


def calls_of(L, M, T, q, sizes):
    """The (L, M, T, q, S, m, c) of a sequence from an empty stream: the state follows from the definitions."""
    S = m = 0
    calls = []
    for c in sizes:
        calls.append((L, M, T, q, S, m, c))
        S += c
        while need(L, M, T, q, m) <= S:
            m += 1
    return calls


def overlap(a, b):
    return a[0] == b[0] and a[1] < b[2] and b[1] < a[2]


def replay(calls, plans, rng):
    L, M, T, q = calls[0][:4]
    hist = np.full(plans[0]["caps"][HIST], POISON, np.int64)
    seen = {"kept": 0, "from_both": 0, "seam": 0, "lead": 0}
    for what, p in zip(calls, plans):
        S, m, c = what[4:]
        assert p["ok"] == 1, what
        caps = p["caps"]
        assert caps[HIST] == caps[SPARE] == -(-T // L) and caps[SEAM] == 2 * caps[HIST], what
        # the state the call starts from: the history holds x[first .. S) from offset 0
        assert p["first"] == first(L, M, q, m) and p["hist"] == max(S - p["first"], 0) <= max(caps[HIST] - 1, 0), what
        assert np.array_equal(hist[:p["hist"]], np.arange(p["first"], p["first"] + p["hist"])), what
        buf = {HIST: hist, SPARE: np.full(caps[SPARE], POISON, np.int64), SEAM: np.full(caps[SEAM], POISON, np.int64),
               CHUNK: np.arange(S, S + c, dtype=np.int64)}
        valid = {HIST: p["hist"], CHUNK: c}
        segs = p["segs"]
        assert len(segs) <= 4, what
        dsts, srcs = [], []
        for dst, dst_off, src, src_off, count in segs:
            assert count > 0, (what, segs)
            assert dst in (SPARE, SEAM) and src in (HIST, CHUNK), (what, segs)
            assert dst_off + count <= caps[dst], (what, segs)        # inside the buffer's capacity
            assert src_off + count <= valid[src], (what, segs)       # inside the samples its source holds
            dsts.append((dst, dst_off, dst_off + count))
            srcs.append((src, src_off, src_off + count))
        for i, d in enumerate(dsts):
            assert not any(overlap(d, e) for e in dsts[i + 1:]) and not any(overlap(d, s) for s in srcs), (what, segs)
        for dst, dst_off, src, src_off, count in rng.sample(segs, len(segs)):
            buf[dst][dst_off:dst_off + count] = buf[src][src_off:src_off + count]
        # the spare: exactly x[first_after .. S1) from offset 0, nothing else written
        S1, f1 = S + c, p["first_after"]
        n_after = p["hist_after"]
        assert n_after == max(S1 - f1, 0), what
        want = np.full(caps[SPARE], POISON, np.int64)
        want[:n_after] = np.arange(f1, f1 + n_after)
        assert np.array_equal(buf[SPARE], want), (what, segs)
        # the seam buffer: from first - origin, exactly the samples the seam outputs read
        want = np.full(caps[SEAM], POISON, np.int64)
        if p["seam"]:
            s = q + m * M
            last = need(L, M, T, q, m + p["seam"] - 1)
            assert p["lead"] == p["first"] - s // L and p["head"] == last - S, what
            want[p["lead"]:p["lead"] + last - p["first"]] = np.arange(p["first"], last)
            for k in range(m, m + p["seam"]):        # every seam output's samples are there, at the one-shot call's index
                lo, hi = first(L, M, q, k), need(L, M, T, q, k)
                assert p["first"] <= lo < S and hi <= last, (what, k)
            seen["seam"] += 1
            seen["lead"] += p["lead"]
        assert np.array_equal(buf[SEAM], want), (what, segs)
        if p["outputs"] > p["seam"]:                 # the other outputs' call starts at its origin in the chunk
            k = m + p["seam"]
            assert p["main_off"] == (q + k * M) // L - S and first(L, M, q, k) >= S, what
            assert need(L, M, T, q, m + p["outputs"] - 1) <= S1, what
        srcs_used = {seg[2] for seg in segs if seg[0] == SPARE}
        seen["kept"] += HIST in srcs_used
        seen["from_both"] += srcs_used == {HIST, CHUNK}
        # the swap: the spare is the next call's history
        hist = buf[SPARE] if n_after else np.full(caps[HIST], POISON, np.int64)
    return seen


def sequences(L, M, T, q, seed):
    rng = random.Random(seed)
    return [calls_of(L, M, T, q, chunk_sizes(rng, L, M, T, CHUNKS)) for _ in range(SEQUENCES)]


def run_shape(moves, L, M, T):
    total = {}
    for q in sorted({0, L - 1}):
        seqs = sequences(L, M, T, q, L * 1000003 + M * 101 + T + q)
        plans = moves([call for calls in seqs for call in calls])
        rng = random.Random(T)
        for i, calls in enumerate(seqs):
            seen = replay(calls, plans[i * CHUNKS:(i + 1) * CHUNKS], rng)
            total = {k: total.get(k, 0) + v for k, v in seen.items()}
    return total


@pytest.mark.parametrize("L,M,T", SHAPES)
def test_resampler_shapes(moves, L, M, T):
    seen = run_shape(moves, L, M, T)
    if -(-T // L) > 2:   # a history of two samples or more: both kinds of next history and a seam were met
        assert seen["from_both"] > 0 and seen["seam"] > 0, seen
    if (L, M, T) == (24, 125, 769):
        assert seen["lead"] > 0      # a seam buffer that starts one sample in front of the history


@pytest.mark.parametrize("D,W", STREAM_SHAPES)
def test_stream_shapes(moves, D, W):
    seen = run_shape(moves, 1, D, W)
    assert seen["lead"] == 0
    if W > 2:
        assert seen["from_both"] > 0 and seen["seam"] > 0, seen


def test_a_refused_call_has_no_moves(moves):
    for case in [(1, 4, 127, 0, (1 << 64) - 1, 0, 1), (1, 4, 127, 0, 0, (1 << 63) // 4, 1), (24, 125, 0, 0, 0, 0, 100)]:
        p = moves([case])[0]
        assert p["ok"] == 0 and p["segs"] == [] and p["outputs"] == p["hist_after"] == 0
