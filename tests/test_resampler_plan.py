"""CPU: the host plan of the streaming resampler (gsdrxResamplerPlan, gsdr_amd/csrc/stream_plan.hpp) against
a brute-force model written here from the definitions of include/gsdr/resampler.h, and the argument checks of the
gsdrxResampler entry points that return before any device work.

    s(m) = phase0 + m M,  first(m) = ceil(s(m) / L),  need(m) = floor((s(m) + T - 1) / L) + 1:
output m reads x[first(m) .. need(m)) and is written by the first call after which need(m) samples have arrived.
"""
import ctypes
import random

import pytest

from resample_ref import inputs_for

HIP_SUCCESS = 0
HIP_ERROR_INVALID_VALUE = 1

SHAPES = [(24, 125, 769), (24, 125, 1), (24, 125, 23), (24, 125, 24), (4, 1, 65), (125, 24, 2000), (5, 6, 23),
          (2, 100001, 7), (1, 4, 127), (4096, 4099, 8192)]
SEQUENCES, CHUNKS = 40, 30


@pytest.fixture(scope="module")
def plan():
    from gsdr_amd.stream import resampler_plan

    return resampler_plan


def first(L, M, q, m):
    return -(-(q + m * M) // L)


def need(L, M, T, q, m):
    return (q + m * M + T - 1) // L + 1


def total_outputs(L, M, T, q, S):
    """The largest N with inputs_for(L, M, q, T, N) <= S, checked against inputs_for itself."""
    N = (S * L - T - q) // M + 1 if S * L >= T + q else 0
    assert inputs_for(L, M, q, T, N) <= S < inputs_for(L, M, q, T, N + 1)
    return N


def chunk_sizes(rng, L, M, T, count):
    w = -(-T // L)
    per = -(-M // L)
    menu = [0, 1, 2, max(w - 1, 0), w, w + 1, per - 1, per, per + 1]
    return [rng.choice(menu) if rng.random() < 0.6 else rng.randint(0, 4 * w + 40) for _ in range(count)]


def run_sequence(plan, L, M, T, q, sizes, S=0, m=0):
    """Feeds `sizes` from the state (S consumed, m written); returns the final (S, m). The model keeps the history as
    the index range [hs, S) (empty: hs == S) and the samples still to skip."""
    w = -(-T // L)
    assert m == total_outputs(L, M, T, q, S)
    hs = min(first(L, M, q, m), S)
    to_skip = first(L, M, q, m) - hs if hs == S else 0
    for c in sizes:
        n, seam, hist, skip, hist_after, skip_after = plan(L, M, T, q, S, m, c)
        S1 = S + c
        what = (L, M, T, q, S, m, c)
        # brute force: the outputs this call allows, in order; none of them was allowed before
        due = []
        k = m
        while need(L, M, T, q, k) <= S1:
            assert need(L, M, T, q, k) > S, what
            due.append(k)
            k += 1
        assert n == len(due), what
        assert n == total_outputs(L, M, T, q, S1) - total_outputs(L, M, T, q, S), what   # OutputsFor's rule
        # the state the call starts from
        assert hist == S - hs and hist <= max(w - 1, 0), what
        assert skip == min(to_skip, c), what
        assert hist == 0 or to_skip == 0
        # seam outputs start in the history and none before its first sample; direct ones at or after the skip
        assert 0 <= seam <= n, what
        for j, k in enumerate(due):
            f = first(L, M, q, k)
            if j < seam:
                assert hs <= f < S, (what, k)
            else:
                assert f >= S + skip, (what, k)
            assert f >= hs, (what, k)
        # the state it leaves: [first(next output), S1), or empty with the samples still to skip
        m1 = m + n
        f1 = first(L, M, q, m1)
        assert f1 >= hs, what
        if f1 < S1:
            assert (hist_after, skip_after) == (S1 - f1, 0), what
            if f1 < S:   # the tail of the old history and the whole chunk
                assert hist_after == (S - f1) + c and S - f1 <= hist, what
            else:        # the tail of the chunk
                assert hist_after <= c, what
        else:
            assert (hist_after, skip_after) == (0, f1 - S1), what
        assert hist_after <= max(w - 1, 0), what
        S, m = S1, m1
        hs = min(f1, S)
        to_skip = f1 - S if f1 >= S else 0
    return S, m


@pytest.mark.parametrize("L,M,T", SHAPES)
def test_plan_against_brute_force(plan, L, M, T):
    for q in sorted({0, L - 1}):
        rng = random.Random(L * 1000003 + M * 101 + T + q)
        for _ in range(SEQUENCES):
            sizes = chunk_sizes(rng, L, M, T, CHUNKS)
            S, m = run_sequence(plan, L, M, T, q, sizes)
            assert S == sum(sizes) and m == total_outputs(L, M, T, q, S)


def test_plan_where_the_zero_stuffed_index_crosses_2_to_32(plan):
    L, M, T, q = 4096, 4099, 8192, 4095
    cross = -(-((1 << 32) - q) // M)            # the first output with s(m) >= 2^32
    m0 = cross - 150
    S0 = inputs_for(L, M, q, T, m0)             # a state the stream passes through: m0 outputs written
    assert total_outputs(L, M, T, q, S0) == m0
    rng = random.Random(32)
    sizes = chunk_sizes(rng, L, M, T, CHUNKS)
    S, m = run_sequence(plan, L, M, T, q, sizes, S0, m0)
    assert m0 < cross < m and q + (m - 1) * M > 1 << 32


def test_plan_refuses_what_the_object_refuses(plan):
    zero = (0,) * 6
    assert plan(0, 125, 769, 0, 0, 0, 100) == zero
    assert plan(24, 0, 769, 0, 0, 0, 100) == zero
    assert plan(24, 125, 0, 0, 0, 0, 100) == zero
    assert plan(24, 125, 769, 24, 0, 0, 100) == zero
    # phase0 + m M + T leaves 63 bits
    m = (1 << 63) // 125
    assert plan(24, 125, 769, 0, inputs_for(24, 125, 0, 769, m), m, 100) == zero
    assert plan(24, 125, 769, 0, (1 << 64) - 1, 0, 100) == zero          # consumed + chunk leaves 64 bits
    from gsdr_amd.abi import lib

    lib.gsdrxResamplerPlan(24, 125, 769, 0, 0, 0, 100, None)             # a null plan: nothing written


def test_argument_validation_without_device_work():
    from gsdr_amd.abi import lib

    null = None
    dummy = ctypes.c_void_p(16)
    h = ctypes.c_void_p(0xdead)
    ref = ctypes.byref(h)
    # (handle, sampleType, interpolation, decimation, phase, taps, numTaps, device)
    assert lib.gsdrxResamplerCreate(null, 0, 24, 125, 0, dummy, 769, 0) == HIP_ERROR_INVALID_VALUE
    bad = [(2, 24, 125, 0, dummy, 769), (-1, 24, 125, 0, dummy, 769),     # unknown sample type
           (0, 0, 125, 0, dummy, 769), (1, 24, 0, 0, dummy, 769),          # interpolation, decimation == 0
           (0, 24, 125, 24, dummy, 769), (1, 1, 4, 1, dummy, 127),         # phase >= interpolation
           (0, 24, 125, 0, null, 769), (1, 24, 125, 0, dummy, 0)]          # null taps, no taps
    for args in bad:
        h.value = 0xdead
        assert lib.gsdrxResamplerCreate(ref, *args, 0) == HIP_ERROR_INVALID_VALUE, args
        assert not h.value, args                                            # the handle is cleared
    written = ctypes.c_size_t(99)
    assert lib.gsdrxResamplerProcess(null, dummy, 16, dummy, 16, ctypes.byref(written), null) == \
        HIP_ERROR_INVALID_VALUE
    assert written.value == 0
    assert lib.gsdrxResamplerProcess(null, null, 0, null, 0, null, null) == HIP_ERROR_INVALID_VALUE
    assert lib.gsdrxResamplerOutputsFor(null, 100) == 0
    assert lib.gsdrxResamplerDestroy(null) == HIP_SUCCESS
