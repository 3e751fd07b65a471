"""GPU: the streaming rational resampler (gsdrxResampler, include/gsdr/resampler.h; gsdr_amd.stream.Resampler) against
the one-shot call it is the stream form of: concatenated over any cut of a stream into chunks, the outputs are those
of ONE ops.resample call over the whole stream, compared as raw bits.

Every chunk is copied into a buffer of its own, NaN on both sides and starting k elements past a 16-byte boundary (k
cycling over the alignments of the sample type), so a read outside the chunk that reaches an output shows as NaN and
every head / tail path of the staging runs. Outputs go into guarded buffers (helpers.guarded) at element offsets 0 and
1. Tile sizes come from the library's own launch plan, as in test_gpu_resample.py.
"""
import ctypes

import numpy as np
import pytest
import torch

from helpers import check_guards, guarded
from resample_ref import build_plan_program, inputs_for

pytestmark = pytest.mark.gpu

DTYPES = [torch.float32, torch.complex64]
TILE, GENERIC = 0, 1
HIP_ERROR_INVALID_VALUE = 1


@pytest.fixture(scope="module")
def plan_of(tmp_path_factory):
    """plan_of(L, M, T, dtype) -> the library's one-shot plan for that shape (route, kt, ...)."""
    run = build_plan_program(tmp_path_factory.mktemp("resampler_plan_gpu"))
    cache = {}

    def look(L, M, T, dtype):
        key = (L, M, T, 8 if dtype.is_complex else 4, 1)
        if key not in cache:
            cache[key] = run([key])[0]
        return cache[key]

    return look


def dev(a, cuda):
    return torch.from_numpy(np.ascontiguousarray(a)).to(cuda)


def samples(n, cplx, seed):
    rng = np.random.default_rng(seed)
    x = rng.uniform(-1, 1, n).astype(np.float32)
    if cplx:
        x = (x + 1j * rng.uniform(-1, 1, n).astype(np.float32)).astype(np.complex64)
    return x


def taps_of(T, seed):
    rng = np.random.default_rng(1000 + seed)
    return (rng.uniform(0.1, 1.0, T) * rng.choice([-1.0, 1.0], T)).astype(np.float32)


def total_outputs(L, M, T, q, S):
    """The largest N with inputs_for(L, M, q, T, N) <= S."""
    return (S * L - T - q) // M + 1 if S * L >= T + q else 0


def bits(t):
    return (torch.view_as_real(t) if t.is_complex() else t).contiguous().view(torch.int32)


def chunk_input(x_d, lo, hi, k):
    """x_d[lo:hi] in a buffer of its own: NaN on both sides, the view k elements past a 16-byte boundary."""
    g = 16 // x_d.element_size()
    nan = complex(float("nan"), float("nan")) if x_d.is_complex() else float("nan")
    buf = torch.full((2 * g + k + (hi - lo) + 4,), nan, dtype=x_d.dtype, device=x_d.device)
    assert buf.data_ptr() % 16 == 0 and 0 <= k < g
    view = buf[g + k:g + k + hi - lo]
    view.copy_(x_d[lo:hi])
    return view


def feed(cuda, r, x_d, sizes, shape, what=""):
    """Feeds x_d through Resampler r in chunks of `sizes` (clipped to the stream; whatever is left goes last) and
    returns the concatenated outputs. Checks each call's count against the rule, and the guards of every output."""
    L, M, T, q = shape
    g = 16 // x_d.element_size()
    S, parts, call = 0, [], 0
    todo = list(sizes) + [x_d.numel()]
    while todo:
        c = min(todo.pop(0), x_d.numel() - S)
        want = total_outputs(L, M, T, q, S + c) - total_outputs(L, M, T, q, S)
        assert r.outputs_for(c) == want, (what, S, c)
        buf, out = guarded(cuda, x_d.dtype, want, call % 2)
        got = r.process(chunk_input(x_d, S, S + c, call % g), out=out)
        assert got.numel() == want and (want == 0 or got.data_ptr() == out.data_ptr())
        check_guards(buf, out, what=f"{what} call {call}: {c} samples at {S}")
        parts.append(out)
        S += c
        call += 1
        if S == x_d.numel():
            break
    assert S == x_d.numel()
    return torch.cat(parts)


def samples_for(L, M, T, q, S, n):
    """The smallest chunk after S consumed samples that brings n more outputs (exactly n when M >= L)."""
    return max(inputs_for(L, M, q, T, total_outputs(L, M, T, q, S) + n) - S, 0)


def schedule_a(L, M, T, q, kt):
    """0, 1, 1, 2, 3, w - 1, w, w + 1 samples, then the samples for exactly 1, kt - 1, kt and kt + 1 outputs."""
    w = -(-T // L)
    sizes = [0, 1, 1, 2, 3, max(w - 1, 0), w, w + 1]
    S = sum(sizes)
    for n in (1, kt - 1, kt, kt + 1):
        c = samples_for(L, M, T, q, S, n)
        if M >= L:
            assert total_outputs(L, M, T, q, S + c) - total_outputs(L, M, T, q, S) == n
        sizes.append(c)
        S += c
    return sizes


def schedule_b(total, seed):
    """Fifty 1-sample chunks, then seeded random sizes (about twenty chunks, some of them tiny)."""
    rng = np.random.default_rng(seed)
    sizes = [1] * 50
    while sum(sizes) < total:
        sizes.append(int(rng.integers(0, 4)) if rng.random() < 0.25 else int(rng.integers(1, max(2, total // 10))))
    return sizes


TILE_SHAPES = [(24, 125, 769), (160, 147, 1601), (4, 1, 65), (125, 24, 2000), (5, 6, 23), (24, 125, 1), (24, 125, 23),
               (24, 125, 24)]
GENERIC_SHAPES = [(3, 2, 20000, 1100), (2, 100001, 7, 600)]


@pytest.mark.parametrize("dtype", DTYPES, ids=["FF", "FC"])
@pytest.mark.parametrize("L,M,T,fixed_n", [s + (None,) for s in TILE_SHAPES] + GENERIC_SHAPES + [(1, 4, 127, None)])
def test_chunked_equals_monolithic(cuda, plan_of, L, M, T, fixed_n, dtype):
    from gsdr_amd import ops
    from gsdr_amd.stream import Resampler

    p = plan_of(L, M, T, dtype)
    if L > 1:
        assert p["route"] == (GENERIC if fixed_n else TILE), (L, M, T)
    kt = p["kt"]
    h_d = dev(taps_of(T, T), cuda)
    for q in sorted({0, L - 1}):
        sizes_a = schedule_a(L, M, T, q, kt)
        # 3 kt + 37 outputs, and where L > M (schedule (a)'s first chunks already bring outputs) enough for all of (a)
        N = fixed_n or max(3 * kt + 37, total_outputs(L, M, T, q, sum(sizes_a)) + 37)
        x_d = dev(samples(inputs_for(L, M, q, T, N), dtype.is_complex, seed=L * M + T + q), cuda)
        S = x_d.numel()
        total = total_outputs(L, M, T, q, S)   # N, or a few more where several outputs end on one sample (L > M)
        assert N <= total < N + L and inputs_for(L, M, q, T, total) <= S < inputs_for(L, M, q, T, total + 1)
        if L == 1:
            whole = ops.fir(h_d, x_d, M, total)
        else:
            whole = ops.resample(h_d, x_d, L, M, q, total)
        for name, sizes in (("a", sizes_a), ("b", schedule_b(S, seed=T + q))):
            what = f"L={L} M={M} T={T} q={q} {dtype} schedule {name}"
            r = Resampler(h_d, L, M, q, complex_samples=dtype.is_complex)
            try:
                got = feed(cuda, r, x_d, sizes, (L, M, T, q), what)
            finally:
                torch.cuda.synchronize()
                r.close()
            assert got.numel() == total, what
            assert torch.equal(bits(got), bits(whole)), what


@pytest.mark.parametrize("dtype", DTYPES, ids=["FF", "FC"])
def test_non_finite_samples_across_seams(cuda, plan_of, dtype):
    """+Inf, -Inf and NaN where a seam can mishandle them: as the last sample of a kept history, and as the first
    sample of a chunk. The NaN / +-Inf pattern equals the one-shot call's, and every finite output its bits."""
    from gsdr_amd import ops
    from gsdr_amd.stream import Resampler, resampler_plan

    L, M, T, q = 24, 125, 99, 7
    N = 3 * plan_of(L, M, T, dtype)["kt"] + 37
    x = samples(inputs_for(L, M, q, T, N), dtype.is_complex, seed=99)
    rng = np.random.default_rng(5)
    sizes = [int(rng.integers(1, x.size // 15)) for _ in range(60)]   # about thirty of them span the stream
    # the stream's seams and the history kept at each, from the plan
    seams, S, m = [], 0, 0
    for c in sizes:
        if S + c >= x.size:
            break
        pl = resampler_plan(L, M, T, q, S, m, c)
        S, m = S + c, m + pl[0]
        seams.append((S, pl[4]))
    kept = [s for s, hist in seams if hist >= 1][::3][:6]
    heads = [s for s, hist in seams if s not in kept][::3][:6]
    assert len(kept) >= 3 and len(heads) >= 3
    bad = [np.inf, -np.inf, np.nan]
    for k, s in enumerate(kept):
        x[s - 1] = bad[k % 3] if not dtype.is_complex else complex(bad[k % 3], 0.5)      # the history's last sample
    for k, s in enumerate(heads):
        x[s] = bad[(k + 1) % 3] if not dtype.is_complex else complex(-0.25, bad[(k + 1) % 3])  # a chunk's first
    h_d, x_d = dev(taps_of(T, 17), cuda), dev(x, cuda)
    whole = ops.resample(h_d, x_d, L, M, q, N)
    r = Resampler(h_d, L, M, q, complex_samples=dtype.is_complex)
    try:
        got = feed(cuda, r, x_d, sizes, (L, M, T, q), f"non-finite {dtype}")
    finally:
        torch.cuda.synchronize()
        r.close()
    assert got.numel() == N
    g, w = torch.view_as_real(got) if dtype.is_complex else got, torch.view_as_real(whole) if dtype.is_complex else whole
    assert torch.equal(torch.isnan(g), torch.isnan(w))
    assert torch.equal(torch.isposinf(g), torch.isposinf(w)) and torch.equal(torch.isneginf(g), torch.isneginf(w))
    finite = torch.isfinite(w)
    assert finite.sum() > finite.numel() // 2 and torch.isnan(w).any() and torch.isinf(w).any()
    assert torch.equal(g[finite].view(torch.int32), w[finite].view(torch.int32))


@pytest.mark.parametrize("dtype", DTYPES, ids=["FF", "FC"])
def test_capacity_and_retry(cuda, plan_of, dtype):
    """A call that is refused (capacity one short, a missing output, a missing input) leaves the object unchanged: the
    same chunk passed again with room continues the stream bit for bit."""
    from gsdr_amd import ops
    from gsdr_amd.abi import lib
    from gsdr_amd.stream import Resampler

    L, M, T, q = 24, 125, 769, 5
    N = 3 * plan_of(L, M, T, dtype)["kt"] + 37
    h_d = dev(taps_of(T, 3), cuda)
    x_d = dev(samples(inputs_for(L, M, q, T, N), dtype.is_complex, seed=31), cuda)
    whole = ops.resample(h_d, x_d, L, M, q, N)
    r = Resampler(h_d, L, M, q, complex_samples=dtype.is_complex)
    try:
        a, b = 5001, 17000
        first = r.process(x_d[:a])
        chunk = x_d[a:b]
        due = r.outputs_for(chunk.numel())
        assert due > 1
        buf, out = guarded(cuda, dtype, due, 1)
        written = ctypes.c_size_t(77)
        stream = torch.cuda.current_stream(cuda).cuda_stream
        for inp, outp, cap in ((chunk.data_ptr(), out.data_ptr(), due - 1), (chunk.data_ptr(), None, due),
                               (None, out.data_ptr(), due)):
            assert lib.gsdrxResamplerProcess(r._h, inp, chunk.numel(), outp, cap, ctypes.byref(written), stream) == \
                HIP_ERROR_INVALID_VALUE
            assert written.value == 0 and r.outputs_for(chunk.numel()) == due
        check_guards(buf, out[:0], what="refused calls wrote nothing")
        second = r.process(chunk, out=out)
        check_guards(buf, out, what="the retried chunk")
        third = r.process(x_d[b:])
        got = torch.cat([first, second, third])
    finally:
        torch.cuda.synchronize()
        r.close()
    assert got.numel() == N and torch.equal(bits(got), bits(whole))


def test_past_2_to_32_in_the_zero_stuffed_index(cuda, plan_of):
    """The shape of test_gpu_resample.py's case of this name, fed in chunks of 2^16 + 13 samples: seams on either side
    of the output where s(m) crosses 2^32."""
    from gsdr_amd import ops
    from gsdr_amd.stream import Resampler

    L, M, T, N, q = 4096, 4099, 8192, (1 << 20) + 1024, 4095
    assert plan_of(L, M, T, torch.float32)["route"] == TILE
    h_d = dev(taps_of(T, 13), cuda)
    x_d = dev(samples(inputs_for(L, M, q, T, N), False, seed=32), cuda)
    S, step = x_d.numel(), (1 << 16) + 13
    cross = -(-((1 << 32) - q) // M)   # the first output with s(m) >= 2^32
    at = inputs_for(L, M, q, T, cross + 1)   # samples that output needs: the call that reaches them writes it
    seams = range(step, S, step)
    assert 0 < cross < N - 1 and seams[0] < at <= seams[-1]
    whole = ops.resample(h_d, x_d, L, M, q, N)
    r = Resampler(h_d, L, M, q)
    try:
        parts = [r.process(x_d[lo:lo + step]) for lo in range(0, S, step)]
    finally:
        torch.cuda.synchronize()
        r.close()
    got = torch.cat(parts)
    assert got.numel() == N and sum(p.numel() > 0 for p in parts) >= 16
    assert torch.equal(bits(got), bits(whole))


def test_receiver_chain(cuda):
    """Stream("fm", decimation 4) feeding Resampler(24 / 125, 769 taps) chunk by chunk, 2^14 RF samples a chunk,
    against ops.fm_demod over the whole input followed by one ops.resample."""
    from gsdr_amd import ops
    from gsdr_amd.signals import lowpass_taps
    from gsdr_amd.stream import Resampler, Stream

    fs, tune, chan, devi, D = 1.0e6, 0.0, 1.0e5, 2.0e4, 4
    L, M, T = 24, 125, 769
    rf_taps = dev(lowpass_taps(127, 0.4 / D).astype(np.float32), cuda)
    h_d = dev((lowpass_taps(T, 0.4 / M) * L).astype(np.float32), cuda)
    n_chunks, size = 12, 1 << 14
    rf = dev(samples(n_chunks * size, True, seed=41), cuda)
    audio = ops.fm_demod(rf, rf_taps, fs, tune, chan, devi, D)
    whole = ops.resample(h_d, audio, L, M)
    assert whole.numel() > 3 * 2048
    fm = Stream("fm", rf_taps, D, fs, tune, chan, devi)
    rs = Resampler(h_d, L, M)
    try:
        parts = [rs.process(fm.process(rf[k * size:(k + 1) * size])) for k in range(n_chunks)]
    finally:
        torch.cuda.synchronize()
        fm.close()
        rs.close()
    got = torch.cat(parts)
    assert got.numel() == whole.numel()
    assert torch.equal(bits(got), bits(whole))
