"""GPU: the polyphase rational resampler (gsdrxResampleFF / FC, gsdr_ext.h) against the float64 reference of
resample_ref.py (tied to the oracle by test_resample_host.py).

Bars: normwise 1e-5 against S_m = sum |h| |x| over the products of the definition, strict (an output with an empty
window must be exactly zero); every cut of a stream into calls, and interpolation == 1 against gsdrFirFF / FC, bit
for bit. Every output is written into the middle of a sentinel-filled buffer, at element offsets 0 and 1, whose
guards must stay untouched. Tile sizes come from the library's own launch plan (resample_plan.hpp, compiled into a
host program as in test_resample_plan.py), so the sizes here follow the plan if it changes.
"""
import numpy as np
import pytest
import torch

from helpers import FLOAT_TOL, check_guards, guarded, normwise_err_strict
from resample_ref import build_plan_program, continuation, inputs_for, resample_bound, resample_ref

pytestmark = pytest.mark.gpu

RATIOS = [(2, 1), (4, 1), (3, 2), (2, 3), (5, 6), (24, 125), (125, 24), (147, 160), (160, 147), (7, 3)]
DTYPES = [torch.float32, torch.complex64]
TILE, GENERIC = 0, 1


def tap_counts(L):
    return [1, L - 1, L, 4 * L + 3, 16 * L]


@pytest.fixture(scope="module")
def plan_of(tmp_path_factory):
    """plan_of(L, M, T, dtype) -> the library's plan for that shape (route, kt, ...)."""
    run = build_plan_program(tmp_path_factory.mktemp("resample_plan_gpu"))
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
    """Taps of both signs, none of them zero (a zero tap would hide a product that should not be formed)."""
    rng = np.random.default_rng(1000 + seed)
    return (rng.uniform(0.1, 1.0, T) * rng.choice([-1.0, 1.0], T)).astype(np.float32)


def guarded_call(cuda, h_d, x_d, L, M, q, N, off=0):
    """ops.resample into a guarded buffer `off` elements past its 16-byte alignment; returns the output tensor (on the
    device) after checking the guards."""
    from gsdr_amd import ops

    buf, out = guarded(cuda, x_d.dtype, N, off)
    got = ops.resample(h_d, x_d, L, M, q, N, out=out)
    assert got.data_ptr() == out.data_ptr()
    check_guards(buf, out, what=f"resample L={L} M={M} T={h_d.numel()} q={q} N={N} off={off}")
    return out


def parity(cuda, h, x, L, M, q, N, off=0, x_d=None, label=""):
    x_d = dev(x, cuda) if x_d is None else x_d
    got = guarded_call(cuda, dev(h, cuda), x_d, L, M, q, N, off).cpu().numpy()
    ref = resample_ref(h, x, L, M, q, N)
    err = normwise_err_strict(got, ref, resample_bound(h, x, L, M, q, N))
    print(f"resample parity {label} L={L} M={M} T={h.size} q={q} N={N} {x.dtype}: normwise error {err:.3e} "
          f"(bar {FLOAT_TOL:.1e})")
    assert err <= FLOAT_TOL, (L, M, h.size, q, N, err)
    return got


@pytest.mark.parametrize("dtype", DTYPES, ids=["FF", "FC"])
@pytest.mark.parametrize("L,M", RATIOS)
def test_parity_matrix(cuda, plan_of, L, M, dtype):
    """T in {1, L - 1, L, 4 L + 3, 16 L} x q in {0, L / 2, L - 1}, three of the shape's tiles plus 37 outputs: a ragged
    tail and more than one tile boundary. T = L - 1 leaves empty windows, which must be exactly +0."""
    case = 0
    for T in tap_counts(L):
        p = plan_of(L, M, T, dtype)
        assert p["route"] == TILE, (L, M, T)
        N = 3 * p["kt"] + 37
        h = taps_of(T, T)
        for q in sorted({0, L // 2, L - 1}):
            x = samples(inputs_for(L, M, q, T, N), dtype.is_complex, seed=L * M + T + q)
            got = parity(cuda, h, x, L, M, q, N, off=case % 2)
            if T < L:
                empty = resample_bound(h, x, L, M, q, N) == 0
                assert empty.any()
                assert not np.signbit(got[empty].real).any() and not np.signbit(got[empty].imag).any()
            case += 1


@pytest.mark.parametrize("dtype,offsets", [(torch.float32, (1, 2, 3)), (torch.complex64, (1,))], ids=["FF", "FC"])
def test_parity_input_views_off_16_byte_alignment(cuda, plan_of, dtype, offsets):
    """The input a view 1, 2, 3 floats (4, 8, 12 bytes) or 1 complex sample (8 bytes) past a 16-byte boundary: the
    staging's head / tail path."""
    L, M, T, q = 24, 125, 4 * 24 + 3, 7
    N = 3 * plan_of(L, M, T, dtype)["kt"] + 37
    h = taps_of(T, 5)
    x = samples(inputs_for(L, M, q, T, N), dtype.is_complex, seed=77)
    want = None
    for k in (0,) + offsets:
        base = torch.zeros(x.size + 4, dtype=dtype, device=cuda)
        assert base.data_ptr() % 16 == 0
        view = base[k:k + x.size]
        view.copy_(dev(x, cuda))
        assert view.data_ptr() % 16 == (k * x.itemsize) % 16
        got = parity(cuda, h, x, L, M, q, N, off=k % 2, x_d=view, label=f"input +{k}")
        want = got if want is None else want
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), k   # the alignment changes no bit


@pytest.mark.parametrize("dtype", DTYPES, ids=["FF", "FC"])
@pytest.mark.parametrize("M", [1, 4, 5])
def test_interpolation_1_is_the_fir_bit_for_bit(cuda, M, dtype):
    from gsdr_amd import ops

    T, N = 127, 5000
    h = dev(taps_of(T, 3), cuda)
    x = dev(samples((N - 1) * M + T, dtype.is_complex, seed=M), cuda)
    assert ops.resample_inputs_for(1, M, 0, T, N) == x.numel()
    got = guarded_call(cuda, h, x, 1, M, 0, N, off=M % 2)
    want = ops.fir(h, x, M, N)
    torch.cuda.synchronize()
    assert torch.equal(got.view(torch.int32), want.view(torch.int32))


def split_is_bit_identical(cuda, h, x, L, M, phase0, N, cuts):
    h_d, x_d = dev(h, cuda), dev(x, cuda)
    whole = guarded_call(cuda, h_d, x_d, L, M, phase0, N)
    edges = [0] + sorted(set(c for c in cuts if 0 < c < N)) + [N]
    parts = []
    for k, (a, b) in enumerate(zip(edges, edges[1:])):
        first, q = continuation(phase0, a, L, M)
        need = inputs_for(L, M, q, h.size, b - a)
        assert first + need <= x.size
        parts.append(guarded_call(cuda, h_d, x_d[first:first + need], L, M, q, b - a, off=k % 2))
    got = torch.cat(parts)
    torch.cuda.synchronize()
    assert torch.equal(got.view(torch.int32), whole.view(torch.int32)), (L, M, h.size, phase0, edges)
    return whole


@pytest.mark.parametrize("dtype", DTYPES, ids=["FF", "FC"])
@pytest.mark.parametrize("L,M,T", [(24, 125, 769), (160, 147, 1601), (3, 2, 20000)])
def test_split_invariance(cuda, plan_of, L, M, T, dtype):
    """One call against the same stream cut at outputs {1, 255, 256, 1000, N - 1} through continuation(): the raw bits.
    The advanced input pointers fall at every 4- / 8-byte alignment. (3, 2, 20000) runs the generic kernel."""
    p = plan_of(L, M, T, dtype)
    assert p["route"] == (GENERIC if T == 20000 else TILE)
    N = 3 * p["kt"] + 37 if p["route"] == TILE else 1100
    h = taps_of(T, 9)
    for phase0 in (0, L - 1):
        x = samples(inputs_for(L, M, phase0, T, N), dtype.is_complex, seed=T + phase0)
        split_is_bit_identical(cuda, h, x, L, M, phase0, N, [1, 255, 256, 1000, N - 1])


@pytest.mark.parametrize("dtype", DTYPES, ids=["FF", "FC"])
@pytest.mark.parametrize("L,M,T,N", [(3, 2, 20000, 300), (2, 100001, 7, 600)])
def test_generic_route(cuda, plan_of, L, M, T, N, dtype):
    """80 KB of taps, and about 50,000 input samples an output: neither fits a tile's LDS."""
    assert plan_of(L, M, T, dtype)["route"] == GENERIC
    q = L - 1
    x = samples(inputs_for(L, M, q, T, N), dtype.is_complex, seed=T)
    parity(cuda, taps_of(T, 11), x, L, M, q, N, off=1)


def test_past_2_to_32_in_the_zero_stuffed_index(cuda, plan_of):
    """L = 4096, M = 4099: N M > 2^32 with about 1.05 M input samples. Every output against the reference, and a cut at
    the output where s(m) crosses 2^32 bit for bit. The shape runs the tiled kernel."""
    L, M, T, N, q = 4096, 4099, 8192, (1 << 20) + 1024, 4095
    assert plan_of(L, M, T, torch.float32)["route"] == TILE
    assert q + (N - 1) * M > 1 << 32
    h = taps_of(T, 13)
    x = samples(inputs_for(L, M, q, T, N), False, seed=32)
    assert x.size < 1.06 * (1 << 20)
    cross = -(-((1 << 32) - q) // M)   # the first output with s(m) >= 2^32
    assert 0 < cross < N - 1 and q + (cross - 1) * M < 1 << 32 <= q + cross * M
    whole = split_is_bit_identical(cuda, h, x, L, M, q, N, [cross]).cpu().numpy()
    ref = resample_ref(h, x, L, M, q, N)
    err = normwise_err_strict(whole, ref, resample_bound(h, x, L, M, q, N))
    print(f"resample past 2^32: normwise error {err:.3e} (bar {FLOAT_TOL:.1e}), cut at output {cross}")
    assert err <= FLOAT_TOL


@pytest.mark.parametrize("dtype", DTYPES, ids=["FF", "FC"])
@pytest.mark.parametrize("L,M,T", [(3, 2, 10), (24, 125, 4 * 24 + 3), (5, 6, 23)])
def test_non_finite_samples_stay_in_their_windows(cuda, plan_of, L, M, T, dtype):
    """+-Inf and NaN at sparse positions, T no multiple of L: some windows take ceil(T / L) samples and some one
    fewer, so a non-finite sample sits right behind the last sample a window reads. The NaN / Inf pattern and the
    infinities' signs equal the reference's; finite outputs meet the bar."""
    assert T % L != 0
    N = plan_of(L, M, T, dtype)["kt"] + 300
    q = L // 2
    h = taps_of(T, 17)
    x = samples(inputs_for(L, M, q, T, N), dtype.is_complex, seed=99)
    m = np.arange(N, dtype=np.int64)
    s = q + m * M
    i0 = (L - s % L) % L
    n0 = (s + i0) // L
    count = np.where(i0 < T, -(-(T - i0) // L), 0)    # samples output m reads
    short = np.flatnonzero(count == T // L)           # windows one sample shorter than the longest
    assert short.size and (count == T // L + 1).any()
    # the first sample a short window does not read, and the last sample one reads, far enough apart that most
    # windows stay finite
    bad = [np.inf, -np.inf, np.nan]
    stride = max(1, short.size // 12)
    for k, mm in enumerate(short[::stride][:12]):
        at = n0[mm] + count[mm] - (k % 2)   # even k: just behind the window; odd k: its last sample
        if at < x.size:
            x[at] = bad[k % 3] if not dtype.is_complex else complex(bad[k % 3], 1.0) if k % 4 < 2 else complex(0.5, bad[k % 3])
    got = guarded_call(cuda, dev(h, cuda), dev(x, cuda), L, M, q, N, off=1).cpu().numpy()
    with np.errstate(invalid="ignore", over="ignore"):
        ref = resample_ref(h, x, L, M, q, N)
    parts = [(got.real, ref.real), (got.imag, ref.imag)] if dtype.is_complex else [(got, ref)]
    for g, r in parts:
        assert np.array_equal(np.isnan(g), np.isnan(r))
        assert np.array_equal(np.isposinf(g), np.isposinf(r)) and np.array_equal(np.isneginf(g), np.isneginf(r))
    finite = np.isfinite(ref)
    assert finite.sum() > N // 2 and (~finite).any()
    # a short window right in front of a non-finite sample stayed finite in the reference: the case is exercised
    behind = [mm for mm in short if n0[mm] + count[mm] < x.size and not np.isfinite(x[n0[mm] + count[mm]])]
    assert any(finite[mm] for mm in behind)
    xf = np.where(np.isfinite(x), x, 0)
    sb = resample_bound(h, xf, L, M, q, N)
    err = normwise_err_strict(got[finite], ref[finite], sb[finite])
    print(f"resample non-finite L={L} M={M} T={T} {x.dtype}: finite outputs' normwise error {err:.3e}")
    assert err <= FLOAT_TOL


@pytest.mark.parametrize("dtype", DTYPES, ids=["FF", "FC"])
def test_edges(cuda, dtype):
    from gsdr_amd import ops

    L, M, q = 3, 2, 1
    x = dev(samples(4000, dtype.is_complex, seed=5), cuda)
    # no taps: zeros, inside the guards
    none = torch.empty(0, dtype=torch.float32, device=cuda)
    for off in (0, 1):
        out = guarded_call(cuda, none, x, L, M, q, 1000, off)
        assert torch.equal(out.view(torch.int32), torch.zeros_like(out).view(torch.int32))
    # one output
    h = taps_of(31, 1)
    xs = x[:inputs_for(L, M, q, 31, 1)]
    got = guarded_call(cuda, dev(h, cuda), xs, L, M, q, 1, off=1).cpu().numpy()
    xn = xs.cpu().numpy()
    assert normwise_err_strict(got, resample_ref(h, xn, L, M, q, 1), resample_bound(h, xn, L, M, q, 1)) <= FLOAT_TOL
    # no outputs: success, nothing written
    buf, out = guarded(cuda, dtype, 16, 0)
    ops.resample(dev(h, cuda), x, L, M, q, 0, out=out[:0])
    check_guards(buf, out[:0], what="no outputs")
    # num_outputs defaults to the most the input supports: one more would need more input
    y = ops.resample(dev(h, cuda), x, L, M, q)
    assert inputs_for(L, M, q, 31, y.numel()) <= x.numel() < inputs_for(L, M, q, 31, y.numel() + 1)
    # a short input raises before any call
    with pytest.raises(ValueError):
        ops.resample(dev(h, cuda), x[:-1], L, M, q, y.numel() + 1)
    with pytest.raises(ValueError):
        ops.resample(dev(h, cuda), x, L, M, L)


def test_known_answer_250_khz_to_48_khz(cuda):
    """A 1 kHz sine at 250 kHz through L / M = 24 / 125 (48 kHz out) and a 769-tap Hamming-windowed sinc, cutoff
    20 kHz at the 6 MHz rate, taps summing to L: output m is sin(2 pi 1000 (m M + 384) / 6e6) within 1e-3. The float64
    evaluation of this design is off by 5.8e-4 (the filter's own ripple; asserted below), the fp32 bar adds at most
    1e-5 S with S <= 1.3, and the rest is margin."""
    L, M, T, N = 24, 125, 769, 3 * 1024 + 37
    i = np.arange(T) - (T - 1) // 2
    h = np.sinc(2 * 20e3 / 6e6 * i) * np.hamming(T)
    h = (h * L / h.sum()).astype(np.float32)
    x = np.sin(2 * np.pi * 1000.0 * np.arange(inputs_for(L, M, 0, T, N)) / 250e3).astype(np.float32)
    want = np.sin(2 * np.pi * 1000.0 * (np.arange(N) * M + 384) / 6e6)
    design = float(np.max(np.abs(resample_ref(h, x, L, M, 0, N) - want)))
    assert design <= 6e-4, design
    got = guarded_call(cuda, dev(h, cuda), dev(x, cuda), L, M, 0, N).cpu().numpy()
    err = float(np.max(np.abs(got - want)))
    print(f"resample known answer: max error {err:.3e} (design {design:.3e}, bar 1e-3)")
    assert err <= 1e-3
