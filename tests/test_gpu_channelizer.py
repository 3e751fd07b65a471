"""GPU: the polyphase filter bank (gsdrxChannelizer, gsdr_ext.h) against the float64 term-by-term reference of
channelizer_ref.py (tied to the oracle by test_channelizer_host.py).

Bars: normwise FLOAT_TOL (1e-5) against S_m = sum |h| |x| over output time m's window, for every channel, strict;
every cut of a stream into calls, every input alignment and int8 against converted input, bit for bit. An fp32
restatement of the computation (sequential branch sums, complex64 FFT, rotation) stays below 1e-7 of S against the
float64 definition (the kernels measure up to 1.6e-7, in the one-tap cases), so the bar holds with room. Every call writes into the middle of a sentinel-filled
buffer of M N elements, at element offsets 0 and 1, whose guards must stay untouched. Tile sizes come from the
library's own launch plan (channelizer_plan.hpp, compiled into a host program as in test_channelizer_plan.py).
"""
import numpy as np
import pytest
import torch

from channelizer_ref import build_plan_program, channelizer_bound, channelizer_ref, int8_to_float
from helpers import FLOAT_TOL, check_guards, guarded, normwise_err_strict

pytestmark = pytest.mark.gpu

BANKS = [2, 4, 8, 16, 32, 64]
FORMATS = ["CF32", "CS8"]
TILE, GENERIC = 0, 1


@pytest.fixture(scope="module")
def plan_of(tmp_path_factory):
    """plan_of(M, D, T) -> the library's plan for that shape (route, kt, ...)."""
    run = build_plan_program(tmp_path_factory.mktemp("channelizer_plan_gpu"))
    cache = {}

    def look(M, D, T):
        key = (M, D, T, 1)
        if key not in cache:
            cache[key] = run([key])[0]
        return cache[key]

    return look


def dev(a, cuda):
    return torch.from_numpy(np.ascontiguousarray(a)).to(cuda)


def samples(n, fmt, seed):
    """n samples as the call takes them: complex64 in [-1, 1)^2, or 2 n interleaved int8 (-128 included)."""
    rng = np.random.default_rng(seed)
    if fmt == "CS8":
        return rng.integers(-128, 128, 2 * n, dtype=np.int8)
    return (rng.random(2 * n, dtype=np.float32) * np.float32(2) - np.float32(1)).view(np.complex64)


def values(x):
    """The complex64 samples the kernel computes on."""
    return int8_to_float(x) if x.dtype == np.int8 else x


def per(x):
    return 2 if x.dtype in (np.int8, torch.int8) else 1   # elements a sample


def taps_of(T, seed):
    """Taps of both signs, none of them zero (a zero tap would hide a product that should not be formed)."""
    rng = np.random.default_rng(1000 + seed)
    return (rng.uniform(0.1, 1.0, T) * rng.choice([-1.0, 1.0], T)).astype(np.float32)


def guarded_call(cuda, h_d, x_d, M, D, n0, N, off=0):
    """ops.channelizer into a guarded buffer of M N elements `off` elements past its 16-byte alignment; returns the
    (M, N) output tensor (on the device) after checking the guards."""
    from gsdr_amd import ops

    buf, flat = guarded(cuda, torch.complex64, M * N, off)
    out = flat.view(M, N)
    got = ops.channelizer(x_d, h_d, M, D, n0, N, out=out)
    assert got.data_ptr() == out.data_ptr()
    check_guards(buf, flat, what=f"channelizer M={M} D={D} T={h_d.numel()} n0={n0} N={N} off={off}")
    return out


def channel_errors(got, ref, s):
    return max(normwise_err_strict(got[c], ref[c], s) for c in range(ref.shape[0]))


def parity(cuda, h, x, M, D, n0, N, off=0, x_d=None, label=""):
    x_d = dev(x, cuda) if x_d is None else x_d
    got = guarded_call(cuda, dev(h, cuda), x_d, M, D, n0, N, off).cpu().numpy()
    xv = values(x)
    err = channel_errors(got, channelizer_ref(h, xv, M, D, n0, N), channelizer_bound(h, xv, D, N))
    print(f"channelizer parity {label} M={M} D={D} T={h.size} n0={n0} N={N} {x.dtype}: normwise error {err:.3e} "
          f"(bar {FLOAT_TOL:.1e})")
    assert err <= FLOAT_TOL, (M, D, h.size, n0, N, err)
    return got


@pytest.mark.parametrize("fmt", FORMATS)
@pytest.mark.parametrize("M", BANKS)
def test_parity_matrix(cuda, plan_of, M, fmt):
    """D in {M, M / 2} x T in {1, M - 1, M, 4 M + 3, 8 M} x n0 in {0, 12345}, three of the shape's tiles plus 37
    output times: a ragged tail and more than one tile boundary. Every one runs the tiled kernel."""
    case = 0
    worst = 0.0
    for D in sorted({M, max(1, M // 2)}):
        for T in [1, M - 1, M, 4 * M + 3, 8 * M]:
            p = plan_of(M, D, T)
            assert p["route"] == TILE, (M, D, T)
            N = 3 * p["kt"] + 37
            h = taps_of(T, T)
            x = samples((N - 1) * D + T, fmt, seed=M * D + T)
            x_d = dev(x, cuda)
            xv = values(x)
            s = channelizer_bound(h, xv, D, N)
            for n0 in (0, 12345):
                got = guarded_call(cuda, dev(h, cuda), x_d, M, D, n0, N, off=case % 2).cpu().numpy()
                err = channel_errors(got, channelizer_ref(h, xv, M, D, n0, N), s)
                print(f"channelizer parity M={M} D={D} T={T} n0={n0} N={N} {fmt}: normwise error {err:.3e}")
                assert err <= FLOAT_TOL, (M, D, T, n0, fmt, err)
                worst = max(worst, err)
                case += 1
    print(f"channelizer parity matrix M={M} {fmt}: worst normwise error {worst:.3e} (bar {FLOAT_TOL:.1e})")


@pytest.mark.parametrize("fmt", FORMATS)
@pytest.mark.parametrize("M,D,T,N", [(4, 3, 33, 1100), (16, 5, 127, 1100), (64, 48, 300, 600), (8, 1, 64, 1100),
                                     (8, 8, 20000, 600), (8, 100001, 7, 600)])
def test_generic_route(cuda, plan_of, M, D, T, N, fmt):
    """Decimations outside {M, M / 2} (r0 varies with m), 160 KB of samples a window, and windows 100001 samples
    apart: one output time a thread from global memory."""
    assert plan_of(M, D, T)["route"] == GENERIC
    x = samples((N - 1) * D + T, fmt, seed=T)
    parity(cuda, taps_of(T, 11), x, M, D, 7, N, off=1, label="generic")


@pytest.mark.parametrize("fmt", FORMATS)
def test_rows_against_the_single_channel_call(cuda, plan_of, fmt):
    """Row c against ops.xlating_fir(fs = 16, tune = 0, chan = c): two results each within the bar of the same value
    differ by at most twice the bar."""
    from gsdr_amd import ops

    M, D, T, n0 = 16, 8, 127, 12345
    N = 3 * plan_of(M, D, T)["kt"] + 37
    h = taps_of(T, 3)
    x = samples((N - 1) * D + T, fmt, seed=21)
    h_d, x_d = dev(h, cuda), dev(x, cuda)
    got = guarded_call(cuda, h_d, x_d, M, D, n0, N).cpu().numpy()
    s = channelizer_bound(h, values(x), D, N)
    worst = 0.0
    for c in range(M):
        one = ops.xlating_fir(x_d, h_d, 16.0, 0.0, float(c), D, n0, N).cpu().numpy()
        worst = max(worst, normwise_err_strict(got[c], one, s))
    print(f"channelizer against xlating_fir {fmt}: worst normwise difference {worst:.3e} (bar {2 * FLOAT_TOL:.1e})")
    assert worst <= 2 * FLOAT_TOL


@pytest.mark.parametrize("M,D,T", [(16, 8, 127), (64, 64, 512)])
def test_int8_is_the_converted_input_bit_for_bit(cuda, plan_of, M, D, T):
    from gsdr_amd import ops

    N = 3 * plan_of(M, D, T)["kt"] + 37
    h_d = dev(taps_of(T, 4), cuda)
    x8 = dev(samples((N - 1) * D + T, "CS8", seed=M), cuda)
    xf = ops.int8_to_norm_float(x8)
    assert xf.dtype == torch.float32 and xf.numel() == x8.numel()
    a = guarded_call(cuda, h_d, x8, M, D, 12345, N)
    b = guarded_call(cuda, h_d, torch.view_as_complex(xf.view(-1, 2)), M, D, 12345, N, off=1)
    torch.cuda.synchronize()
    assert torch.equal(torch.view_as_real(a).view(torch.int32), torch.view_as_real(b).view(torch.int32))


def shifted(x, shift, cuda):
    """x on the device as a view `shift` samples past a 16-byte boundary."""
    e = per(x)
    base = torch.zeros(x.size + 16 * e, dtype=torch.from_numpy(x[:1]).dtype, device=cuda)
    assert base.data_ptr() % 16 == 0
    view = base[shift * e:shift * e + x.size]
    view.copy_(dev(x, cuda))
    return view


def bits(t):
    return torch.view_as_real(t.contiguous()).view(torch.int32)


@pytest.mark.parametrize("fmt", FORMATS)
@pytest.mark.parametrize("M,D,T", [(16, 8, 127), (64, 64, 512), (16, 5, 127), (8, 8, 20000)])
def test_split_invariance(cuda, plan_of, M, D, T, fmt):
    """One call against the same stream cut at output times {1, 255, 256, 1000, N - 1}, the call whose first output is
    a given input + a D and firstSampleIndex + a D: the raw bits. Each part's input sits at its own offset from a
    16-byte boundary, every 8-byte (CF32) / 2-byte (CS8) alignment among them. (16, 5, 127) and (8, 8, 20000) run
    the generic kernel."""
    p = plan_of(M, D, T)
    assert p["route"] == (GENERIC if (D == 5 or T == 20000) else TILE)
    N = max(3 * p["kt"] + 37, 1137)
    h_d = dev(taps_of(T, 9), cuda)
    granule = 8 if fmt == "CS8" else 2      # samples in 16 bytes
    seen = set()
    for n0 in (0, 3):
        x = samples((N - 1) * D + T, fmt, seed=T + n0)
        e = per(x)
        whole = guarded_call(cuda, h_d, dev(x, cuda), M, D, n0, N)
        edges = [0] + sorted({c for c in (1, 255, 256, 1000, N - 1) if 0 < c < N}) + [N]
        assert len(edges) == 7
        parts = []
        for k, (a, b) in enumerate(zip(edges, edges[1:])):
            need = (b - a - 1) * D + T
            x_part = shifted(x[a * D * e:(a * D + need) * e], (k + 4 * (n0 != 0)) % granule, cuda)
            seen.add(x_part.data_ptr() % 16)
            parts.append(guarded_call(cuda, h_d, x_part, M, D, n0 + a * D, b - a, off=k % 2))
        got = torch.cat(parts, dim=1)
        torch.cuda.synchronize()
        assert torch.equal(bits(got), bits(whole)), (M, D, T, n0, fmt)
    assert seen == set(range(0, 16, 16 // granule)), seen


@pytest.mark.parametrize("fmt,offsets", [("CF32", (1,)), ("CS8", (1, 3, 7))])
def test_parity_input_views_off_16_byte_alignment(cuda, plan_of, fmt, offsets):
    """The input a view 1 complex sample (8 bytes) or 1, 3, 7 int8 samples (2, 6, 14 bytes) past a 16-byte boundary:
    the staging's head / tail path. Parity holds and the alignment changes no bit."""
    M, D, T, n0 = 16, 8, 127, 12345
    N = 3 * plan_of(M, D, T)["kt"] + 37
    h = taps_of(T, 5)
    x = samples((N - 1) * D + T, fmt, seed=77)
    want = None
    for k in (0,) + offsets:
        view = shifted(x, k, cuda)
        assert view.data_ptr() % 16 == (k * x.itemsize * per(x)) % 16
        got = parity(cuda, h, x, M, D, n0, N, off=k % 2, x_d=view, label=f"input +{k}")
        want = got if want is None else want
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), k


@pytest.mark.parametrize("M,D,T", [(16, 8, 127), (4, 3, 33)])
def test_non_finite_samples_stay_in_their_windows(cuda, plan_of, M, D, T):
    """+Inf, -Inf and NaN at a dozen sparse positions, in the real or the imaginary component: exactly the output
    times whose window holds one are non-finite, in all M channels; every other output meets the bar."""
    N = plan_of(M, D, T)["kt"] + 300
    n0 = 12345
    h = taps_of(T, 17)
    x = samples((N - 1) * D + T, "CF32", seed=99).copy()
    bad = [np.inf, -np.inf, np.nan]
    at = np.linspace(T // 2, x.size - 1 - T // 3, 12).astype(np.int64)
    for k, j in enumerate(at):
        x[j] = complex(bad[k % 3], x[j].imag) if k % 4 < 2 else complex(x[j].real, bad[k % 3])
    m = np.arange(N, dtype=np.int64)
    hit = np.zeros(N, bool)
    for j in at:
        hit |= (m * D <= j) & (j < m * D + T)
    assert hit.any() and (~hit).sum() > N // 4
    got = guarded_call(cuda, dev(h, cuda), dev(x, cuda), M, D, n0, N, off=1).cpu().numpy()
    finite = np.isfinite(got.real) & np.isfinite(got.imag)
    assert not finite[:, hit].any(), "an output time with a non-finite sample in its window is finite in some channel"
    assert finite[:, ~hit].all(), "a non-finite sample reached an output time outside its windows"
    xz = np.where(np.isfinite(x.real) & np.isfinite(x.imag), x, 0).astype(np.complex64)
    ref = channelizer_ref(h, xz, M, D, n0, N)
    s = channelizer_bound(h, xz, D, N)
    err = channel_errors(got[:, ~hit], ref[:, ~hit], s[~hit])
    print(f"channelizer non-finite M={M} D={D} T={T}: {hit.sum()} of {N} output times hit, the others' normwise error "
          f"{err:.3e}")
    assert err <= FLOAT_TOL


def test_known_answer_tone_on_channel_3(cuda, plan_of):
    """A tone on channel 3's centre through a 16-tap boxcar (taps 1 / 16), M = D = 16, n0 = 5: row 3 is
    exp(-j 2 pi 15 / 16) everywhere (the phase of sample index 5 times 3 / 16 of a turn, conjugated) and the boxcar's
    nulls sit on every other channel centre. Bar FLOAT_TOL (S = 1) + 1e-7 for the tone's own rounding to float32."""
    M = D = T = 16
    n0 = 5
    N = plan_of(M, D, T)["kt"] + 37
    j = np.arange((N - 1) * D + T, dtype=np.int64)
    x = np.exp(2j * np.pi * ((3 * j) % 16) / 16).astype(np.complex64)
    h = np.full(T, 1.0 / 16, np.float32)
    got = guarded_call(cuda, dev(h, cuda), dev(x, cuda), M, D, n0, N).cpu().numpy()
    want = np.zeros((M, N), np.complex128)
    want[3] = np.exp(-2j * np.pi * 15 / 16)
    err = float(np.max(np.abs(got - want)))
    print(f"channelizer known answer: max error {err:.3e} (bar {FLOAT_TOL + 1e-7:.3e})")
    assert err <= FLOAT_TOL + 1e-7


@pytest.mark.parametrize("fmt", FORMATS)
def test_edges(cuda, fmt):
    from gsdr_amd import ops

    M, D, T = 8, 4, 31
    x_h = samples(4000, fmt, seed=5)
    x = dev(x_h, cuda)
    e = per(x_h)
    # no taps: zeros, inside the guards
    none = torch.empty(0, dtype=torch.float32, device=cuda)
    for off in (0, 1):
        out = guarded_call(cuda, none, x, M, D, 3, 900, off)
        assert torch.equal(bits(out), torch.zeros_like(bits(out)))
    # one output time
    h = taps_of(T, 1)
    got = guarded_call(cuda, dev(h, cuda), x[:T * e], M, D, 3, 1, off=1).cpu().numpy()
    xv = values(x_h[:T * e])
    assert channel_errors(got, channelizer_ref(h, xv, M, D, 3, 1), channelizer_bound(h, xv, D, 1)) <= FLOAT_TOL
    # no outputs: success, nothing written
    buf, flat = guarded(cuda, torch.complex64, 16, 0)
    ops.channelizer(x, dev(h, cuda), M, D, 3, 0, out=flat[:0].view(M, 0))
    check_guards(buf, flat[:0], what="no outputs")
    # num_outputs defaults to the most the input supports: one more would need more input
    y = ops.channelizer(x, dev(h, cuda), M, D)
    assert y.shape == (M, (4000 - T) // D + 1) and y.dtype == torch.complex64
    assert (y.shape[1] - 1) * D + T <= 4000 < y.shape[1] * D + T
    # rejected before any call
    with pytest.raises(ValueError):
        ops.channelizer(x, dev(h, cuda), M, D, 0, y.shape[1] + 1)    # a short input
    for bad_m in (12, 128):
        with pytest.raises(ValueError):
            ops.channelizer(x, dev(h, cuda), bad_m, D)
    with pytest.raises(ValueError):
        ops.channelizer(x, dev(h, cuda), M, 0)
