"""The headline FIR tile (real taps, complex samples, D = 4: R 4, chunk 16, WG 256) stages whole tiles wave by wave,
with the wave's own wait where the workgroup barrier stood, reads odd taps from the high half of their SGPR pair and
reads the carried window rows where the old ones die (fir_staging.hpp: stage_tile_wave; fir_engine.hpp: TapChunk::pair,
poly_compute).
None of it may change a bit: every kernel with the same (D, chunk) sums the same products in the same order.

Bars. Bit identity (uint64 views of the complex64 outputs) of gsdrFirFC against gsdrxFirFCVariant 28 and 24, the same
(D, chunk) on workgroups of 128 and 64 threads, which keep the workgroup's staging map and its barrier, and against
variant 0, the headline tile shape named outright (short calls take smaller tiles by default). The oracle's bar is the
float path's normwise one (helpers.FLOAT_TOL against S_k = sum |t_i| |x_kD+i|). Inputs are seeded uniform samples, all
distinct, so a granule staged to the wrong slot cannot cancel.

Tile arithmetic used below: a tile is 1,024 outputs = 4,096 samples; its staged span is 4,092 + 64 ceil(T / 64)
samples, and a tile is staged wave by wave only when that whole span is readable, i.e. lies within the call's
(N - 1) D + T samples."""
import functools

import numpy as np
import pytest
import torch

from helpers import FLOAT_TOL, bound, normwise_err
from oracle import oracle as o

pytestmark = pytest.mark.gpu

D = 4
TILE = 1024
SIZES = (1, 1023, 1024, 1025, 2048, 3 * 1024 + 5)
TAPS = (1, 2, 63, 64, 65, 127, 128, 129, 191)
OLD_MAP = (28, 24)  # same (D, chunk), WG 128 / 64: the workgroup's staging map
NMAX = max(SIZES)


def dev(a, cuda):
    return torch.from_numpy(np.array(a, copy=True)).to(cuda)  # (the shared cases are read-only arrays)


def bits(y):
    return np.ascontiguousarray(y).view(np.uint64)


@functools.lru_cache(maxsize=None)
def case(T):
    """Taps, samples for the largest size (the smaller sizes use a prefix) and the oracle's outputs and bound for it;
    computed once per tap count and left unchanged."""
    rng = np.random.default_rng(1000 + T)
    taps = (rng.standard_normal(T) / np.sqrt(T)).astype(np.float32)
    x = (rng.random(2 * ((NMAX - 1) * D + T), dtype=np.float32) * 2 - 1).view(np.complex64)
    ref = o.fir(taps, x, D, NMAX)
    s = bound(taps, x, D, NMAX)
    for a in (taps, x, ref, s):
        a.setflags(write=False)
    return taps, x, ref, s


def run_all(cuda, taps_d, x_d, N):
    """gsdrFirFC and the comparison variants on the same device buffers."""
    from gsdr_amd import ops

    y = ops.fir(taps_d, x_d, D, N).cpu().numpy()
    others = {v: ops.fir_variant(v, taps_d, x_d, D, N).cpu().numpy() for v in OLD_MAP + (0,)}
    return y, others


@pytest.mark.parametrize("T", TAPS)
def test_bit_identical_to_old_map_and_oracle_parity(cuda, T):
    taps, x, ref, s = case(T)
    taps_d = dev(taps, cuda)
    for N in SIZES:
        L = (N - 1) * D + T
        x_d = dev(x[:L], cuda)
        y, others = run_all(cuda, taps_d, x_d, N)
        for v, yv in others.items():
            assert np.array_equal(bits(y), bits(yv)), f"T {T} N {N}: gsdrFirFC != variant {v}"
        # (the oracle's outputs for a prefix of the samples are a prefix of its outputs)
        err = normwise_err(y, ref[:N], s[:N])
        assert err <= FLOAT_TOL, f"T {T} N {N}: normwise error {err}"


@pytest.mark.parametrize("T", TAPS)
def test_shifted_input_bit_identical_to_aligned(cuda, T):
    """The input pointer one sample (8 bytes) off 16-byte alignment: the shifted staging path, which keeps the
    workgroup's map. Same samples, same bits."""
    from gsdr_amd import ops

    taps, x, ref, s = case(T)
    taps_d = dev(taps, cuda)
    N = NMAX
    L = (N - 1) * D + T
    aligned = dev(x[:L], cuda)
    holder = torch.empty(L + 1, dtype=torch.complex64, device=cuda)
    shifted = holder[1:]
    shifted.copy_(aligned)
    assert aligned.data_ptr() % 16 == 0 and shifted.data_ptr() % 16 == 8
    ya = ops.fir(taps_d, aligned, D, N).cpu().numpy()
    ys = ops.fir(taps_d, shifted, D, N).cpu().numpy()
    assert np.array_equal(bits(ya), bits(ys))
    for v in OLD_MAP + (0,):
        yv = ops.fir_variant(v, taps_d, shifted, D, N).cpu().numpy()
        assert np.array_equal(bits(ya), bits(yv)), f"variant {v} on the shifted input"
    assert normwise_err(ys, ref[:N], s[:N]) <= FLOAT_TOL


CUT_TAPS = (1, 59, 100, 121)  # T + 4 < 64 ceil(T / 64): tile 1's staged span ends past the call's samples


@pytest.mark.parametrize("T", CUT_TAPS + (127,))
def test_cut_input_bit_identical_to_long_call(cuda, T):
    """The call's readable samples end inside the second-to-last tile's staged span: N = 2 tiles + 1 output reads
    2,048 D + T samples, and tile 1's span ends at sample 8,188 + 64 ceil(T / 64), past them for the CUT_TAPS (T = 127
    leaves tile 1 whole: the control). That tile is then staged granule by granule behind the barrier. Its outputs
    must equal, bit for bit, those of the longer call on the same samples, where tile 1 is whole and staged wave by
    wave."""
    from gsdr_amd import ops

    taps, x, ref, s = case(T)
    taps_d = dev(taps, cuda)
    N = 2 * TILE + 1
    L = (N - 1) * D + T
    span_end = TILE * D + (TILE - 1) * D + 64 * ((T + 63) // 64)
    assert (L < span_end) == (T in CUT_TAPS)
    long_d = dev(x, cuda)  # NMAX outputs' worth
    y_long = ops.fir(taps_d, long_d, D, NMAX).cpu().numpy()
    cut_d = dev(x[:L], cuda)  # a buffer of its own that ends where the call's samples end
    y_cut, others = run_all(cuda, taps_d, cut_d, N)
    assert np.array_equal(bits(y_cut), bits(y_long[:N]))
    for v, yv in others.items():
        assert np.array_equal(bits(y_cut), bits(yv)), f"variant {v}"
    assert normwise_err(y_cut, ref[:N], s[:N]) <= FLOAT_TOL


@pytest.mark.parametrize("calls", [1, 2, 7])
def test_stream_bit_identical_to_monolithic(cuda, calls):
    """A three-tile channel through gsdrxStream (complex float FIR, D = 4) in 1, 2 and 7 calls: the history tile
    followed by whole tiles. Chunk lengths are multiples of two samples where that is possible, so later calls keep
    the aligned staging."""
    from gsdr_amd import ops
    from gsdr_amd.stream import Stream

    T = 127
    taps, x, ref, s = case(T)
    N = 3 * TILE
    L = (N - 1) * D + T
    taps_d, x_d = dev(taps, cuda), dev(x[:L], cuda)
    want = ops.fir(taps_d, x_d, D, N)
    st = Stream("fir", taps_d, D)
    step = -(-L // calls)
    step += step % 2
    parts = [st.process(x_d[p:min(L, p + step)]).clone() for p in range(0, L, step)]
    st.close()
    assert len(parts) == calls
    got = torch.cat(parts)
    assert got.numel() == N
    assert np.array_equal(bits(got.cpu().numpy()), bits(want.cpu().numpy()))


def assert_same_specials(got, want):
    g = np.ascontiguousarray(got).view(np.float32)
    w = np.ascontiguousarray(want).view(np.float32)
    assert np.array_equal(np.isnan(g), np.isnan(w)), "NaN pattern"
    inf = np.isinf(w)
    assert np.array_equal(np.isinf(g), inf), "Inf pattern"
    assert np.array_equal(g[inf], w[inf]), "Inf signs"


# tile-local sample offsets of (+Inf, NaN): granules 512 .. 573 follow wave 0's share (samples 1,024 .. 1,147),
# granules 1,536 .. 1,597 follow wave 2's (samples 3,072 .. 3,195), and samples 4,096 .. 4,219 are the tile's halo
PLACES = {"after_wave0": (1030, 1101), "after_wave2": (3080, 3150), "halo": (4100, 4200)}


@pytest.mark.parametrize("place", sorted(PLACES))
def test_nonfinite_in_shared_granules(cuda, place):
    """One +Inf and one NaN sample in the granules two waves stage (or in the halo) of tile 1, a whole tile of a
    three-tile call: finiteness and sign follow the oracle, as tests/test_gpu_nonfinite.py checks them."""
    T, N = 127, NMAX
    taps, x, _, _ = case(T)
    xp = x.copy()
    a, b = PLACES[place]
    xp[TILE * D + a] = np.complex64(complex(np.inf, 0.25))
    xp[TILE * D + b] = np.complex64(complex(-0.5, np.nan))
    ref = o.fir(taps, xp, D, N)
    taps_d, x_d = dev(taps, cuda), dev(xp, cuda)
    y, others = run_all(cuda, taps_d, x_d, N)
    assert_same_specials(y, ref)
    ok = np.isfinite(ref.real) & np.isfinite(ref.imag)
    assert 0 < (~ok).sum() < 100
    assert normwise_err(y[ok], ref[ok], bound(taps, xp, D, N)[ok]) <= FLOAT_TOL
    for v, yv in others.items():
        assert_same_specials(yv, ref)
        fin = np.isfinite(y.view(np.float32))
        assert np.array_equal(y.view(np.float32)[fin], yv.view(np.float32)[fin]), f"variant {v}"
