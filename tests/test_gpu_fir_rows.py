"""GPU: every tile shape of the FIR engine in FIR mode (the 37 rows of GSDR_FIR_ROWS and the runtime-decimation
tile), each at its own tap-chunk and tile edges (tests/fir_sweep.py; test_fir_sweep_plan.py proves on the host that
each call here reaches the row it names).

Per (row, tap kind), for 1, 2 and 3 tap chunks, full and with a last chunk of one tap:
  * one output, one short of a tile, a tile, a tile plus one, and two tiles with a ragged third: within the float bar
    of the C oracle, and bit-identical to the first outputs of the largest call (an output depends on its own window
    only: fir_engine.hpp, "Exact zero-padding semantics");
  * the input pointer off 16-byte alignment: the aligned call's bits;
  * int8 I/Q where the row takes it: the bits of the call on the converted floats;
  * one +Inf that only padding taps of some outputs see, and a NaN in the last sample: the oracle's NaN and Inf
    pattern, and the bar on the finite outputs.
At D = 4 on complex samples the three tiles are named outright for real taps (gsdrxFirFCVariant 0, 25, 26) and must
agree with the routed call bit for bit; complex taps reach the two larger tiles by the call's size alone.

Samples are a seeded permutation of a uniform grid on (-1, 1), all distinct, so a window read one sample off cannot
pass; taps are standard normal / sqrt(T). Measured maxima: DESIGN.md section 6.
"""
import numpy as np
import pytest
import torch

import fir_sweep as sw
from helpers import FLOAT_TOL, bound, finite_elements, normwise_err, same_specials
from oracle import oracle as o

pytestmark = pytest.mark.gpu


def dev(a, cuda):
    return torch.from_numpy(np.ascontiguousarray(a)).to(cuda)


def bits(t):
    return (torch.view_as_real(t) if t.is_complex() else t).view(torch.int32)


def same_bits(a, b):
    return a.shape == b.shape and torch.equal(bits(a), bits(b))


def make_taps(taps, T, seed):
    rng = np.random.default_rng(seed)
    t = (rng.standard_normal(T) / np.sqrt(T)).astype(np.float32)
    if taps == sw.COMPLEX_TAPS:
        t = (t + 1j * (rng.standard_normal(T) / np.sqrt(T))).astype(np.complex64)
    return t


def make_samples(sample, L, seed):
    """L samples whose components are a permutation of the M-point uniform grid on (-1, 1): all distinct."""
    M = L * (2 if sample == sw.COMPLEX else 1)
    assert M < 1 << 22
    v = ((2.0 * np.random.default_rng(seed).permutation(M) + 1.0 - M) / M).astype(np.float32)
    assert np.unique(v).size == M and np.all(np.abs(v) < 1)
    return v.view(np.complex64) if sample == sw.COMPLEX else v


def shifted(xd, off):
    """The same samples `off` samples off 16-byte alignment (run_fir's x_offset, test_gpu_fir.py)."""
    y = torch.cat([torch.zeros(off, dtype=xd.dtype, device=xd.device), xd])[off:]
    assert xd.data_ptr() % 16 == 0 and y.data_ptr() % 16 == (off * xd.element_size()) % 16 != 0
    return y


def caller(variant):
    from gsdr_amd import ops

    if variant < 0:
        return lambda td, xd, D, N: ops.fir(td, xd, D, N)
    return lambda td, xd, D, N: ops.fir_variant(variant, td, xd, D, N)


def report(what, name, family, err):
    print(f"SWEEP {what} family={family} case={name} max_err={err:.3e}")


def sweep(cuda, name, family, sample, taps, D, ts, ns, call, also=()):
    """The T x N grid: bar and prefix bit-identity for `call`; every call of `also` gives `call`'s bits."""
    worst = 0.0
    nmax = ns[-1]
    for T in ts:
        t = make_taps(taps, T, seed=1000 * D + T)
        x = make_samples(sample, (nmax - 1) * D + T, seed=77 * D + T)
        ref, s = o.fir(t, x, D, nmax), bound(t, x, D, nmax)
        td, xd = dev(t, cuda), dev(x, cuda)
        full = call(td, xd, D, nmax)
        for N in ns:
            xn = xd[:(N - 1) * D + T]
            y = call(td, xn, D, N)
            assert same_bits(y, full[:N]), f"{name} T={T} N={N}: not the first outputs of the {nmax}-output call"
            for other_name, other in also:
                assert same_bits(other(td, xn, D, N), y), f"{name} T={T} N={N}: {other_name} differs"
            err = normwise_err(y.cpu().numpy(), ref[:N], s[:N])
            worst = max(worst, err)
            assert err <= FLOAT_TOL, f"{name} T={T} N={N}: normwise error {err:.3e}"
    report("fir", name, family, worst)


def shifted_pointer(cuda, name, sample, taps, D, T, N, call):
    t = make_taps(taps, T, seed=1000 * D + T)
    x = make_samples(sample, (N - 1) * D + T, seed=77 * D + T)
    td, xd = dev(t, cuda), dev(x, cuda)
    aligned = call(td, xd, D, N)
    for off in sw.fir_offsets(sample):
        assert same_bits(call(td, shifted(xd, off), D, N), aligned), f"{name} T={T} N={N}: input {off} samples off"


def padding_poison(cuda, name, sample, taps, D, T, span, tile, N, at, call):
    """+Inf at sample `at` -- past output k*'s T taps, inside its padded span -- and NaN in the last sample."""
    kstar = tile + 1
    assert N == 2 * tile + 3 and kstar * D + T <= at < kstar * D + span
    t = make_taps(taps, T, seed=1000 * D + T)
    x = make_samples(sample, (N - 1) * D + T, seed=77 * D + T).copy()
    f = x.view(np.float32)
    per = 2 if sample == sw.COMPLEX else 1
    f[per * at] = np.inf
    f[-1] = np.nan
    ref = o.fir(t, x, D, N)
    ok = finite_elements(ref)
    k = np.arange(N)
    padding_only = (k * D + T <= at) & (at < k * D + span)
    assert padding_only[kstar] and np.all(ok[padding_only]), name   # the reference never forms those products
    assert np.count_nonzero(padding_only) >= 1 and 1 <= np.count_nonzero(~ok) < N // 2, name
    y = call(dev(t, cuda), dev(x, cuda), D, N).cpu().numpy()
    assert same_specials(y, ref), f"{name} T={T}: NaN / Inf pattern"
    assert normwise_err(y[ok], ref[ok], bound(t, x, D, N)[ok]) <= FLOAT_TOL, name


def int8_iq(L, seed):
    return np.random.default_rng(seed).integers(-128, 128, 2 * L, dtype=np.int8)


# ------------------------------------------------------------------------------------------------
# The table rows
# ------------------------------------------------------------------------------------------------
def row_call(row, taps):
    """(call, the other calls that must give its bits) for a row's sweep."""
    if sw.is_d4_complex(row) and taps == sw.REAL_TAPS:
        mine = sw.D4_VARIANT[row.name]
        also = [("routed", caller(-1))] + [(f"variant {v}", caller(v)) for v in sw.D4_VARIANT.values() if v != mine]
        return caller(mine), also
    return caller(-1), []


@pytest.mark.parametrize("param", sw.FIR_PARAMS, ids=sw.fir_id)
def test_row_tap_and_tile_edges(cuda, param):
    row, taps = param
    ts, ns = sw.fir_grid(row)
    call, also = row_call(row, taps)
    sweep(cuda, sw.fir_id(param), sw.FAMILY_NAMES[row.kernel], sw.sample_of(row), taps, row.D, ts, ns, call, also)


@pytest.mark.parametrize("param", sw.FIR_PARAMS, ids=sw.fir_id)
def test_row_input_off_alignment(cuda, param):
    row, taps = param
    ts, ns = sw.fir_grid(row)
    shifted_pointer(cuda, sw.fir_id(param), sw.sample_of(row), taps, row.D, ts[-1], ns[-1], row_call(row, taps)[0])


@pytest.mark.parametrize("param", [p for p in sw.FIR_PARAMS if sw.fir_takes_int8(*p)], ids=sw.fir_id)
def test_row_int8_equals_converted_float(cuda, param):
    """gsdrxFirFCInt8 off D = 4 takes the float rows; at D = 4 variant 0 is the float-shaped tile int8 takes."""
    from gsdr_amd import ops

    row, taps = param
    ts, ns = sw.fir_grid(row)
    T, N, D = ts[-1], ns[-1], row.D
    call = row_call(row, taps)[0]
    td = dev(make_taps(taps, T, seed=1000 * D + T), cuda)
    x8 = dev(int8_iq((N - 1) * D + T, seed=D + T), cuda)
    xf = ops.int8_to_norm_float(x8).view(torch.complex64)
    assert same_bits(call(td, x8, D, N), call(td, xf, D, N)), sw.fir_id(param)


@pytest.mark.parametrize("param", sw.FIR_PARAMS, ids=sw.fir_id)
def test_row_padding_poison(cuda, param):
    row, taps = param
    c, D = sw.ct(row), row.D
    T = c + 1                       # two chunks, the second all padding but one tap
    span = 2 * c
    at = (sw.kt(row) + 1) * D + T + (span - T) // 2
    padding_poison(cuda, sw.fir_id(param), sw.sample_of(row), taps, D, T, span, sw.kt(row), sw.fir_grid(row)[1][-1], at,
                   row_call(row, taps)[0])


# ------------------------------------------------------------------------------------------------
# D = 4, complex taps on complex samples: the two larger tiles by size
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("T", sw.D4_BIG_T)
@pytest.mark.parametrize("tile", [512, 1024], ids=["C4R2", "C4"])
def test_d4_complex_taps_larger_tiles(cuda, tile, T):
    """One gsdrFirCC call sized for the tile; its head, a window across a middle tile edge and its tail equal
    515-output calls on the same samples bit for bit, and the oracle within the bar."""
    from gsdr_amd import ops

    D, W = 4, sw.D4_WINDOW
    cus = torch.cuda.get_device_properties(cuda).multi_processor_count
    N = sw.d4_n_r2(cus) if tile == 512 else sw.d4_n_r4(cus)
    gen = torch.Generator(device=cuda).manual_seed(tile + T)
    x = (torch.rand(2 * ((N - 1) * D + T), device=cuda, generator=gen) * 2 - 1).view(torch.complex64)
    t = make_taps(sw.COMPLEX_TAPS, T, seed=4000 + T)
    td = dev(t, cuda)
    y = ops.fir(td, x, D, N)
    worst = 0.0
    for k0 in sw.big_windows(N, tile):
        xs = x[k0 * D:(k0 + W - 1) * D + T]
        assert same_bits(ops.fir(td, xs, D, W), y[k0:k0 + W]), f"window at output {k0}"
        xh = xs.cpu().numpy()
        worst = max(worst, normwise_err(y[k0:k0 + W].cpu().numpy(), o.fir(t, xh, D, W), bound(t, xh, D, W)))
    report("fir", f"C4-tile{tile}-complex-T{T}", "polyphase", worst)
    assert worst <= FLOAT_TOL


# ------------------------------------------------------------------------------------------------
# The runtime-decimation tile
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("param", sw.RT_FIR_PARAMS, ids=sw.rt_fir_id)
def test_runtime_d_tap_and_tile_edges(cuda, param):
    sample, taps, D = param
    ts, ns = sw.rt_fir_grid(sample, D)
    sweep(cuda, sw.rt_fir_id(param), "runtime-D", sample, taps, D, ts, ns, caller(-1))


@pytest.mark.parametrize("param", sw.RT_FIR_PARAMS, ids=sw.rt_fir_id)
def test_runtime_d_input_off_alignment(cuda, param):
    sample, taps, D = param
    ts, ns = sw.rt_fir_grid(sample, D)
    shifted_pointer(cuda, sw.rt_fir_id(param), sample, taps, D, ts[-1], ns[-1], caller(-1))


@pytest.mark.parametrize("param", sw.RT_FIR_PARAMS, ids=sw.rt_fir_id)
def test_runtime_d_padding_poison(cuda, param):
    """15 padding taps: the +Inf sits on the first of them."""
    sample, taps, D = param
    T, tile = sw.rt_poison_t(D), sw.RT_WG[(sample, D)]
    span = -(-T // sw.RT_CHUNK) * sw.RT_CHUNK
    assert span - T == 15
    padding_poison(cuda, sw.rt_fir_id(param), sample, taps, D, T, span, tile, sw.rt_fir_grid(sample, D)[1][-1],
                   (tile + 1) * D + T, caller(-1))
