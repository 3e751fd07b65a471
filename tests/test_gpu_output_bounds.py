"""GPU: no FIR / FM / AM / int8 / multi-channel / stream entry point writes outside [output, output + numOutputs),
whatever the output pointer's alignment and however the output count falls on the tiles.

Every entry point takes a raw pointer and a count, and every kernel picks its store path from the address (8- / 16-byte
vector stores when a thread's R outputs are all in range and aligned, scalar stores otherwise; whole-tile stores through
LDS; the matrix-core kernels' output-aligned flag; anchored FM / AM tiles that start before output 0; FM tiles that
overlap). Each case here writes into a view in the middle of a sentinel-filled buffer (helpers.guarded) and asserts
  * the call returns that view,
  * the guard elements on both sides are untouched, compared bytewise,
  * the outputs meet the entry point's parity bar against the oracle (the bars of test_gpu_fir.py / test_gpu_chains.py /
    test_gpu_int8.py), and
  * the outputs at every pointer offset equal the offset-0 outputs bit for bit: the store path may depend on the
    address, the values may not.
Output offsets: 0 and 1 element for complex outputs (16- and 8-byte aligned), 0..3 for float outputs. Output counts: one
thread's R outputs (1, 2, 3, 5), and one below / at / one above the 256-, 512- and 1,024-output tiles, FM's 255 / 510 /
1,020-output strides and the NCO cells at D = 4.
"""
import numpy as np
import pytest
import torch

from helpers import FLOAT_TOL, bound, check_guards, default_sentinel, guarded, normwise_err, wrapped_angle_err
from oracle import oracle as o
from test_gpu_fir import TYPES, make
from test_gpu_stream import chunks

pytestmark = pytest.mark.gpu

FS, TUNE, CHAN, DEV = 1.0e6, 0.0, 1.0e5, 2.0e4
NS = [1, 2, 3, 5, 254, 255, 256, 257, 509, 511, 1019, 1020, 1021, 1023, 1025, 2047, 2051]
NMAX = max(NS)
C64, F32 = torch.complex64, torch.float32

# One decimation of every dispatch class of DESIGN.md section 3.1 (fir_dispatch.hpp launch_fir), 33 taps: the default
# shapes of D = 1, 2, 4, 8; launch_other_d's contiguous-window and short polyphase tiles (3, 5, 6, 12, 16) and its
# one-output-a-thread polyphase tiles (20, 64); the runtime-decimation kernel k_fir_rt (9, 13, 50); and the generic
# kernel through launch_rt's D >= T branch (D = 64, T = 8).
DISPATCH_CASES = [(D, 33) for D in (1, 2, 4, 8, 3, 5, 6, 12, 16, 20, 48, 64, 9, 13, 50)] + [(64, 8)]

# The generic kernel's other way in: at D = 4 the shortest filter whose tile no longer fits kMaxTileLds = 64 KiB
# (fir_dispatch.hpp tap_span -> launch_generic), for the shape these output counts take.
#   complex samples (FC, CF): launch_poly_d4's short-call shape R = 1, JC = 16, WG = 256. The tap span is T rounded up
#   to 64 samples; NG = 510 + span / 2 granules, padded by one for every two: (g + g // 2 + 1) * 16 B with g = NG - 1
#   fits while g <= 2730, i.e. span <= 4416 -- T = 4417 leaves the tiles.
#   real samples (FF, CC): R = 8, JC = 8, WG = 128. Span = T rounded up to 32; NG = 1023 + span / 4, padded by one for
#   every eight: g + g // 8 <= 4095 while g <= 3640, i.e. span <= 10464 -- T = 10465 leaves the tiles.
LONG_T = {"FC": 4417, "CF": 4417, "FF": 10465, "CC": 10465}


def dev(a, cuda):
    return torch.from_numpy(np.ascontiguousarray(a)).to(cuda)


def host(t):
    torch.cuda.synchronize()
    return t.cpu().numpy()


def fm_gain():
    return float(np.float32(FS) / (np.float32(2.0) * np.float32(np.pi) * np.float32(DEV)))


def offsets(dtype):
    return (0, 1) if dtype.is_complex else (0, 1, 2, 3)


def sweep(cuda, dtype, call, check, ns=NS, what=""):
    """For every output count and output pointer offset: call(N, out) (returns the entry point's result) into a guarded
    view; the result is that view, the guards are intact, check(N, outputs) holds at offset 0 and the other offsets
    give the same bytes."""
    for N in ns:
        first = None
        for off in offsets(dtype):
            case = f"{what} N={N} output offset {off}"
            buf, view = guarded(cuda, dtype, N, off)
            got = call(N, view)
            assert got.data_ptr() == view.data_ptr() and got.shape == view.shape and got.dtype == dtype, case
            check_guards(buf, view, what=case)
            y = host(view)
            if first is None:
                first = y
                check(N, y)
            else:
                assert y.tobytes() == first.tobytes(), f"{case}: outputs differ from those at offset 0"


@pytest.mark.parametrize("D,T", DISPATCH_CASES + [(4, "long")])
@pytest.mark.parametrize("tt", list(TYPES))
def test_fir_output_bounds(cuda, tt, D, T):
    """gsdrFir{FC,FF,CC,CF}: store_fir's vector / scalar choice in every dispatch class, and the generic kernel."""
    from gsdr_amd import ops

    if T == "long":
        T = LONG_T[tt]
    taps, x = make(tt, T, (NMAX - 1) * D + T, seed=D * 1000 + T)
    ref, s = o.fir(taps, x, D, NMAX), bound(taps, x, D, NMAX)
    td, xd = dev(taps, cuda), dev(x, cuda)

    def call(N, out):
        return ops.fir(td, xd[:(N - 1) * D + T], D, N, out=out)

    def check(N, y):
        err = normwise_err(y, ref[:N], s[:N])
        assert err <= FLOAT_TOL, f"{tt} D={D} T={T} N={N}: normwise error {err:.3e}"

    sweep(cuda, F32 if tt == "FF" else C64, call, check, what=f"gsdrFir{tt} D={D} T={T}")


def variant_output_bounds(cuda, variant, ns):
    from gsdr_amd import ops

    D, T = 4, 33
    nmax = max(ns)
    taps, x = make("FC", T, (nmax - 1) * D + T, seed=variant)
    ref, s = o.fir(taps, x, D, nmax), bound(taps, x, D, nmax)
    td, xd = dev(taps, cuda), dev(x, cuda)
    base = {}

    def call_variant(v):
        return lambda N, out: ops.fir_variant(v, td, xd[:(N - 1) * D + T], D, N, out=out)

    def keep(N, y):
        assert normwise_err(y, ref[:N], s[:N]) <= FLOAT_TOL, N
        base[N] = y

    def same_as_variant_0(N, y):
        assert y.tobytes() == base[N].tobytes(), f"variant {variant} N={N}: differs from variant 0"

    sweep(cuda, C64, call_variant(0), keep, ns, what="gsdrxFirFCVariant 0")
    sweep(cuda, C64, call_variant(variant), same_as_variant_0, ns, what=f"gsdrxFirFCVariant {variant}")


@pytest.mark.parametrize("variant", [9, 10, 11, 14])
def test_fir_fc_d4_store_variants_output_bounds(cuda, variant):
    """gsdrxFirFCVariant 9 (XCD tile order), 10 / 11 (tile stored through LDS: store_tile_lds's whole-tile / aligned
    condition, plain and non-temporal), 14 (LDS-DMA staging): one below, at and above one 1,024-output tile, whole
    tiles, and whole tiles plus one output; bit-identical to variant 0, which is guarded too."""
    variant_output_bounds(cuda, variant, [1023, 1024, 1025, 2 * 1024, 3 * 1024 + 1])


@pytest.mark.parametrize("variant", [1, 25])
def test_fir_fc_d4_tile_shapes_output_bounds(cuda, variant):
    """A call of a few thousand outputs runs gsdrFirFC's 256-output short-call shape, one output a thread, whose
    store has no vector form; the shapes a whole channel runs are reached here by name: variant 0 (R = 4, the
    reference in variant_output_bounds), 25 (R = 2, the 512-output tiles) and 1 (R = 8). Every output count."""
    variant_output_bounds(cuda, variant, NS)


def chain_input(fm, L, seed, n0):
    """The parity tests' signals (test_gpu_chains.py): constant-envelope FM for the discriminator, uniform I/Q for AM."""
    from gsdr_amd.signals import fm_test_signal, uniform_iq

    if fm:
        return fm_test_signal(L, fs=FS, noise=0.05, seed=seed, n0=n0 % (1 << 20))
    return (0.7 * uniform_iq(L, seed=seed)).astype(np.complex64)


def first_sample_indices(D):
    """tile_shift = (firstSampleIndex / D) mod stride zero, non-zero (output 0 inside its tile: the first tile starts
    before the output buffer, with a wrapped first index) and past 2^32."""
    return (0, 1333 * D + 1, (1 << 32) + 5)


@pytest.mark.parametrize("D,T", DISPATCH_CASES)
@pytest.mark.parametrize("kind", ["fm", "am"])
def test_chain_output_bounds(cuda, kind, D, T):
    """gsdrFmDemod / gsdrAmDemod: store_chain in every dispatch class; anchored tiles whose first one starts before
    output 0; FM's overlapping tiles, whose last thread's outputs belong to the next tile."""
    from gsdr_amd import ops
    from gsdr_amd.signals import lowpass_taps

    fm = kind == "fm"
    taps = lowpass_taps(T, 0.1)
    td = dev(taps, cuda)

    def need(N):
        return (N if fm else N - 1) * D + T

    for n0 in first_sample_indices(D):
        x = chain_input(fm, need(NMAX), D + T, n0)
        xd = dev(x, cuda)
        if fm:
            ref = o.fm_demod(x, taps, FS, TUNE, CHAN, DEV, D, n0, NMAX)
        else:
            ref = o.am_demod(x, taps, FS, TUNE, CHAN, D, n0, NMAX)

        def call(N, out):
            if fm:
                return ops.fm_demod(xd[:need(N)], td, FS, TUNE, CHAN, DEV, D, n0, N, out=out)
            return ops.am_demod(xd[:need(N)], td, FS, TUNE, CHAN, D, n0, N, out=out)

        def check(N, y):
            err = wrapped_angle_err(y, ref[:N], fm_gain()) if fm else float(np.max(np.abs(y - ref[:N])))
            assert err <= FLOAT_TOL, f"{kind} D={D} T={T} n0={n0} N={N}: error {err:.3e}"

        sweep(cuda, F32, call, check, what=f"{kind} D={D} T={T} firstSampleIndex={n0}")


@pytest.mark.parametrize("tiles", ["tiles512", "tiles1024"])
@pytest.mark.parametrize("kind", ["fm", "am"])
def test_chain_d4_channel_tile_shapes_output_bounds(cuda, kind, tiles):
    """At D = 4 a call of a few thousand outputs runs the 256-output short-call tiles (launch_poly_d4), one output a
    thread, so test_chain_output_bounds never reaches store_chain's float2 / float4 stores of the shapes a whole
    channel runs: the 512-output tiles (R = 2) and the 1,024-output tiles (R = 4), chosen by the output count
    (test_gpu_chains.d4_outputs). Four consecutive counts just inside each shape put the last thread's 0 .. R - 1
    valid outputs at every position; all four output offsets; output 0 inside its tile. The 512-output shape is held
    to the oracle; the 1,024-output shape (3.1 M outputs, device-generated input) to the guards and to equal bytes at
    every offset, its parity being test_fm_full_config's business."""
    from gsdr_amd import ops
    from gsdr_amd.signals import lowpass_taps
    from test_gpu_chains import d4_outputs

    D, T, n0, fm = 4, 33, 4 * 1333 + 1, kind == "fm"
    first = d4_outputs(cuda, tiles)
    ns = [first + i for i in range(4)]
    taps = lowpass_taps(T, 0.1)
    td = dev(taps, cuda)

    def need(N):
        return (N if fm else N - 1) * D + T

    if tiles == "tiles512":
        x = chain_input(fm, need(ns[-1]), 5, n0)
        xd = dev(x, cuda)
        if fm:
            ref = o.fm_demod(x, taps, FS, TUNE, CHAN, DEV, D, n0, ns[-1])
        else:
            ref = o.am_demod(x, taps, FS, TUNE, CHAN, D, n0, ns[-1])
    else:
        gen = torch.Generator(device=cuda).manual_seed(4)
        xd = torch.view_as_complex(torch.rand(need(ns[-1]), 2, device=cuda, generator=gen) - 0.5)
        ref = None

    def call(N, out):
        if fm:
            return ops.fm_demod(xd[:need(N)], td, FS, TUNE, CHAN, DEV, D, n0, N, out=out)
        return ops.am_demod(xd[:need(N)], td, FS, TUNE, CHAN, D, n0, N, out=out)

    def check(N, y):
        if ref is not None:
            err = wrapped_angle_err(y, ref[:N], fm_gain()) if fm else float(np.max(np.abs(y - ref[:N])))
            assert err <= FLOAT_TOL, f"{kind} {tiles} N={N}: error {err:.3e}"

    sweep(cuda, F32, call, check, ns, what=f"{kind} D=4 {tiles}")


def int8_signal(L, n0):
    """The int8 chain tests' signal (test_gpu_int8.py): the FM test signal at 100 / 127 of full scale."""
    from gsdr_amd.signals import fm_test_signal

    x = fm_test_signal(L, noise=0.02, n0=n0 % (1 << 20))
    return np.clip(np.round(np.stack([x.real, x.imag], 1).ravel() * 100), -128, 127).astype(np.int8)


# tap counts the matrix-core kernels take (fir_dispatch.hpp: I8Mfma<4, 8>::MAXT, I8ChainMfma<MODE>::MAXT)
INT8_MFMA_MAXT = {"fir": 196, "fm": 132, "am": 132}


@pytest.mark.parametrize("D,T", [(4, 33), (4, "above"), (1, 33), (3, 33), (8, 33)])
@pytest.mark.parametrize("kind", ["fir", "fm", "am"])
def test_int8_output_bounds(cuda, kind, D, T):
    """gsdrxFirFCInt8 / gsdrxFmDemodInt8 / gsdrxAmDemodInt8. D = 4, T = 33: the matrix-core kernels (output-aligned
    stores at offset 0, the unaligned form at offset 1 for the complex FIR outputs; the chains' float outputs at all
    four offsets), which gsdr_ext.h holds to the parity bar against the float entry point. D = 4 with one tap more
    than the matrix-core kernel takes, and D = 1, 3, 8: the float-shaped tiles, bit-identical to gsdrInt8ToNormFloat
    followed by the float entry point."""
    from gsdr_amd import ops
    from gsdr_amd.signals import lowpass_taps

    limit = INT8_MFMA_MAXT[kind]
    if T == "above":
        T = limit + 1
    exact = not (D == 4 and T <= limit)
    fir, fm = kind == "fir", kind == "fm"
    taps = lowpass_taps(T)
    td = dev(taps, cuda)
    g = fm_gain()

    def need(N):
        return (N if fm else N - 1) * D + T

    def run(x, N, n0, out=None):
        if fir:
            return ops.fir(td, x, D, N, out=out)
        if fm:
            return ops.fm_demod(x, td, FS, TUNE, CHAN, DEV, D, n0, N, out=out)
        return ops.am_demod(x, td, FS, TUNE, CHAN, D, n0, N, out=out)

    for n0 in ((0,) if fir else (0, 1333 * D + 1)):
        L = need(NMAX)
        x8 = int8_signal(L, n0)
        xf = o.int8_to_float(x8).view(np.complex64)
        x8d = dev(x8, cuda)
        xfd = torch.view_as_complex(ops.int8_to_norm_float(x8d).view(L, 2))
        assert host(xfd).tobytes() == xf.tobytes()
        if fir:
            ref, s = o.fir(taps, xf, D, NMAX), bound(taps, xf, D, NMAX)
        elif fm:
            ref = o.fm_demod(xf, taps, FS, TUNE, CHAN, DEV, D, n0, NMAX)
        else:
            ref = o.am_demod(xf, taps, FS, TUNE, CHAN, D, n0, NMAX)

        def err(N, y, want):
            if fir:
                return normwise_err(y, want, s[:N])
            return wrapped_angle_err(y, want, g) if fm else float(np.max(np.abs(y - want)))

        def call(N, out):
            return run(x8d[:2 * need(N)], N, n0, out)

        def check(N, y):
            where = f"int8 {kind} D={D} T={T} n0={n0} N={N}"
            e = err(N, y, ref[:N])
            assert e <= FLOAT_TOL, f"{where}: error against the oracle {e:.3e}"
            yf = host(run(xfd[:need(N)], N, n0))
            if exact:
                assert y.tobytes() == yf.tobytes(), f"{where}: differs from conversion + the float entry point"
            else:
                e = err(N, y, yf)
                assert e <= FLOAT_TOL, f"{where}: error against the float entry point {e:.3e}"

        sweep(cuda, C64 if fir else F32, call, check, what=f"int8 {kind} D={D} T={T} firstSampleIndex={n0}")


def channel_list(C):
    return [float(v) for v in np.linspace(-0.35, 0.35, C) * FS]


@pytest.mark.parametrize("int8", [False, True])
@pytest.mark.parametrize("D", [4, 3])
@pytest.mark.parametrize("C", [3, 17])
@pytest.mark.parametrize("kind", ["fm", "am", "xlate"])
def test_multi_output_bounds(cuda, kind, C, D, int8):
    """gsdrxFmDemodMulti / gsdrxAmDemodMulti / gsdrxXlatingFirMulti: the grouped kernel (D = 4; 17 channels are two
    launches) and the per-channel fallback (D = 3). The output counts are odd, so with row c at c * numOutputs elements
    rows 1.. start off alignment whatever the base; guards before row 0 and after the last row; every row equals the
    single-channel call bit for bit."""
    from gsdr_amd import ops
    from gsdr_amd.signals import fm_test_signal, lowpass_taps

    T, n0 = 33, 1333 * D + 1
    fm = kind == "fm"
    odt = C64 if kind == "xlate" else F32
    td = dev(lowpass_taps(T), cuda)
    chans = channel_list(C)
    devs = [DEV * (1 + 0.1 * c) for c in range(C)]
    for N in (255, 1021, 2051):
        L = (N if fm else N - 1) * D + T
        x = dev(int8_signal(L, n0) if int8 else fm_test_signal(L, noise=0.02, n0=n0), cuda)
        if fm:
            singles = [ops.fm_demod(x, td, FS, TUNE, chans[c], devs[c], D, n0, N) for c in range(C)]
        elif kind == "am":
            singles = [ops.am_demod(x, td, FS, TUNE, chans[c], D, n0, N) for c in range(C)]
        else:
            singles = [ops.xlating_fir(x, td, FS, TUNE, chans[c], D, n0, N) for c in range(C)]
        for off in (0, 1):
            case = f"{kind} multi C={C} D={D} int8={int8} N={N} output offset {off}"
            buf, flat = guarded(cuda, odt, C * N, off)
            out = flat.view(C, N)
            if fm:
                got = ops.fm_demod_multi(x, td, FS, TUNE, chans, devs, D, n0, N, out=out)
            elif kind == "am":
                got = ops.am_demod_multi(x, td, FS, TUNE, chans, D, n0, N, out=out)
            else:
                got = ops.xlating_fir_multi(x, td, FS, TUNE, chans, D, n0, N, out=out)
            assert got.data_ptr() == out.data_ptr() and got.shape == (C, N), case
            check_guards(buf, flat, what=case)
            for c in range(C):
                assert host(out[c]).tobytes() == host(singles[c]).tobytes(), f"{case}: row {c}"


def stream_input(cuda, L, n0, int8):
    from gsdr_amd.signals import fm_test_signal

    x = fm_test_signal(L, noise=0.02, n0=n0)
    if int8:
        return dev(np.clip(np.round(np.stack([x.real, x.imag], 1).ravel() * 100), -128, 127).astype(np.int8), cuda)
    return dev(x, cuda)


@pytest.mark.parametrize("int8", [False, True])
@pytest.mark.parametrize("D", [4, 3, 9])
@pytest.mark.parametrize("kind", ["fir", "fm", "am", "xlate"])
def test_stream_output_bounds(cuda, kind, D, int8):
    """gsdrxStreamProcess into the caller's buffer: the one-launch step on the tiled kernels (D = 4, 3) and the seam
    plan's two filter calls a chunk (D = 9), whose second call writes at output + (seam outputs). Every call's
    outputs go into a guarded view whose alignment changes from call to call; the concatenation equals the monolithic
    call bit for bit."""
    from gsdr_amd import ops
    from gsdr_amd.signals import lowpass_taps
    from gsdr_amd.stream import Stream

    T, n0, L = 33, 4_000_000_123, 20_000
    per = 2 if int8 else 1
    odt = C64 if kind in ("fir", "xlate") else F32
    xd = stream_input(cuda, L, n0, int8)
    taps = dev(lowpass_taps(T), cuda)
    if kind == "fir":
        want = ops.fir(taps, xd, D)
    elif kind == "fm":
        want = ops.fm_demod(xd, taps, FS, TUNE, CHAN, DEV, D, n0)
    elif kind == "am":
        want = ops.am_demod(xd, taps, FS, TUNE, CHAN, D, n0)
    else:
        want = ops.xlating_fir(xd, taps, FS, TUNE, CHAN, D, n0)
    s = Stream(kind, taps, D, FS, TUNE, CHAN, DEV, first_sample_index=n0, int8=int8)
    parts, pos = [], 0
    for i, m in enumerate(chunks(L, seed=D * 10 + len(kind) + int8, W=T + D if kind == "fm" else T)):
        case = f"stream {kind} D={D} int8={int8} call {i} ({m} samples at {pos})"
        n_out = s.outputs_for(m)
        buf, view = guarded(cuda, odt, n_out, i % len(offsets(odt)))
        got = s.process(xd[pos * per:(pos + m) * per], out=view)
        assert got.numel() == n_out and (n_out == 0 or got.data_ptr() == view.data_ptr()), case
        check_guards(buf, view, what=case)
        parts.append(view.clone())
        pos += m
    s.close()
    assert pos == L
    got = torch.cat(parts)
    assert got.numel() == want.numel() > 0
    assert host(got).tobytes() == host(want).tobytes()


@pytest.mark.parametrize("kind", ["fm", "am", "xlate"])
def test_multi_stream_output_capacity_tail_untouched(cuda, kind):
    """A multi-channel stream (C = 3) writing rows of outputCapacity elements, more than a call produces: channel c's
    outputs start at c * outputCapacity, the unused tail of every row and the guards around the rows keep the
    sentinel, and every row equals the single-channel monolithic call."""
    from gsdr_amd import ops
    from gsdr_amd.signals import lowpass_taps
    from gsdr_amd.stream import Stream

    D, C, T, n0, L = 4, 3, 33, 4_000_000_123, 20_000
    odt = C64 if kind == "xlate" else F32
    xd = stream_input(cuda, L, n0, False)
    taps = dev(lowpass_taps(T), cuda)
    chans = channel_list(C)
    devs = [DEV * (1 + 0.1 * c) for c in range(C)]
    s = Stream(kind, taps, D, FS, TUNE, chans, devs, first_sample_index=n0)
    untouched = np.full(1, default_sentinel(odt), dtype=np.complex64 if odt == C64 else np.float32).tobytes()
    parts, pos = [], 0
    for i, m in enumerate(chunks(L, seed=7 + len(kind), W=T + D if kind == "fm" else T)):
        case = f"multi stream {kind} call {i} ({m} samples at {pos})"
        n_out = s.outputs_for(m)
        cap = n_out + 3 + i % 2
        buf, flat = guarded(cuda, odt, C * cap, i % len(offsets(odt)))
        out = flat.view(C, cap)
        got = s.process(xd[pos:pos + m], out=out)
        assert got.shape == (C, n_out) and (n_out == 0 or got.data_ptr() == out.data_ptr()), case
        check_guards(buf, flat, what=case)
        tail = host(out[:, n_out:].contiguous())
        assert tail.tobytes() == untouched * (C * (cap - n_out)), f"{case}: wrote past a row's outputs"
        parts.append(got.clone())
        pos += m
    s.close()
    rows = torch.cat(parts, dim=1)
    for c in range(C):
        if kind == "fm":
            one = ops.fm_demod(xd, taps, FS, TUNE, chans[c], devs[c], D, n0)
        elif kind == "am":
            one = ops.am_demod(xd, taps, FS, TUNE, chans[c], D, n0)
        else:
            one = ops.xlating_fir(xd, taps, FS, TUNE, chans[c], D, n0)
        assert rows.shape[1] == one.numel() > 0
        assert host(rows[c].contiguous()).tobytes() == host(one).tobytes(), f"multi stream {kind}: row {c}"
