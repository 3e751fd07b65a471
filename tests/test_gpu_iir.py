"""GPU parity: gsdrIirFF / gsdrIirCC (include/gsdr/iir.h, a true recursive IIR with history) against
the float64 oracle (itself pinned to scipy.signal.lfilter, tests/test_oracle_iir.py). The GPU runs the
recursion as a parallel scan with the state, scan and transition matrices in double (samples float32
in HBM), so within one call the error relative to the output's peak,
e = max|y_gpu - y_oracle| / max(1, max|y|), is bounded by IIR_TOL = 1e-6 for every filter tested --
well under e_seq32, the same measure for a plain sequential float32 loop (oracle_iir_f32, what the
reference's per-sample loop computes), which reaches 1e-4..1e-3 on the high-order filters below.
Across calls the state travels through the caller's float32 history buffers (the reference ABI), whose
rounding the next call's outputs inherit; that end-to-end check uses max(IIR_TOL, 4 * e_seq32)."""
import ctypes
import os

import numpy as np
import pytest
import torch
from scipy import signal

from helpers import check_guards, guarded
from oracle import oracle as o

pytestmark = pytest.mark.gpu

IIR_TOL = 1e-6


PROBES = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "build", "probes",
                      "libgsdr_probes.so")
HIP_ERROR_NOT_SUPPORTED, HIP_ERROR_LAUNCH_FAILURE = 801, 719
_probes = []


def probes_lib():
    """The tuning-probe build (make probes), which alone carries the single-pass IIR kernel; the product
    library runs the multi-pass scan only. Missing on a GPU box = a failed test, not a skip."""
    if not _probes:
        assert os.path.exists(PROBES), f"{PROBES} missing (make probes)"
        lib = ctypes.CDLL(PROBES)
        p, sz = ctypes.c_void_p, ctypes.c_size_t
        for name in ("gsdrxIirFFSinglePass", "gsdrxIirCCSinglePass"):
            fn = getattr(lib, name)
            fn.restype = ctypes.c_int
            fn.argtypes = [p, p, sz, p, p, p, p, sz, ctypes.c_uint32, ctypes.c_int32, p]
        lib.gsdrxIirSinglePassStatus.restype = ctypes.c_int
        lib.gsdrxIirSinglePassStatus.argtypes = [ctypes.c_int32, p]
        _probes.append(lib)
    return _probes[0]


def single_pass(bd, ad, xd, xh=None, yh=None, max_polls=1 << 22):
    """gsdrxIirFFSinglePass / CC of the probes build on torch tensors (ops.iir's contract); returns (rc, y)."""
    lib = probes_lib()
    y = torch.empty_like(xd)
    fn = lib.gsdrxIirCCSinglePass if xd.dtype == torch.complex64 else lib.gsdrxIirFFSinglePass
    ptr = lambda t: None if t is None else t.data_ptr()  # noqa: E731
    rc = fn(bd.data_ptr(), ad.data_ptr(), bd.numel(), ptr(xh), ptr(yh), xd.data_ptr(), y.data_ptr(), xd.numel(),
            max_polls, xd.device.index, torch.cuda.current_stream(xd.device).cuda_stream)
    return rc, y


@pytest.fixture(params=["scan", "single_pass"])
def iir_fn(request, cuda):
    """Every parity test runs on both IIR formulations: the multi-pass scan (gsdrIirFF / gsdrIirCC, the product) and
    the single-pass kernel (probes build, chosen per call; K <= 9 only -- it refuses larger K with
    hipErrorNotSupported, which those cases check). After each single-pass call the device status word must be
    clear (no tile gave up waiting)."""
    from gsdr_amd import ops

    if request.param == "scan":
        return ops.iir

    def run(bd, ad, xd, xh=None, yh=None):
        rc, y = single_pass(bd, ad, xd, xh, yh)
        if bd.numel() > 9:
            assert rc == HIP_ERROR_NOT_SUPPORTED
            pytest.skip("single-pass kernel: K <= 9")
        assert rc == 0
        assert probes_lib().gsdrxIirSinglePassStatus(cuda.index, torch.cuda.current_stream(cuda).cuda_stream) == 0
        return y

    return run


def bar(b, a, x, want, xh=None, yh=None):
    return max(IIR_TOL, 4 * err(o.iir_f32(b, a, x, xh, yh), want))


def design(kind, order):
    if kind == "butter":
        b, a = signal.butter(order, 0.1)
    else:
        rng = np.random.default_rng(order)
        a = np.poly(rng.uniform(-0.8, 0.8, order))
        b = rng.uniform(-0.5, 0.5, order + 1)
    return b.astype(np.float32), a.astype(np.float32)


def dev(a, cuda):
    return torch.from_numpy(np.ascontiguousarray(a)).to(cuda)


def err(got, want):
    return float(np.max(np.abs(got - want))) / max(1.0, float(np.max(np.abs(want))))


SIZES = [1, 2, 5, 127, 128, 129, 1000, 8192, 8193, 128 * 64 + 1, 128 * 64 * 64 + 7, (1 << 22) + 3, 1 << 24]


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("cplx", [False, True])
def test_iir_butter4_sizes(cuda, iir_fn, n, cplx):
    b, a = design("butter", 4)
    rng = np.random.default_rng(n)
    x = rng.uniform(-1, 1, n).astype(np.float32)
    if cplx:
        x = (x + 1j * rng.uniform(-1, 1, n)).astype(np.complex64)
    y = iir_fn(dev(b, cuda), dev(a, cuda), dev(x, cuda)).cpu().numpy()
    want, _, _ = o.iir(b, a, x)
    e = err(y, want)
    print(f"n={n} cplx={cplx} err={e:.2e}")
    assert e <= IIR_TOL


@pytest.mark.parametrize("kind,order", [("butter", 1), ("butter", 2), ("butter", 3), ("butter", 6), ("poles", 5),
                                        ("poles", 9), ("poles", 16), ("poles", 20), ("poles", 31)])
def test_iir_orders_with_history(cuda, iir_fn, kind, order):
    b, a = design(kind, order)
    rng = np.random.default_rng(order)
    n = 200_003
    x = rng.uniform(-1, 1, n).astype(np.float32)
    xh = rng.uniform(-1, 1, order).astype(np.float32)
    yh = rng.uniform(-1, 1, order).astype(np.float32)
    xh_d, yh_d = dev(xh, cuda), dev(yh, cuda)
    y = iir_fn(dev(b, cuda), dev(a, cuda), dev(x, cuda), xh_d, yh_d).cpu().numpy()
    want, xh2, yh2 = o.iir(b, a, x, xh, yh)
    e = err(y, want)
    print(f"{kind}{order} err={e:.2e} seq32={err(o.iir_f32(b, a, x, xh, yh), want):.2e}")
    assert e <= IIR_TOL
    assert np.array_equal(xh_d.cpu().numpy(), xh2)  # last K-1 inputs, exactly
    assert np.array_equal(yh_d.cpu().numpy(), y[::-1][:order])  # last K-1 outputs as written


@pytest.mark.parametrize("order", [4, 6])
@pytest.mark.parametrize("cplx", [False, True])
def test_iir_chunked_calls_continue(cuda, iir_fn, order, cplx):
    """Consecutive calls continue one recursion through the history buffers. Every call is checked
    against the float64 oracle started from the history the GPU handed over (the property that holds
    for any filter); for the well-conditioned 4th-order filter the concatenation is also checked
    against one monolithic evaluation. (Direct-form 6th order at 0.1 fs amplifies a state difference
    ~200-1000x: float32 history values that are each within rounding of the true state can move the
    next call's outputs by ~1e-2, as they would for any float32 implementation fed those values.)"""
    b, a = design("butter", order)
    rng = np.random.default_rng(7)
    n = 100_000
    x = rng.uniform(-1, 1, n).astype(np.float32)
    if cplx:
        x = (x + 1j * rng.uniform(-1, 1, n)).astype(np.complex64)
    want, _, _ = o.iir(b, a, x)
    xd = dev(x, cuda)
    dt = torch.complex64 if cplx else torch.float32
    xh = torch.zeros(order, dtype=dt, device=cuda)
    yh = torch.zeros(order, dtype=dt, device=cuda)
    bd, ad = dev(b, cuda), dev(a, cuda)
    parts, pos = [], 0
    for m in (1, 2, 3, 127, 129, 5000, 20000, n):
        m = min(m, n - pos)
        if m == 0:
            break
        hx, hy = xh.cpu().numpy().copy(), yh.cpu().numpy().copy()
        y = iir_fn(bd, ad, xd[pos:pos + m], xh, yh).cpu().numpy()
        w, _, _ = o.iir(b, a, x[pos:pos + m], hx, hy)
        assert err(y, w) <= IIR_TOL, (pos, m)
        parts.append(y)
        pos += m
    if order == 4:
        assert err(np.concatenate(parts), want) <= bar(b, a, x, want)


def test_iir_impulse_and_validation(cuda):
    from gsdr_amd import abi, ops

    c = np.float32(0.1)
    b = np.array([c, c], np.float32)
    a = np.array([1.0, -(1.0 - c)], np.float32)
    x = np.zeros(300, np.float32)
    x[0] = 1.0
    y = ops.iir(dev(b, cuda), dev(a, cuda), dev(x, cuda)).cpu().numpy()
    want, _, _ = o.iir(b, a, x)
    assert np.max(np.abs(y - want)) < 1e-6
    st = torch.cuda.current_stream(cuda).cuda_stream
    bd = dev(np.ones(40, np.float32), cuda)
    xd = dev(x, cuda)
    yd = torch.empty_like(xd)
    for K in (0, 1, 33):  # reference limits 2 <= K <= 32
        assert abi.lib.gsdrIirFF(bd.data_ptr(), bd.data_ptr(), K, None, None, xd.data_ptr(), yd.data_ptr(), 300,
                                 cuda.index, st) != 0
    assert abi.lib.gsdrIirFFCustom(bd.data_ptr(), bd.data_ptr(), 3, None, None, xd.data_ptr(), yd.data_ptr(), 300,
                                   0, cuda.index, st) != 0
    assert abi.lib.gsdrIirFFCustom(bd.data_ptr(), bd.data_ptr(), 3, None, None, xd.data_ptr(), yd.data_ptr(), 0,
                                   8, cuda.index, st) == 0


@pytest.mark.parametrize("order,n", [(4, 1 << 25), (4, (1 << 25) + 1), (8, (1 << 21) + 3), (2, (1 << 22) + 9),
                                     (1, 3 * (1 << 21) + 1), (6, 64 * 64 * 32 * 3 + 5)])
def test_iir_scan_paths(cuda, iir_fn, order, n):
    """Levels >= 2 and level 1's down-sweep run in one launch (k_iir_scan_upper) up to 256 level-2
    elements (2^25 samples); past that, the per-level launches. Inputs at and past the limit, partial
    groups at every level, and a level-2 scan of one group (levels == 2), each against the float64
    oracle with history."""
    b, a = design("poles", order)
    rng = np.random.default_rng(n)
    x = rng.uniform(-1, 1, n).astype(np.float32)
    xh = rng.uniform(-1, 1, order).astype(np.float32)
    yh = rng.uniform(-1, 1, order).astype(np.float32)
    y = iir_fn(dev(b, cuda), dev(a, cuda), dev(x, cuda), dev(xh, cuda), dev(yh, cuda)).cpu().numpy()
    want, _, _ = o.iir(b, a, x, xh, yh)
    e = err(y, want)
    print(f"order={order} n={n} err={e:.2e}")
    assert e <= IIR_TOL


@pytest.mark.parametrize("order,n", [(16, 4101), (31, 4101), (16, 131105), (31, 131105), (4, 131105)])
def test_iir_complex_scan_routes_with_history(cuda, order, n):
    """Complex samples with complex histories through the scan routes the real-valued tests leave out. Orders 16
    and 31 run the unfused chunk passes: 4101 samples are 129 chunks, so level 0 itself goes through
    k_iir_scan_rest (last group and last chunk partial); 131105 samples are 4098 chunks (E1 = 65, E2 = 2), level 0
    by k_iir_up / k_iir_down and levels 1, 2 in k_iir_scan_rest, a partial group at every level. Order 4 at
    131105 samples is the fused route with levels == 2: k_iir_scan_upper on both components from a non-zero
    entry state. The multi-pass scan only (ops.iir): the single-pass kernel refuses K > 9."""
    from gsdr_amd import ops

    b, a = design("poles", order)
    rng = np.random.default_rng(1000 * order + n)

    def cplx(m):
        return (rng.uniform(-1, 1, m) + 1j * rng.uniform(-1, 1, m)).astype(np.complex64)

    x, xh, yh = cplx(n), cplx(order), cplx(order)
    xh_d, yh_d = dev(xh, cuda), dev(yh, cuda)
    y = ops.iir(dev(b, cuda), dev(a, cuda), dev(x, cuda), xh_d, yh_d).cpu().numpy()
    want, xh2, yh2 = o.iir(b, a, x, xh, yh)
    e = err(y, want)
    print(f"poles{order} n={n} complex err={e:.2e}")
    assert e <= IIR_TOL
    assert np.array_equal(xh_d.cpu().numpy(), xh2)  # last K-1 inputs, exactly
    assert np.array_equal(yh_d.cpu().numpy(), y[::-1][:order])  # last K-1 outputs as written


@pytest.mark.parametrize("order", [1, 2])
@pytest.mark.parametrize("n", [3 * 8192 + 1, 3 * (1 << 21) + 5])
@pytest.mark.parametrize("cplx", [False, True])
def test_iir_slow_decay_carries(cuda, iir_fn, order, n, cplx):
    """Poles at radius 1 - 1e-6: the state entering a tile carries weight ~e^-2 across a superblock of 2^21
    samples, so a carry dropped or misordered anywhere in the single-pass scan (chunks within a wave,
    waves within a tile, tiles within a superblock, superblocks) shows at O(1) rather than under the
    tolerance, as it would for a fast-decaying filter. DC input plus noise keeps the output O(1)."""
    r = 1.0 - 1e-6
    a = np.poly([r] if order == 1 else [r * np.exp(3e-3j), r * np.exp(-3e-3j)]).real.astype(np.float32)
    b = np.zeros(order + 1, np.float32)
    b[0] = np.float32(np.sum(a.astype(np.float64)))  # unit DC gain
    rng = np.random.default_rng(n + order)
    x = rng.uniform(0, 1, n).astype(np.float32)
    if cplx:
        x = (x + 1j * rng.uniform(-1, 0, n)).astype(np.complex64)
    y = iir_fn(dev(b, cuda), dev(a, cuda), dev(x, cuda)).cpu().numpy()
    want, _, _ = o.iir(b, a, x)
    e = float(np.max(np.abs(y - want))) / float(np.max(np.abs(want)))
    print(f"order={order} n={n} cplx={cplx} err={e:.2e} peak={float(np.max(np.abs(want))):.3g}")
    assert e <= 1e-5


def test_iir_single_pass_give_up_is_reported(cuda):
    """The single-pass kernel's bounded waits: with maxPolls = 0 every tile that has to wait for an earlier tile
    gives up at once. The call itself returns hipSuccess (the kernel cannot fail a launch), but
    gsdrxIirSinglePassStatus then reports hipErrorLaunchFailure (and clears the word), the outputs past the
    first tile are NaN rather than plausible values, and the caller's history buffers are left as they were (the
    last tile did not wait for the readers). The first tile, which waits for nothing, is still exact."""
    lib = probes_lib()
    st = torch.cuda.current_stream(cuda).cuda_stream
    assert lib.gsdrxIirSinglePassStatus(cuda.index, st) == 0
    b, a = design("butter", 4)
    bd, ad = dev(b, cuda), dev(a, cuda)
    n = 5 * 8192 + 17  # six tiles of 8192 real samples
    x = np.random.default_rng(11).uniform(-1, 1, n).astype(np.float32)
    xh0 = np.full(4, 0.25, np.float32)
    yh0 = np.full(4, -0.5, np.float32)
    xh, yh = dev(xh0.copy(), cuda), dev(yh0.copy(), cuda)
    rc, y = single_pass(bd, ad, dev(x, cuda), xh, yh, max_polls=0)
    assert rc == 0
    assert lib.gsdrxIirSinglePassStatus(cuda.index, st) == HIP_ERROR_LAUNCH_FAILURE
    assert lib.gsdrxIirSinglePassStatus(cuda.index, st) == 0  # cleared by the query
    yc = y.cpu().numpy()
    want, _, _ = o.iir(b, a, x, xh0, yh0)
    assert err(yc[:8192], want[:8192]) <= IIR_TOL
    assert np.isnan(yc[8192:]).all()
    assert np.array_equal(xh.cpu().numpy(), xh0) and np.array_equal(yh.cpu().numpy(), yh0)
    # the normal bound on the same call: exact, status clear, history advanced
    rc, y = single_pass(bd, ad, dev(x, cuda), xh, yh)
    assert rc == 0 and lib.gsdrxIirSinglePassStatus(cuda.index, st) == 0
    assert err(y.cpu().numpy(), want) <= IIR_TOL
    assert not np.array_equal(xh.cpu().numpy(), xh0)


# The edges of the contract in include/gsdr/iir.h, on the multi-pass scan (ops.iir): output and history writes stay
# inside their buffers at every alignment, calls shorter than the history, one history buffer alone, a[0] unused.
# Orders: every compiled state size P (1, 2, 4, 8, 16, 31), at it and just above the one below (K - 1 < P, where the
# history write has to stop short of the compiled state; orders 16, 17, 31 run the unfused chunk passes).
EDGE_ORDERS = [1, 2, 3, 4, 5, 8, 9, 16, 17, 31]


def samples(rng, m, cplx):
    v = rng.uniform(-1, 1, m).astype(np.float32)
    return (v + 1j * rng.uniform(-1, 1, m)).astype(np.complex64) if cplx else v


def shifted(t, off):
    """The same samples `off` elements off 16-byte alignment (run_fir's construction, test_gpu_fir.py)."""
    if off == 0:
        return t
    y = torch.cat([torch.zeros(off, dtype=t.dtype, device=t.device), t])[off:]
    assert t.data_ptr() % 16 == 0 and y.data_ptr() % 16 == (off * t.element_size()) % 16
    return y


def guarded_history(cuda, h, off=1):
    """A history buffer of K - 1 samples in the middle of a sentinel buffer: (buf, view), view holding h."""
    buf, view = guarded(cuda, torch.complex64 if np.iscomplexobj(h) else torch.float32, h.size, off)
    view.copy_(torch.from_numpy(h))
    return buf, view


def history_after(new, before):
    """The K - 1 newest samples, newest first, of `before` (newest first) followed by `new` (oldest first)."""
    return np.concatenate([new[::-1], before])[:before.size]


@pytest.mark.parametrize("cplx", [False, True])
@pytest.mark.parametrize("order", EDGE_ORDERS)
def test_iir_output_bounds_and_alignment(cuda, order, cplx):
    """k_iir_chunks picks whole-tile float4 loads / stores from aligned16(x) && aligned16(y) and writes the ragged last
    tile per sample: one sample to two tiles of 4,096 complex / 8,192 real samples (one below / above each tile
    edge, one chunk of 32 +- 1), and levels = 2 on both routes (131,105 samples, orders 4 and 31), with the input
    and the output each on and off 16-byte alignment. The output is a view inside a sentinel buffer, and so are both
    histories: nothing outside them changes, the outputs meet the float64 oracle, and they are the same bits at
    every alignment."""
    from gsdr_amd import ops

    b, a = design("poles", order)
    bd, ad = dev(b, cuda), dev(a, cuda)
    rng = np.random.default_rng(100 * order + cplx)
    dt = torch.complex64 if cplx else torch.float32
    sizes = [1, 2, 5, 31, 33, 2047, 2049, 4095, 4097, 8195] + ([131105] if order in (4, 31) else [])
    offs = [(0, 0), (1, 0), (0, 1), (1, 1)] + ([] if cplx else [(3, 3)])
    for n in sizes:
        x, xh, yh = samples(rng, n, cplx), samples(rng, order, cplx), samples(rng, order, cplx)
        want, xh2, _ = o.iir(b, a, x, xh, yh)
        xd = dev(x, cuda)
        first = None
        for xo, yo in offs:
            case = f"order {order} complex={cplx} n={n} offsets x {xo} y {yo}"
            hx_buf, hx = guarded_history(cuda, xh)
            hy_buf, hy = guarded_history(cuda, yh)
            buf, view = guarded(cuda, dt, n, yo)
            got = ops.iir(bd, ad, shifted(xd, xo), hx, hy, out=view)
            assert got.data_ptr() == view.data_ptr() and got.shape == view.shape, case
            check_guards(buf, view, what=case + ", output")
            check_guards(hx_buf, hx, what=case + ", inputHistory")
            check_guards(hy_buf, hy, what=case + ", outputHistory")
            y = view.cpu().numpy()
            if first is None:
                first = y
                e = err(y, want)
                assert e <= IIR_TOL, f"{case}: error {e:.2e}"
            else:
                assert y.tobytes() == first.tobytes(), f"{case}: outputs differ from the aligned call's"
            assert hx.cpu().numpy().tobytes() == xh2.tobytes(), case
            assert np.array_equal(hy.cpu().numpy(), history_after(y, yh)), case


@pytest.mark.parametrize("cplx", [False, True])
@pytest.mark.parametrize("order", EDGE_ORDERS)
def test_iir_history_write_stops_at_k_minus_1(cuda, order, cplx):
    """The final pass's last chunk holds the compiled state (P entries) and writes K - 1 of them to the caller's
    history buffers (the i < Pk guard of k_iir_chunks): with both buffers K - 1 samples in the middle of sentinel
    buffers, at every alignment of the buffer, the sentinels on both sides survive calls shorter than, as long as and
    longer than the history."""
    from gsdr_amd import ops

    b, a = design("poles", order)
    bd, ad = dev(b, cuda), dev(a, cuda)
    rng = np.random.default_rng(200 * order + cplx)
    for n in (1, order, 33, 2049):
        for off in (0, 1) if cplx else (0, 1, 2, 3):
            case = f"order {order} complex={cplx} n={n} history offset {off}"
            x, xh, yh = samples(rng, n, cplx), samples(rng, order, cplx), samples(rng, order, cplx)
            hx_buf, hx = guarded_history(cuda, xh, off)
            hy_buf, hy = guarded_history(cuda, yh, off)
            y = ops.iir(bd, ad, dev(x, cuda), hx, hy).cpu().numpy()
            check_guards(hx_buf, hx, what=case + ", inputHistory")
            check_guards(hy_buf, hy, what=case + ", outputHistory")
            assert hx.cpu().numpy().tobytes() == history_after(x, xh).tobytes(), case
            assert hy.cpu().numpy().tobytes() == history_after(y, yh).tobytes(), case


@pytest.mark.parametrize("cplx", [False, True])
@pytest.mark.parametrize("order", EDGE_ORDERS)
def test_iir_short_calls_with_history(cuda, order, cplx):
    """numElements below, at and above K - 1 (iir.h: the histories then keep older entries): the input history is the
    K - 1 newest of (old history, x) exactly, the output history the K - 1 newest of (old history, y as written)
    exactly -- old entries travel float -> double -> float unrounded -- and a second call continues from them as the
    float64 oracle does from the same handed-over values. (K - 2 = 0 at order 1: a call with no samples succeeds and
    leaves the histories alone.)"""
    from gsdr_amd import ops

    K = order + 1
    b, a = design("poles", order)
    bd, ad = dev(b, cuda), dev(a, cuda)
    rng = np.random.default_rng(300 * order + cplx)
    for n in sorted({1, 2, K - 2, K - 1, K}):
        case = f"order {order} complex={cplx} n={n}"
        x, xh, yh = samples(rng, n, cplx), samples(rng, order, cplx), samples(rng, order, cplx)
        hx_buf, hx = guarded_history(cuda, xh)
        hy_buf, hy = guarded_history(cuda, yh)
        y = ops.iir(bd, ad, dev(x, cuda), hx, hy).cpu().numpy()
        check_guards(hx_buf, hx, what=case + ", inputHistory")
        check_guards(hy_buf, hy, what=case + ", outputHistory")
        xh1, yh1 = hx.cpu().numpy(), hy.cpu().numpy()
        assert xh1.tobytes() == history_after(x, xh).tobytes(), case
        assert yh1.tobytes() == history_after(y, yh).tobytes(), case
        if n:
            want, _, _ = o.iir(b, a, x, xh, yh)
            assert err(y, want) <= IIR_TOL, case
        x2 = samples(rng, 50, cplx)
        y2 = ops.iir(bd, ad, dev(x2, cuda), hx, hy).cpu().numpy()
        want2, xh2, _ = o.iir(b, a, x2, xh1, yh1)
        assert err(y2, want2) <= IIR_TOL, case + ", second call"
        assert hx.cpu().numpy().tobytes() == xh2.tobytes(), case + ", second call"
        assert hy.cpu().numpy().tobytes() == history_after(y2, yh1).tobytes(), case + ", second call"


@pytest.mark.parametrize("which", ["input", "output"])
@pytest.mark.parametrize("cplx", [False, True])
@pytest.mark.parametrize("order", [4, 16])
def test_iir_one_history_buffer(cuda, order, cplx, which):
    """Only inputHistory, or only outputHistory (the other null: zero state, not written): the outputs are the
    oracle's for the same pattern, and the buffer that was given is updated as when both are."""
    from gsdr_amd import ops

    b, a = design("poles", order)
    bd, ad = dev(b, cuda), dev(a, cuda)
    rng = np.random.default_rng(400 * order + cplx)
    for n in (3, 5000):
        case = f"order {order} complex={cplx} n={n} {which} history only"
        x, h = samples(rng, n, cplx), samples(rng, order, cplx)
        h_buf, hd = guarded_history(cuda, h)
        if which == "input":
            want, _, _ = o.iir(b, a, x, h, None)
            y = ops.iir(bd, ad, dev(x, cuda), hd, None).cpu().numpy()
        else:
            want, _, _ = o.iir(b, a, x, None, h)
            y = ops.iir(bd, ad, dev(x, cuda), None, hd).cpu().numpy()
        check_guards(h_buf, hd, what=case)
        e = err(y, want)
        assert e <= IIR_TOL, f"{case}: error {e:.2e}"
        assert hd.cpu().numpy().tobytes() == history_after(x if which == "input" else y, h).tobytes(), case


@pytest.mark.parametrize("a0", [7.5, 0.0, float("nan")])
@pytest.mark.parametrize("order", [2, 8, 31])
def test_iir_a0_is_not_used(cuda, order, a0):
    """iir.h: a[0] is taken as 1 whatever it holds. The outputs and both histories are the same bits as with
    a[0] = 1, for real and complex samples."""
    from gsdr_amd import ops

    b, a = design("poles", order)
    assert a[0] == 1.0
    a_other = a.copy()
    a_other[0] = a0
    n = 5000
    for cplx in (False, True):
        rng = np.random.default_rng(500 * order + cplx)
        x, xh, yh = samples(rng, n, cplx), samples(rng, order, cplx), samples(rng, order, cplx)
        got = []
        for coeffs in (a, a_other):
            hx, hy = dev(xh.copy(), cuda), dev(yh.copy(), cuda)
            y = ops.iir(dev(b, cuda), dev(coeffs, cuda), dev(x, cuda), hx, hy)
            got.append((y.cpu().numpy(), hx.cpu().numpy(), hy.cpu().numpy()))
        want, _, _ = o.iir(b, a, x, xh, yh)
        assert err(got[0][0], want) <= IIR_TOL
        for one, other in zip(*got):
            assert np.all(np.isfinite(one.view(np.float32))) and one.tobytes() == other.tobytes(), (order, a0, cplx)
