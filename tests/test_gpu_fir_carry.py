"""GPU: the polyphase core's carried window rows and whole-chunk tap batches (fir_engine.hpp poly_compute) leave every
output bit as it was.

The core keeps the last R - 1 window rows of each granule column in registers from one tap chunk to the next and
fetches a chunk's taps in one scalar batch. Neither may change a product or its place in an accumulator's sum, so the
witnesses are kernels of the same MAC order (chunk, column, row, element: it depends on D and the chunk rows only) that
carry a different number of rows: at D = 4 the routed call runs the R = 1 (nothing carried) or R = 2 (one row) short
tiles at these sizes and the stream object its own tile choice, while variant 0 is the headline R = 4 tile (three rows
carried) at any size. They must agree bit for bit, and meet the float bar against the C oracle.

Shapes: tap counts with one, two and three chunks of 64 taps, full and with a last chunk of a single tap; output counts
of one thread, below / at / above one 1,024-output tile, and several tiles with a ragged end.
"""
import numpy as np
import pytest
import torch

from helpers import FLOAT_TOL, bound, check_guards, guarded, normwise_err
from oracle import oracle as o
from test_gpu_nonfinite import assert_same_specials, finite_rows

pytestmark = pytest.mark.gpu

D4 = 4
TS = [1, 61, 64, 65, 127, 128, 129, 192]
NS = [1, 3, 1023, 1024, 1025, 3 * 1024 + 5]
NMAX = max(NS)
STREAM_OUTPUTS = [1, 1023, 1024, 1025, 4097]

_CACHE = {}


def dev(a, cuda):
    return torch.from_numpy(np.array(a)).to(cuda)  # (a copy: the cached cases are read-only)


def bits(y):
    return np.ascontiguousarray(y).view(np.uint32)


def taps_of(T, seed=0):
    return (np.random.default_rng(1000 + T + seed).standard_normal(T) / np.sqrt(T)).astype(np.float32)


def samples(L, seed):
    return (np.random.default_rng(seed).random(2 * L, dtype=np.float32) * 2 - 1).view(np.complex64)


def case(T, D, N):
    """(taps, x, oracle outputs, normwise bounds) for N outputs, computed once per (T, D, N). An output depends on its own
    window only, so the first n <= N outputs are the case of n outputs."""
    key = (T, D, N)
    if key not in _CACHE:
        taps, x = taps_of(T), samples((N - 1) * D + T, seed=T * 31 + D)
        _CACHE[key] = (taps, x, o.fir(taps, x, D, N), bound(taps, x, D, N))
        for a in _CACHE[key]:
            a.setflags(write=False)
    return _CACHE[key]


def stream_fir(cuda, taps_d, x_d, D, T, outputs):
    """The CF32 FIR stream fed so that its calls return `outputs` outputs each: after S samples (S - T) // D + 1 outputs
    exist."""
    from gsdr_amd.stream import Stream

    s = Stream("fir", taps_d, D)
    parts, fed, total = [], 0, 0
    for m in outputs:
        total += m
        upto = (total - 1) * D + T
        parts.append(s.process(x_d[fed:upto]).clone())
        assert parts[-1].numel() == m
        fed = upto
    s.close()
    return torch.cat(parts).cpu().numpy()


def test_one_call_equals_stream_chunks(cuda):
    """One gsdrFirFC call, the headline tile (variant 0) and stream calls of 1, 1023, 1024, 1025 and 4097 outputs:
    the same bits; the one call within the float bar of the oracle."""
    from gsdr_amd import ops

    T, N = 127, sum(STREAM_OUTPUTS)
    taps, x, ref, s = case(T, D4, N)
    td, xd = dev(taps, cuda), dev(x, cuda)
    one = ops.fir(td, xd, D4, N).cpu().numpy()
    head = ops.fir_variant(0, td, xd, D4, N).cpu().numpy()
    chunked = stream_fir(cuda, td, xd, D4, T, STREAM_OUTPUTS)
    assert np.array_equal(bits(one), bits(chunked))
    assert np.array_equal(bits(head), bits(chunked))
    assert normwise_err(one, ref, s) <= FLOAT_TOL


@pytest.mark.parametrize("T", TS)
def test_tap_chunks_and_output_counts(cuda, T):
    """nch = 1, 2, 3 tap chunks (full, and a last chunk of one tap) at every output count: routed call == headline
    tile bit for bit, both within the float bar."""
    from gsdr_amd import ops

    taps, x, ref, s = case(T, D4, NMAX)
    td, xd = dev(taps, cuda), dev(x, cuda)
    for N in NS:
        xn = xd[:(N - 1) * D4 + T]
        routed = ops.fir(td, xn, D4, N).cpu().numpy()
        head = ops.fir_variant(0, td, xn, D4, N).cpu().numpy()
        assert np.array_equal(bits(routed), bits(head)), f"T={T} N={N}"
        assert normwise_err(head, ref[:N], s[:N]) <= FLOAT_TOL, f"T={T} N={N}"


@pytest.mark.parametrize("N", [1025, NMAX])
def test_float_and_int8_samples_t197(cuda, N):
    """T = 197 (four chunks, the last of five taps), where int8 I/Q takes the float-shaped tiles: int8 == converted
    float, routed and headline tile, bit for bit; within the float bar of the oracle on the converted samples."""
    from gsdr_amd import ops

    T = 197
    taps = taps_of(T)
    x8 = np.random.default_rng(T + N).integers(-128, 128, 2 * ((N - 1) * D4 + T), dtype=np.int8)
    td, x8d = dev(taps, cuda), dev(x8, cuda)
    xfd = ops.int8_to_norm_float(x8d).view(torch.complex64)
    xf = xfd.cpu().numpy()
    want = ops.fir(td, xfd, D4, N).cpu().numpy()
    for name, got in (("float, headline tile", ops.fir_variant(0, td, xfd, D4, N)),
                      ("int8, routed", ops.fir(td, x8d, D4, N)),
                      ("int8, headline tile", ops.fir_variant(0, td, x8d, D4, N))):
        assert np.array_equal(bits(got.cpu().numpy()), bits(want)), name
    assert normwise_err(want, o.fir(taps, xf, D4, N), bound(taps, xf, D4, N)) <= FLOAT_TOL


@pytest.mark.parametrize("D", [2, 8])
def test_other_decimations_of_the_template(cuda, D):
    """D = 2 and D = 8 share the core (one and four granule columns a row): within the float bar, and equal to the
    stream's calls bit for bit."""
    from gsdr_amd import ops

    T, N = 127, sum(STREAM_OUTPUTS[:4])
    taps, x, ref, s = case(T, D, N)
    td, xd = dev(taps, cuda), dev(x, cuda)
    one = ops.fir(td, xd, D, N).cpu().numpy()
    assert normwise_err(one, ref, s) <= FLOAT_TOL
    assert np.array_equal(bits(one), bits(stream_fir(cuda, td, xd, D, T, STREAM_OUTPUTS[:4])))


def test_nonfinite_in_carried_rows(cuda):
    """+-Inf and NaN in the rows a thread of the headline tile carries from chunk 0 to chunk 1 (rows 16, 17, 18 of its
    window: input rows 4 t + 16 ...), in the column of the padding tap (tap 127 of 128: sample 3 of a row, which
    makes the padding product of output (s - 127) / 4 a NaN the reference never forms) and in column 0. Finiteness,
    signs and the finite outputs match the oracle for the routed call and the headline tile."""
    from gsdr_amd import ops

    T, N = 127, 2051
    taps = taps_of(T)
    x = samples((N - 1) * D4 + T, seed=5).copy()
    f = x.view(np.float32)
    for t, u, col, part, val in ((5, 16, 3, 0, np.inf), (40, 17, 3, 1, -np.inf), (90, 18, 3, 0, np.nan),
                                 (130, 16, 0, 1, -np.inf), (200, 17, 0, 0, np.nan), (300, 18, 0, 1, np.inf)):
        f[2 * ((4 * t + u) * D4 + col) + part] = val
    ref = o.fir(taps, x, D4, N)
    ok = finite_rows(ref)
    assert 0 < np.count_nonzero(~ok) < N // 4
    s = bound(taps, x, D4, N)
    td, xd = dev(taps, cuda), dev(x, cuda)
    for name, got in (("routed", ops.fir(td, xd, D4, N)), ("headline tile", ops.fir_variant(0, td, xd, D4, N))):
        y = got.cpu().numpy()
        assert_same_specials(y, ref)
        assert normwise_err(y[ok], ref[ok], s[ok]) <= FLOAT_TOL, name


def test_guards_untouched(cuda):
    """N = 1025 (one whole tile and one output of the next) into a guarded buffer: nothing written outside it."""
    from gsdr_amd import ops

    T, N = 127, 1025
    taps, x, ref, s = case(T, D4, NMAX)
    td, xd = dev(taps, cuda), dev(x[:(N - 1) * D4 + T], cuda)
    for name, call in (("routed", lambda out: ops.fir(td, xd, D4, N, out=out)),
                       ("headline tile", lambda out: ops.fir_variant(0, td, xd, D4, N, out=out))):
        buf, view = guarded(cuda, torch.complex64, N)
        got = call(view)
        assert got.data_ptr() == view.data_ptr()
        check_guards(buf, view, what=name)
        assert normwise_err(view.cpu().numpy(), ref[:N], s[:N]) <= FLOAT_TOL, name
