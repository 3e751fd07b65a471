"""GPU: stream order. Every entry point takes a hipStream_t and promises that its work is ordered on it (DESIGN.md,
the headers); a receiver calls back to back on several non-blocking streams with a copy-in ahead of each call and
no host sync. Here every family runs that way, through helpers.run_gated():

  reference  the true inputs in the live buffers, the call on the default stream with the device synchronised;
  arm        every input refilled with a decoy (a second draw of the same distribution), every output with a sentinel;
  gated run  on a fresh non-blocking side stream: a sleeping kernel (the gate), the copies that bring the true inputs
             back, the call(s), a snapshot of every output and in/out buffer, an event;
  condition  the event has not fired when the host is done enqueueing (else the case fails as inconclusive);
  compare    every snapshot equals its synchronised reference bit for bit.

Anything the library issues on another stream (a kernel, a hipMemsetAsync, a history copy, a workspace used across
streams) or assumes finished on the host finds an idle device and runs ahead of the copy-in, on the decoys. Two
control cases issue the call on the default stream on purpose and must see a mismatch: if they do not, the runtime
serialises the streams and nothing in this module proves anything.

The side streams are torch's non-blocking ones, each checked before use to run independently of the default stream
(helpers.side_streams): the runtime places streams on a few hardware queues, and behind a side stream that shares
the default stream's queue a launch on the wrong stream waits for the gate with everything else. Before that check,
a scratch build whose zero-tap hipMemsetAsync went to stream 0 passed test_fir on such a stream.

The gate is torch.cuda._sleep(cycles), calibrated once a session by the `gate` fixture (one fixed sleep timed with
a pair of events); it ends by itself. Measured on an MI355X: _sleep(2,000,000) takes 0.84 ms, 2,372 to 2,387 cycles
a microsecond, so the 20 ms gate is 47.4 to 47.7 million cycles. 20 ms was never too short: enqueueing a case takes
well under a millisecond, and the module's 105 cases run in under 6 s.
"""
import numpy as np
import pytest
import torch

from channelizer_ref import build_plan_program as build_channelizer_plan
from helpers import GatedJob, mismatches, raw_bytes, run_gated, run_gated_jobs, stream_sentinel
from resample_ref import build_plan_program as build_resample_plan
from resample_ref import inputs_for

pytestmark = pytest.mark.gpu

GATE_MS = 20.0            # target length of the gate
PROBE_CYCLES = 2_000_000  # the calibration sleep
FS, TUNE, CHAN, DEV = 1.0e6, 0.0, 1.0e5, 2.0e4
N0 = 77_777
MCH = [1.0e5, -2.5e5, 3.3e4, 0.0, -4.4e5, 1.7e5, 2.9e5, -1.1e5, 4.0e5, -3.0e5, 6.0e4, -6.0e4, 2.2e5, -2.2e5, 1.3e5,
       -1.3e5, 3.7e5]
TILE, GENERIC = 0, 1


@pytest.fixture(scope="module")
def gate(cuda):
    """Cycles of torch.cuda._sleep for a GATE_MS gate: the rate of one PROBE_CYCLES sleep between two events (the
    second of two, so that the first launch's set-up is not in it)."""
    ms = 0.0
    for _ in range(2):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize(cuda)
        a.record()
        torch.cuda._sleep(PROBE_CYCLES)
        b.record()
        b.synchronize()
        ms = a.elapsed_time(b)
    assert ms > 0.0
    rate = PROBE_CYCLES / ms
    cycles = int(rate * GATE_MS)
    print(f"gate: _sleep({PROBE_CYCLES}) took {ms:.3f} ms = {rate / 1e3:.1f} cycles/us; {GATE_MS} ms = {cycles} cycles")
    return cycles


@pytest.fixture(scope="module")
def tables(cuda):
    """Both QPSK256 tables, before any gate (gsdrQpsk256InitConstellation synchronises its stream by contract)."""
    from gsdr_amd import ops

    ops.qpsk256_init(0, 1.0)
    ops.qpsk256_init(1, 1.0)
    torch.cuda.synchronize(cuda)


def draw(kind, n, seed):
    """n values of a distribution: "f" / "c" uniform in [-1, 1), "i8" n int8 I/Q samples (2 n elements), "u8" bytes,
    "taps" / "ctaps" both signs and none zero."""
    rng = np.random.default_rng(seed)
    if kind == "f":
        return rng.uniform(-1, 1, n).astype(np.float32)
    if kind == "c":
        return (rng.uniform(-1, 1, n) + 1j * rng.uniform(-1, 1, n)).astype(np.complex64)
    if kind == "i8":
        return rng.integers(-128, 128, 2 * n, dtype=np.int8)
    if kind == "u8":
        return rng.integers(0, 256, n, dtype=np.uint8)
    t = (rng.uniform(0.1, 1.0, n) * rng.choice([-1.0, 1.0], n) / np.sqrt(max(n, 1))).astype(np.float32)
    if kind == "ctaps":
        t = (t + 1j * draw("taps", n, seed + 7)).astype(np.complex64)
    return t


def slot(cuda, true, decoy):
    """(live, true, decoy) on the device from two host arrays."""
    t = torch.from_numpy(np.ascontiguousarray(true)).to(cuda)
    d = torch.from_numpy(np.ascontiguousarray(decoy)).to(cuda)
    assert t.numel() == 0 or not torch.equal(raw_bytes(t), raw_bytes(d))
    return torch.empty_like(t), t, d


def drawn(cuda, kind, n, seed):
    return slot(cuda, draw(kind, n, seed), draw(kind, n, seed + 1000))


def empty(cuda, dtype, *shape):
    return torch.empty(shape, dtype=dtype, device=cuda)


def check(pairs, what=""):
    bad = mismatches(pairs)
    assert not bad, f"{what}: gated buffers {bad} of {len(pairs)} differ from the synchronised run"
    for ref, _ in pairs:   # and the reference itself was written: no output is still all sentinel
        if ref.numel():
            assert not bool((raw_bytes(ref) == raw_bytes(torch.full_like(ref, stream_sentinel(ref.dtype)))).all()), what


# ------------------------------------------------------------------------------------------------ controls

def test_control_kernel_on_the_wrong_stream_is_seen(cuda, gate):
    """ops.fir issued on the idle default stream while its copy-in waits behind the gate: it filters the decoy."""
    from gsdr_amd import ops

    D, T, N = 4, 127, 8192
    taps, x = drawn(cuda, "taps", T, 1), drawn(cuda, "c", (N - 1) * D + T, 2)
    out = empty(cuda, torch.complex64, N)
    pairs = run_gated(cuda, gate, [taps, x], [out], [lambda phase: ops.fir(taps[0], x[0], D, N, out=out)],
                      on_default_stream=True)
    assert mismatches(pairs) == [0], "the default and the side stream are serialised: the gated cases prove nothing"


def test_control_memset_on_the_wrong_stream_is_seen(cuda, gate):
    """The zero-tap routes' fault, played by torch: tensor.zero_() on the idle default stream zeroes the output at
    once, and the sentinel written behind the gate (in stream order: before the call) then covers the zeros."""
    out = empty(cuda, torch.complex64, 8192)
    pairs = run_gated(cuda, gate, [], [out], [lambda phase: out.zero_()], on_default_stream=True)
    assert bool((raw_bytes(pairs[0][0]) == 0).all())
    assert mismatches(pairs) == [0], "the default and the side stream are serialised: the gated cases prove nothing"


# ------------------------------------------------------------------------------------------------ FIR

FIR_CASES = [("FF", 1, 8), ("FC", 4, 127), ("CC", 3, 63), ("FC", 4, 6000), ("I8", 4, 127), ("I8", 3, 127), ("FC", 4, 0)]


@pytest.mark.parametrize("tt,D,T", FIR_CASES, ids=[f"{t}-D{d}-T{n}" for t, d, n in FIR_CASES])
def test_fir(cuda, gate, tt, D, T):
    """FF, the default polyphase route, CC, a long filter on the generic route (test_fir_long_filters), the int8
    matrix-core route and int8 at D = 3, and the zero-tap hipMemsetAsync route over a non-zero sentinel."""
    from gsdr_amd import ops

    N = 5003
    L = (N - 1) * D + max(T, 1)
    taps = drawn(cuda, "ctaps" if tt == "CC" else "taps", T, T + D)
    x = drawn(cuda, {"FF": "f", "I8": "i8"}.get(tt, "c"), L, D)
    out = empty(cuda, torch.float32 if tt == "FF" else torch.complex64, N)
    pairs = run_gated(cuda, gate, [taps, x], [out], [lambda phase: ops.fir(taps[0], x[0], D, N, out=out)])
    if T == 0:
        assert bool((raw_bytes(pairs[0][0]) == 0).all()) and not mismatches(pairs)
    else:
        check(pairs, f"fir {tt} D={D} T={T}")


# ------------------------------------------------------------------------------------------------ chains

def chain_call(kind, x, taps, D, N, out, chans=None):
    from gsdr_amd import ops

    if chans is None:
        if kind == "fm":
            return lambda phase: ops.fm_demod(x, taps, FS, TUNE, CHAN, DEV, D, N0, N, out=out)
        if kind == "am":
            return lambda phase: ops.am_demod(x, taps, FS, TUNE, CHAN, D, N0, N, out=out)
        return lambda phase: ops.xlating_fir(x, taps, FS, TUNE, CHAN, D, N0, N, out=out)
    if kind == "fm":
        devs = [DEV * (1 + 0.1 * c) for c in range(len(chans))]
        return lambda phase: ops.fm_demod_multi(x, taps, FS, TUNE, chans, devs, D, N0, N, out=out)
    if kind == "am":
        return lambda phase: ops.am_demod_multi(x, taps, FS, TUNE, chans, D, N0, N, out=out)
    return lambda phase: ops.xlating_fir_multi(x, taps, FS, TUNE, chans, D, N0, N, out=out)


@pytest.mark.parametrize("D", [4, 9])
@pytest.mark.parametrize("int8", [False, True], ids=["cf32", "cs8"])
@pytest.mark.parametrize("kind", ["fm", "am", "xlate"])
def test_chains(cuda, gate, kind, int8, D):
    T, N = 127, 5003
    taps = drawn(cuda, "taps", T, D)
    x = drawn(cuda, "i8" if int8 else "c", N * D + T, D + int8)
    out = empty(cuda, torch.complex64 if kind == "xlate" else torch.float32, N)
    check(run_gated(cuda, gate, [taps, x], [out], [chain_call(kind, x[0], taps[0], D, N, out)]), f"{kind} D={D}")


@pytest.mark.parametrize("C,int8", [(3, False), (17, False), (3, True)], ids=["C3", "C17", "C3-cs8"])
@pytest.mark.parametrize("kind", ["fm", "am", "xlate"])
def test_multi_channel_chains(cuda, gate, kind, C, int8):
    """One launch a channel (int8), or one per 16 channels: 17 is the grouped kernel plus a remainder launch."""
    D, T, N = 4, 127, 2003
    taps = drawn(cuda, "taps", T, C)
    x = drawn(cuda, "i8" if int8 else "c", N * D + T, C + 50)
    out = empty(cuda, torch.complex64 if kind == "xlate" else torch.float32, C, N)
    check(run_gated(cuda, gate, [taps, x], [out], [chain_call(kind, x[0], taps[0], D, N, out, MCH[:C])]),
          f"{kind}_multi C={C}")


# ------------------------------------------------------------------------------------------------ resample, channelizer

@pytest.fixture(scope="module")
def resample_route(tmp_path_factory):
    run = build_resample_plan(tmp_path_factory.mktemp("resample_plan_stream_order"))
    return lambda L, M, T, dtype: run([(L, M, T, 8 if dtype.is_complex else 4, 1)])[0]


@pytest.fixture(scope="module")
def channelizer_route(tmp_path_factory):
    run = build_channelizer_plan(tmp_path_factory.mktemp("channelizer_plan_stream_order"))
    return lambda M, D, T: run([(M, D, T, 1)])[0]


def resample_job(cuda, L, M, T, N, dtype, seed):
    from gsdr_amd import ops

    q = L - 1
    taps = drawn(cuda, "taps", T, seed)
    x = drawn(cuda, "c" if dtype.is_complex else "f", max(1, inputs_for(L, M, q, T, N)) if T else 4000, seed + 1)
    out = empty(cuda, dtype, N)
    return GatedJob([taps, x], [out], [lambda phase: ops.resample(taps[0], x[0], L, M, q, N, out=out)])


@pytest.mark.parametrize("dtype", [torch.float32, torch.complex64], ids=["FF", "FC"])
@pytest.mark.parametrize("L,M,T,N,route", [(24, 125, 769, None, TILE), (3, 2, 20000, 300, GENERIC), (3, 2, 0, 1000, None)],
                         ids=["tiled", "generic", "no-taps"])
def test_resample(cuda, gate, resample_route, L, M, T, N, route, dtype):
    if route is not None:
        p = resample_route(L, M, T, dtype)
        assert p["route"] == route
        N = p["kt"] + 37 if N is None else N
    pairs = run_gated_jobs(cuda, gate, [resample_job(cuda, L, M, T, N, dtype, T)])[0]
    if T == 0:   # the hipMemsetAsync route
        assert bool((raw_bytes(pairs[0][0]) == 0).all()) and not mismatches(pairs)
    else:
        check(pairs, f"resample L={L} M={M} T={T}")


def channelizer_job(cuda, M, D, T, N, fmt, seed):
    from gsdr_amd import ops

    taps = drawn(cuda, "taps", T, seed)
    x = drawn(cuda, "i8" if fmt == "CS8" else "c", (N - 1) * D + max(T, 1), seed + 1)
    out = empty(cuda, torch.complex64, M, N)
    return GatedJob([taps, x], [out], [lambda phase: ops.channelizer(x[0], taps[0], M, D, N0, N, out=out)])


@pytest.mark.parametrize("fmt", ["CF32", "CS8"])
@pytest.mark.parametrize("M,D,T,N,route", [(16, 8, 127, None, TILE), (16, 5, 127, 1100, GENERIC), (8, 4, 0, 900, None)],
                         ids=["tiled", "generic", "no-taps"])
def test_channelizer(cuda, gate, channelizer_route, M, D, T, N, route, fmt):
    if route is not None:
        p = channelizer_route(M, D, T)
        assert p["route"] == route
        N = p["kt"] + 37 if N is None else N
    pairs = run_gated_jobs(cuda, gate, [channelizer_job(cuda, M, D, T, N, fmt, T + M)])[0]
    if T == 0:   # the hipMemsetAsync route
        assert bool((raw_bytes(pairs[0][0]) == 0).all()) and not mismatches(pairs)
    else:
        check(pairs, f"channelizer M={M} D={D} T={T} {fmt}")


# ------------------------------------------------------------------------------------------------ IIR

IIR_SIZES = {1000: 0, 128 * 64 + 1: 1, 128 * 64 * 64 + 7: 2}   # size -> scan levels


def scan_levels(n):
    """The scan plan's level count (tests/test_iir_plan.py test_levels: 32-sample chunks, groups of 64, the levels stop
    at the first one that is a single group)."""
    e, levels = -(-n // 32), 0
    while e > 64:
        e, levels = -(-e // 64), levels + 1
    return levels


def iir_design(order, seed):
    rng = np.random.default_rng(seed)
    a = np.poly(rng.uniform(-0.8, 0.8, order))
    b = rng.uniform(-0.5, 0.5, order + 1)
    return b.astype(np.float32), a.astype(np.float32)


def iir_job(cuda, order, n, cplx, seed, calls=2):
    """Two calls back to back with histories: the second consumes the xh / yh the first one writes."""
    from gsdr_amd import ops

    kind = "c" if cplx else "f"
    (b1, a1), (b2, a2) = iir_design(order, seed), iir_design(order, seed + 1000)
    b, a = slot(cuda, b1, b2), slot(cuda, a1, a2)
    x1, x2 = drawn(cuda, kind, n, seed + 1), drawn(cuda, kind, n, seed + 2)
    xh, yh = drawn(cuda, kind, order, seed + 3), drawn(cuda, kind, order, seed + 4)
    y1, y2 = empty(cuda, x1[0].dtype, n), empty(cuda, x1[0].dtype, n)
    steps = [lambda phase: ops.iir(b[0], a[0], x1[0], xh[0], yh[0], out=y1),
             lambda phase: ops.iir(b[0], a[0], x2[0], xh[0], yh[0], out=y2)]
    if calls == 1:
        return GatedJob([b, a, x1], [y1], steps[:1], inouts=[xh, yh])
    return GatedJob([b, a, x1, x2], [y1, y2], steps, inouts=[xh, yh])


@pytest.mark.parametrize("n", list(IIR_SIZES))
@pytest.mark.parametrize("order", [2, 9, 20])
@pytest.mark.parametrize("cplx", [False, True], ids=["FF", "CC"])
def test_iir_two_calls_with_histories(cuda, gate, cplx, order, n):
    """Five to eight launches a call, a workspace from the async pool on the caller's stream, and xh copied inside
    the first kernel before the last one overwrites it; scan levels 0, 1 and 2.

    Every launch of both calls is enqueued behind the closed gate, but the host does not get ahead of the gate
    here: the runtime's second hipFreeAsync on a stream that is still busy waits on the host until that stream has
    drained (measured with bare hipMallocAsync / hipFreeAsync pairs behind a 30 ms gate: the first pair returns
    within 0.1 ms, the second pair's free after 30.1 ms, whatever the pool's release threshold), so the second
    call returns when the gate ends and only the snapshots are enqueued after it. iir.h's "the call stays
    asynchronous" holds for the first call on an idle pool only."""
    assert scan_levels(n) == IIR_SIZES[n]
    pairs = run_gated_jobs(cuda, gate, [iir_job(cuda, order, n, cplx, order + n % 1000)])[0]
    check(pairs, f"iir order={order} n={n}")
    assert len(pairs) == 4   # y1, y2, xh, yh


# ------------------------------------------------------------------------------------------------ Stream objects

CHUNKS = [3001, 50, 2777]   # ragged; 50 is shorter than the window, so the next history is old history plus chunk


def stream_job(cuda, kind, int8, D, chans=None, seed=0):
    """Three chunks through Stream.process() back to back: one Stream object a phase (the state lives on the host),
    created here, before any gate (hipMalloc synchronises). Returns (job, close)."""
    from gsdr_amd.stream import Stream

    T = 127
    taps = drawn(cuda, "taps", T, seed + D)
    per = 2 if int8 else 1
    xs = [drawn(cuda, "i8" if int8 else "c", m, seed + 10 * k + D) for k, m in enumerate(CHUNKS)]
    assert min(CHUNKS) < T
    odt = torch.complex64 if kind in ("fir", "xlate") else torch.float32
    shape = (lambda m: (m // D + 2,)) if chans is None else (lambda m: (len(chans), m // D + 2))
    outs = [empty(cuda, odt, *shape(m)) for m in CHUNKS]
    freq = CHAN if chans is None else list(chans)
    devs = DEV if chans is None else [DEV * (1 + 0.1 * c) for c in range(len(chans))]
    objs = {phase: Stream(kind, taps[0], D, FS, TUNE, freq, devs, first_sample_index=N0, int8=int8)
            for phase in ("reference", "gated")}
    written = {"reference": [], "gated": []}

    def step(k):
        def run(phase):
            assert xs[k][0].numel() == CHUNKS[k] * per
            written[phase].append(objs[phase].process(xs[k][0], out=outs[k]).shape[-1])
        return run

    def close(passed=True):
        torch.cuda.synchronize(cuda)
        for s in objs.values():
            s.close()
        if passed:   # every chunk, the short one included, produced outputs, the same count in both runs
            assert written["reference"] == written["gated"] and min(written["gated"]) > 0, written

    return GatedJob([taps] + xs, outs, [step(k) for k in range(len(CHUNKS))]), close


def run_stream_jobs(cuda, gate, made):
    """run_gated_jobs over stream_job() results; the Stream objects are closed after the final sync, pass or fail."""
    try:
        pairs = run_gated_jobs(cuda, gate, [job for job, _ in made])
    except BaseException:
        for _, close in made:
            close(passed=False)
        raise
    for _, close in made:
        close()
    return pairs


@pytest.mark.parametrize("D", [4, 9], ids=["one-launch", "seam-plan"])
@pytest.mark.parametrize("int8", [False, True], ids=["cf32", "cs8"])
@pytest.mark.parametrize("kind", ["fir", "fm", "am", "xlate"])
def test_stream_object(cuda, gate, kind, int8, D):
    """gsdrxStreamProcess swaps its history buffers on the host while the launch that fills the spare one is still
    queued: three calls behind one gate."""
    check(run_stream_jobs(cuda, gate, [stream_job(cuda, kind, int8, D)])[0], f"stream {kind} D={D}")


@pytest.mark.parametrize("kind,D", [("fm", 4), ("xlate", 4), ("am", 9)])
def test_multi_channel_stream_object(cuda, gate, kind, D):
    made = [stream_job(cuda, kind, False, D, chans=MCH[:3], seed=5)]
    check(run_stream_jobs(cuda, gate, made)[0], f"multi-channel stream {kind} D={D}")


# ------------------------------------------------------------------------------------------------ element-wise, quadrature

N_EL = 10_007


def elementwise_cases():
    from gsdr_amd import ops

    f32, c64 = torch.float32, torch.complex64
    # name -> (input kinds, output dtype, call(inputs..., out))
    return {
        "add_const_ff": (["f"], f32, lambda x, out: ops.add_const(x, 3.14, out=out)),
        "add_const_cc": (["c"], c64, lambda x, out: ops.add_const(x, 1.5 - 2.5j, out=out)),
        "add_const_cf": (["c"], c64, lambda x, out: ops.add_const(x, -1.23, out=out)),
        "add_const_fc": (["f"], c64, lambda x, out: ops.add_const(x, 2.5 - 1.5j, out=out)),
        "multiply_cc": (["c", "c"], c64, lambda a, b, out: ops.multiply(a, b, out=out)),
        "multiply_ff": (["f", "f"], f32, lambda a, b, out: ops.multiply(a, b, out=out)),
        "multiply_cf": (["c", "f"], c64, lambda a, b, out: ops.multiply(a, b, out=out)),
        "add_to_magnitude": (["c"], c64, lambda x, out: ops.add_to_magnitude(x, 2.5, out=out)),
        "abs": (["f"], f32, lambda x, out: ops.abs_(x, out=out)),
        "magnitude": (["c"], f32, lambda x, out: ops.magnitude(x, out=out)),
        "int8_to_norm_float": (["i8"], f32, lambda x, out: ops.int8_to_norm_float(x[:N_EL], out=out)),
        "quad_fm_demod": (["c"], f32, lambda x, out: ops.quad_fm_demod(x, 0.75, N_EL - 1, out=out[:N_EL - 1])),
        "quad_am_demod": (["c"], f32, lambda x, out: ops.quad_am_demod(x, N_EL, out=out)),
    }


@pytest.mark.parametrize("name", ["add_const_ff", "add_const_cc", "add_const_cf", "add_const_fc", "multiply_cc",
                                  "multiply_ff", "multiply_cf", "add_to_magnitude", "abs", "magnitude",
                                  "int8_to_norm_float", "quad_fm_demod", "quad_am_demod"])
def test_elementwise_and_quadrature(cuda, gate, name):
    kinds, odt, call = elementwise_cases()[name]
    ins = [drawn(cuda, k, N_EL, 11 + i) for i, k in enumerate(kinds)]
    out = empty(cuda, odt, N_EL)
    check(run_gated(cuda, gate, ins, [out], [lambda phase: call(*[s[0] for s in ins], out)]), name)


@pytest.mark.parametrize("cplx", [True, False], ids=["C", "F"])
def test_cosine(cuda, gate, cplx):
    """No input to gate: the phase ramp is written over the sentinel in stream order, ahead of the snapshot."""
    from gsdr_amd import ops

    out = empty(cuda, torch.complex64 if cplx else torch.float32, N_EL)
    check(run_gated(cuda, gate, [], [out], [lambda phase: ops.cosine(-1.3, 40.0, N_EL, cplx, out=out)]), "cosine")


# ------------------------------------------------------------------------------------------------ QPSK, QPSK256

def test_qpsk(cuda, gate):
    """gsdrQpskModulate into gsdrQpskDemodulate, back to back (the demodulator keeps the high pairs of the last,
    partial byte: the sentinel's, in both runs)."""
    from gsdr_amd import ops

    n = N_EL
    bits = drawn(cuda, "u8", (n + 3) // 4, 21)
    sym, back = empty(cuda, torch.complex64, n), empty(cuda, torch.uint8, (n + 3) // 4)
    steps = [lambda phase: ops.qpsk_modulate(bits[0], n, 0.8, out=sym), lambda phase: ops.qpsk_demodulate(sym, n, out=back)]
    check(run_gated(cuda, gate, [bits], [sym, back], steps), "qpsk")


def test_qpsk_4x_and_templated(cuda, gate):
    from gsdr_amd import ops

    n, S = 4099, 2
    stride = n // 4 + 1
    bits4 = [drawn(cuda, "u8", (n + 3) // 4, 30 + i) for i in range(4)]
    syms4 = [empty(cuda, torch.complex64, n) for _ in range(4)]
    back4 = [empty(cuda, torch.uint8, (n + 3) // 4) for _ in range(4)]
    bits_t = drawn(cuda, "u8", S * stride, 40)
    syms_t, back_t = empty(cuda, torch.complex64, S * n), empty(cuda, torch.uint8, S * stride)
    steps = [lambda phase: ops.qpsk_modulate_4x([b[0] for b in bits4], syms4, n, 1.5),
             lambda phase: ops.qpsk_demodulate_4x(syms4, back4, n),
             lambda phase: ops.qpsk_modulate_templated(bits_t[0], syms_t, n, 1.0, S),
             lambda phase: ops.qpsk_demodulate_templated(syms_t, back_t, n, S)]
    check(run_gated(cuda, gate, bits4 + [bits_t], syms4 + back4 + [syms_t, back_t], steps), "qpsk 4x / templated")


def qpsk256_job(cuda, ctype, seed, n=N_EL):
    """modulate, demodulate of it, modulate_awgn, and the fused round trip (one kernel for table 0, the two calls for
    table 1) of one symbol buffer."""
    from gsdr_amd import ops

    syms = drawn(cuda, "u8", n, seed)
    clean, noisy, fused = (empty(cuda, torch.complex64, n) for _ in range(3))
    back, dec = empty(cuda, torch.uint8, n), empty(cuda, torch.uint8, n)
    sigma = 0.05 if ctype == 0 else 0.02
    steps = [lambda phase: ops.qpsk256_modulate(syms[0], ctype, out=clean),
             lambda phase: ops.qpsk256_demodulate(clean, ctype, out=back),
             lambda phase: ops.qpsk256_modulate_awgn(syms[0], ctype, sigma, 0x5EED + seed, 7 + seed, out=noisy),
             lambda phase: ops.qpsk256_modulate_awgn_demodulate(syms[0], ctype, sigma, 0xFEED + seed, 11 + seed,
                                                                noisy=fused, out=dec)]
    return GatedJob([syms], [clean, back, noisy, fused, dec], steps)


@pytest.mark.parametrize("ctype", [0, 1], ids=["rect", "circ"])
def test_qpsk256(cuda, gate, tables, ctype):
    job = qpsk256_job(cuda, ctype, 50 + ctype)
    pairs = run_gated_jobs(cuda, gate, [job])[0]
    check(pairs, f"qpsk256 table {ctype}")
    assert torch.equal(pairs[1][1], job.inputs[0][1])   # the clean round trip returns the true symbols


def test_qpsk256_4x(cuda, gate, tables):
    from gsdr_amd import ops

    n = 5003
    ins = [drawn(cuda, "u8", n, 60 + i) for i in range(4)]
    outs = [empty(cuda, torch.complex64, n) for _ in range(4)]
    back = [empty(cuda, torch.uint8, n) for _ in range(4)]
    steps = [lambda phase: ops.qpsk256_modulate_4x([s[0] for s in ins], outs, n, 0),
             lambda phase: ops.qpsk256_demodulate_4x(outs, back, n, 0)]
    pairs = run_gated(cuda, gate, ins, outs + back, steps)
    check(pairs, "qpsk256 4x")
    assert all(torch.equal(pairs[4 + i][1], ins[i][1]) for i in range(4))


@pytest.mark.parametrize("ctype", [0, 1], ids=["rect", "circ"])
def test_qpsk256_init_then_modulate_on_a_side_stream(cuda, ctype):
    """Ungated: gsdrQpsk256InitConstellation(type, amp2) on a side stream, at once followed by gsdrQpsk256Modulate on
    the same stream, modulates with amp2's table (the reference's init raced the legacy stream)."""
    from gsdr_amd import ops
    from oracle import oracle as o

    syms = torch.arange(256, dtype=torch.uint8, device=cuda)
    out = empty(cuda, torch.complex64, 256)
    try:
        ops.qpsk256_init(ctype, 1.0)
        torch.cuda.synchronize(cuda)
        side = torch.cuda.Stream(device=cuda)
        with torch.cuda.stream(side):
            ops.qpsk256_init(ctype, 2.5)
            ops.qpsk256_modulate(syms, ctype, out=out)
        side.synchronize()
        assert np.array_equal(out.cpu().numpy(), o.qpsk256_table(ctype, 2.5))
    finally:
        ops.qpsk256_init(ctype, 1.0)   # what the `tables` fixture set
        torch.cuda.synchronize(cuda)


# ------------------------------------------------------------------------------------------------ two streams at once

def check_jobs(all_pairs, what):
    for k, pairs in enumerate(all_pairs):
        check(pairs, f"{what}: stream {'AB'[k]}")


def test_two_streams_iir(cuda, gate):
    """IIR FF order 4 beside IIR CC order 9 at three scan levels' size, with histories: both hold a workspace from
    the async pool at once. One call a stream: a second call's hipFreeAsync waits on the host for its stream's gate
    (test_iir_two_calls_with_histories), after which the other stream's second call is no longer enqueued behind a
    closed gate -- with two calls a stream this case ends as inconclusive at every gate length (20 ms and 100 ms
    tried: the host left the second call on stream A 14.6 ms and 198 ms after entering it)."""
    n = 128 * 64 * 64 + 7
    jobs = [iir_job(cuda, 4, n, False, 71, calls=1), iir_job(cuda, 9, n, True, 72, calls=1)]
    check_jobs(run_gated_jobs(cuda, gate, jobs), "iir")


def test_two_streams_stream_objects(cuda, gate):
    made = [stream_job(cuda, "fm", False, 4, seed=80), stream_job(cuda, "xlate", False, 4, seed=90)]
    check_jobs(run_stream_jobs(cuda, gate, made), "fm / xlate Stream")


def test_two_streams_channelizer_and_resample(cuda, gate, channelizer_route, resample_route):
    kt_c = channelizer_route(16, 8, 127)["kt"]
    kt_r = resample_route(24, 125, 769, torch.complex64)["kt"]
    jobs = [channelizer_job(cuda, 16, 8, 127, kt_c + 37, "CF32", 100),
            resample_job(cuda, 24, 125, 769, kt_r + 37, torch.complex64, 110)]
    check_jobs(run_gated_jobs(cuda, gate, jobs), "channelizer / resample")


def test_two_streams_fused_qpsk256_on_one_table(cuda, gate, tables):
    """Two fused round trips on the same (rectangular) table, different seeds and inputs."""
    check_jobs(run_gated_jobs(cuda, gate, [qpsk256_job(cuda, 0, 120), qpsk256_job(cuda, 0, 130)]), "qpsk256")
