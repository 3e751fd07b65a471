"""Shared parity metrics for the tests."""
from __future__ import annotations

import numpy as np

# north_star: float paths within 1e-5 relative, evaluated normwise (pointwise relative error is not
# attainable by any reordered fp32 sum: two correct orders differ by up to 2.9e-5 pointwise).
FLOAT_TOL = 1e-5


# Guarded output buffers: a kernel's output is a view in the middle of a sentinel-filled buffer, so a store outside
# [output, output + n) lands in the test's own memory and is seen (an exactly sized torch allocation hides a spill of a
# few elements in the allocator's block rounding).
GUARD = 64


def default_sentinel(dtype):
    """A finite value no kernel here produces (every output is O(1), or an angle below a few hundred)."""
    return complex(-7.5, 1234.5) if dtype.is_complex else -4321.5


def guarded(cuda, dtype, n, off=0, sentinel=None):
    """(buf, view): buf holds GUARD + n + GUARD + 4 elements of `sentinel`, view = buf[GUARD + off:][:n]. buf is 16-byte
    aligned, so `off` (0 .. 3 elements) alone decides the alignment of the view."""
    import torch

    assert 0 <= off <= 4
    sentinel = default_sentinel(dtype) if sentinel is None else sentinel
    buf = torch.full((GUARD + n + GUARD + 4,), sentinel, dtype=dtype, device=cuda)
    assert buf.data_ptr() % 16 == 0
    return buf, buf[GUARD + off:GUARD + off + n]


def check_guards(buf, view, sentinel=None, what=""):
    """Every element of buf outside view still holds the sentinel, compared bytewise (a NaN or a -0.0 written over a
    guard is seen too). view: any contiguous view of buf (a (C, N) view of C * N elements included); `what` names the
    case in the failure message."""
    import torch

    sentinel = default_sentinel(buf.dtype) if sentinel is None else sentinel
    size = buf.element_size()
    lo = view.storage_offset() - buf.storage_offset()
    hi = lo + view.numel()
    assert view.is_contiguous() and 0 <= lo <= hi <= buf.numel()
    torch.cuda.synchronize()
    raw = buf.cpu().numpy()
    want = np.full(1, sentinel, dtype=raw.dtype).view(np.uint8)
    for name, part, at in (("before", raw[:lo], 0), ("after", raw[hi:], hi)):
        bad = np.flatnonzero(np.any(part.view(np.uint8).reshape(-1, size) != want, axis=1))
        assert bad.size == 0, (f"{what}: wrote outside [output, output + {view.numel()}): {bad.size} guard elements {name} it, "
                               f"buffer indices {(bad[:8] + at).tolist()} (output at {lo}), values {part[bad[:4]]}")


# Gated streams (test_gpu_stream_order.py): the library's work is enqueued on a non-blocking side stream behind a
# sleeping kernel (the gate) and behind the copies that bring the true inputs in, while the device is otherwise
# idle. Whatever the library issues on another stream (a kernel, a memset, a history copy) or assumes finished on
# the host then runs before the copy-in, on the decoy inputs, and its result differs from the synchronised
# reference. The outputs are refilled with the sentinel behind the gate as well, so a write that ran early is lost
# even where it does not depend on the inputs (a memset). The gate ends by itself: nothing ever waits for the host.
def raw_bytes(t):
    """t's storage bytes as a flat uint8 tensor (a bitwise comparison: NaNs and signed zeros count)."""
    import torch

    t = torch.view_as_real(t) if t.is_complex() else t
    return t.contiguous().view(-1).view(torch.uint8)


def stream_sentinel(dtype):
    import torch

    return 0xA5 if dtype == torch.uint8 else default_sentinel(dtype)


class GatedJob:
    """One side stream's work for run_gated_jobs().

    inputs:  (live, true, decoy) device tensors of one shape: `live` is what the entry point reads.
    outputs: pre-allocated device tensors the entry point writes (the same addresses in both runs).
    inouts:  (live, true, decoy) like inputs, for buffers a call also writes (IIR histories): snapshotted too.
    steps:   callables step(phase), phase "reference" or "gated", each enqueueing library calls on torch's current
             stream; host-side state (a Stream object) is the step's own business, one object a phase.
    on_default_stream: the control: the gated run issues the steps on the idle default stream instead of the side
             stream (the copy-in stays gated), which a working harness must see as a mismatch."""

    def __init__(self, inputs, outputs, steps, inouts=(), on_default_stream=False):
        self.inputs, self.outputs, self.inouts = list(inputs), list(outputs), list(inouts)
        self.steps = list(steps)
        self.on_default_stream = on_default_stream
        for live, true, decoy in self.inputs + self.inouts:
            assert live.shape == true.shape == decoy.shape and live.dtype == true.dtype == decoy.dtype
        self.watched = self.outputs + [live for live, _, _ in self.inouts]


_SIDE_STREAMS = []   # streams that passed side_streams()'s check before: tried first, and checked again


def side_streams(cuda, count, gate_cycles):
    """`count` of torch's non-blocking streams that the device runs independently of the default stream and of each
    other, checked now: with a short sleep (a tenth of the gate) queued on the one, a one-element kernel on the other
    finishes while the first still sleeps. The runtime places its streams on a few hardware queues, and two streams on
    one queue run in order whatever the program says: behind such a side stream a kernel that the library wrongly
    issued on the default stream would wait for the gate like everything else, and the fault would go unseen."""
    import torch

    probe = torch.zeros(1, device=cuda)
    nap = max(1, gate_cycles // 10)

    def independent(sleeper, other):
        torch.cuda.synchronize(cuda)
        asleep, ran = torch.cuda.Event(), torch.cuda.Event()
        with torch.cuda.stream(sleeper):
            torch.cuda._sleep(nap)
            asleep.record(sleeper)
        with torch.cuda.stream(other):
            probe.zero_()
            ran.record(other)
        ran.synchronize()
        return not asleep.query()

    default = torch.cuda.default_stream(cuda)
    chosen = []
    candidates = list(_SIDE_STREAMS)
    for _ in range(64):
        if len(chosen) == count:
            break
        s = candidates.pop(0) if candidates else torch.cuda.Stream(device=cuda)
        if any(s.cuda_stream == c.cuda_stream for c in chosen):
            continue
        if all(independent(s, o) and independent(o, s) for o in [default] + chosen):
            chosen.append(s)
    torch.cuda.synchronize(cuda)
    assert len(chosen) == count, f"found {len(chosen)} of {count} streams that run independently of the default stream"
    for s in chosen:
        if not any(s.cuda_stream == c.cuda_stream for c in _SIDE_STREAMS):
            _SIDE_STREAMS.append(s)
    return chosen


def run_gated_jobs(cuda, gate_cycles, jobs):
    """Reference (synchronised, default stream), arm (decoys in, sentinels out), then every job behind its own gate on
    its own non-blocking side stream (side_streams()), the jobs' steps enqueued alternately. Asserts that every gate was still closed when
    the host had finished enqueueing (else the run is inconclusive and fails). Returns, per job, a list of
    (reference clone, gated snapshot) pairs, one per output and in/out buffer."""
    import contextlib

    import torch

    def fill(job, decoy):
        for live, true, dec in job.inputs + job.inouts:
            live.copy_(dec if decoy else true)
        for out in job.outputs:
            out.fill_(stream_sentinel(out.dtype))

    # 1. reference: device idle, default stream, one job after the other
    refs = []
    for job in jobs:
        torch.cuda.synchronize(cuda)
        fill(job, decoy=False)
        torch.cuda.synchronize(cuda)
        for step in job.steps:
            step("reference")
        torch.cuda.synchronize(cuda)
        refs.append([t.clone() for t in job.watched])
    # 2. arm; the snapshots are allocated here (an allocation behind the gate could wait for the device)
    snaps = []
    for job in jobs:
        fill(job, decoy=True)
        snaps.append([torch.full_like(t, stream_sentinel(t.dtype)) for t in job.watched])
    sides = side_streams(cuda, len(jobs), gate_cycles)
    dones = [torch.cuda.Event() for _ in jobs]
    torch.cuda.synchronize(cuda)
    # 3. gated run
    for job, side in zip(jobs, sides):
        with torch.cuda.stream(side):
            torch.cuda._sleep(gate_cycles)
            for live, true, _ in job.inputs + job.inouts:
                live.copy_(true, non_blocking=True)
            for out in job.outputs:   # whatever was written before this point (a memset on another stream) is lost
                out.fill_(stream_sentinel(out.dtype))
    for k in range(max(len(job.steps) for job in jobs)):
        for job, side in zip(jobs, sides):
            if k < len(job.steps):
                with contextlib.nullcontext() if job.on_default_stream else torch.cuda.stream(side):
                    job.steps[k]("gated")
    for job, side, snap, done in zip(jobs, sides, snaps, dones):
        with torch.cuda.stream(side):
            for s, t in zip(snap, job.watched):
                s.copy_(t, non_blocking=True)
            done.record(side)
    # 4. the gates were closed while all of that was enqueued
    closed = [not done.query() for done in dones]
    # 5. compare
    for side in sides:
        side.synchronize()
    torch.cuda.synchronize(cuda)
    assert all(closed), f"inconclusive: a gate of {gate_cycles} cycles ended before the host had enqueued the work"
    return [list(zip(r, s)) for r, s in zip(refs, snaps)]


def run_gated(cuda, gate_cycles, inputs, outputs, steps, inouts=(), on_default_stream=False):
    """run_gated_jobs() for one stream: the list of (reference, snapshot) pairs."""
    return run_gated_jobs(cuda, gate_cycles, [GatedJob(inputs, outputs, steps, inouts, on_default_stream)])[0]


def mismatches(pairs):
    """Indices of the (reference, snapshot) pairs that differ in any bit."""
    import torch

    return [k for k, (r, s) in enumerate(pairs) if not torch.equal(raw_bytes(r), raw_bytes(s))]


def bound(taps, x, D, N, k0=0, k1=None):
    """S_k = sum_i |t_i| |x_{kD+i}| in float64, for k in [k0, k1)."""
    k1 = N if k1 is None else k1
    T = taps.size
    at = np.abs(taps.astype(np.complex128))
    ax = np.abs(x.astype(np.complex128))
    # valid correlation then decimation, only over the needed span
    lo, hi = k0 * D, (k1 - 1) * D + T
    c = np.correlate(ax[lo:hi], at, mode="valid")
    return c[::D][: k1 - k0]


def normwise_err(got, want, s):
    """max_k |got_k - want_k| / S_k (S_k floored to avoid 0/0 on all-zero windows)."""
    got = np.asarray(got).astype(np.complex128)
    want = np.asarray(want).astype(np.complex128)
    s = np.maximum(np.asarray(s, dtype=np.float64), 1e-30)
    return float(np.max(np.abs(got - want) / s)) if got.size else 0.0


def wrapped_angle_err(got, want, g):
    """max |remainder(got - want, 2 pi g)| / (pi g): discriminator outputs are angles scaled by g."""
    d = np.remainder(np.asarray(got, np.float64) - np.asarray(want, np.float64) + np.pi * g, 2 * np.pi * g) - np.pi * g
    return float(np.max(np.abs(d)) / (np.pi * abs(g))) if d.size else 0.0


def normwise_err_strict(got, want, s):
    """max_k |got_k - want_k| / S_k with no floor: an output whose window contributes nothing (S_k = 0)
    must match exactly (returns inf otherwise). For tap sets near the bottom of the float range and for
    sparse inputs, where S_k itself is tiny or zero."""
    got = np.asarray(got).astype(np.complex128)
    want = np.asarray(want).astype(np.complex128)
    s = np.asarray(s, dtype=np.float64)
    d = np.abs(got - want)
    if np.any(d[s == 0] != 0):
        return float("inf")
    pos = s > 0
    return float(np.max(d[pos] / s[pos])) if np.any(pos) else 0.0


def fm_conditioned_err(got, want, y_ref, s, g, eps=2e-6):
    """FM discriminator error relative to its conditioning: the wrapped angle error of output k divided by
    the angle the fp32 evaluation itself cannot resolve, with y the oracle's FIR outputs (N + 1) and S their
    normwise bounds:
      * a pair with a zero window (S_k = 0 or S_{k+1} = 0): the discriminator product is exactly zero and
        the reference's atan2f(+-0, +-0) value (0 or +-pi, from the signs) must come out: bar 1e-5 pi;
      * otherwise max(1e-5 pi, eps (S_k/|y_k| + S_{k+1}/|y_{k+1}|) + 8 * 2^-149 / (|y_k| |y_{k+1}|)) rad: a
        window that cancels to a small |y| makes any fp32 summation order's angle uncertain by ~eps S/|y|,
        and a product y_{k+1} conj(y_k) below fp32's normal range keeps only its subnormal absolute
        precision (2^-149 a component) in the reference as here.
    Returns the max ratio (<= 1 passes)."""
    got = np.asarray(got, np.float64)
    want = np.asarray(want, np.float64)
    d = np.abs(np.remainder(got - want + np.pi * g, 2 * np.pi * g) - np.pi * g) / abs(g)
    ay = np.abs(np.asarray(y_ref).astype(np.complex128))
    s = np.asarray(s, np.float64)
    zero_pair = (s[:-1] == 0) | (s[1:] == 0)
    prod = ay[:-1] * ay[1:]
    with np.errstate(divide="ignore", invalid="ignore"):
        kappa = s / ay  # S > 0 with |y| = 0: unbounded
        allowed = eps * (kappa[:-1] + kappa[1:]) + 8.0 * 2.0 ** -149 / prod
    allowed = np.where(zero_pair, 1e-5 * np.pi, np.maximum(1e-5 * np.pi, np.nan_to_num(allowed, nan=np.inf)))
    return float(np.max(d / allowed)) if d.size else 0.0


# Reference-run vectors (tests/golden/ref_*.npz, written by tests/golden/make_reference_vectors.py): what the
# reference's own kernel text computes on the stored inputs, built with and without contraction of a * b + c.
REF_BUILDS = ("contract", "nocontract")


def ref_vectors(stem):
    import os

    return np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", stem + ".npz"), allow_pickle=False)


def ref_pick(g, name, build):
    """Output `name` of `build`: stored once, under `name`, where the two builds agree bit for bit."""
    return g[name] if name in g.files else g[f"{name}__{build}"]


def same_values(got, want):
    """Bit identity of two float / complex / integer arrays, with every NaN equal to every NaN: IEEE 754 leaves the
    sign and payload of a NaN that an operation produces open (x86 and the GPU differ, and so do two operand orders
    on x86), everything else, the sign of a zero included, is compared bitwise. Returns the number of differing
    elements (0 passes), or -1 for a dtype or shape mismatch."""
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    if got.dtype != want.dtype or got.shape != want.shape:
        return -1
    if got.dtype.kind not in "fc":
        return int(np.count_nonzero(got != want))
    g, w = got.view(np.float32), want.view(np.float32)
    gn, wn = np.isnan(g), np.isnan(w)
    return int(np.count_nonzero((gn != wn) | (~wn & (g.view(np.uint32) != w.view(np.uint32)))))


def same_specials(got, want):
    """The NaN pattern, the Inf pattern and the signs of the infinities agree, component by component."""
    g = np.ascontiguousarray(got).view(np.float32)
    w = np.ascontiguousarray(want).view(np.float32)
    inf = np.isinf(w)
    return bool(np.array_equal(np.isnan(g), np.isnan(w)) and np.array_equal(np.isinf(g), inf)
                and np.array_equal(g[inf], w[inf]))


def finite_elements(a):
    a = np.asarray(a)
    return np.isfinite(a.real) & np.isfinite(a.imag) if np.iscomplexobj(a) else np.isfinite(a)
