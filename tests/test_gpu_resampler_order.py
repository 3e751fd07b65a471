"""GPU: gsdrxResamplerProcess on a busy non-blocking side stream (helpers.run_gated, the method of
test_gpu_stream_order.py): three calls on one object are enqueued behind a sleeping kernel and behind the copies that
bring the true inputs in. The object swaps its history buffers on the host while the launch that fills the spare one
is still queued, so a history copy, a seam gather or a memset issued on another stream, or anything assumed finished
on the host, would run on the decoy inputs and differ from the synchronised run.
"""
import numpy as np
import pytest
import torch

from helpers import mismatches, raw_bytes, run_gated, stream_sentinel
from resample_ref import build_plan_program

pytestmark = pytest.mark.gpu

GATE_MS = 20.0            # target length of the gate
PROBE_CYCLES = 2_000_000  # the calibration sleep
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
    return int(PROBE_CYCLES / ms * GATE_MS)


def slot(cuda, kind, n, seed):
    """(live, true, decoy) device tensors: "f" / "c" samples in [-1, 1), "taps" of both signs and none zero."""
    def draw(s):
        rng = np.random.default_rng(s)
        if kind == "taps":
            return (rng.uniform(0.1, 1.0, n) * rng.choice([-1.0, 1.0], n) / np.sqrt(n)).astype(np.float32)
        x = rng.uniform(-1, 1, n).astype(np.float32)
        return x if kind == "f" else (x + 1j * rng.uniform(-1, 1, n)).astype(np.complex64)

    t, d = torch.from_numpy(draw(seed)).to(cuda), torch.from_numpy(draw(seed + 1000)).to(cuda)
    assert not torch.equal(raw_bytes(t), raw_bytes(d))
    return torch.empty_like(t), t, d


# (L, M, T, chunks): the middle chunk is shorter than the kept history, so the next history is old history plus chunk
CASES = [(24, 125, 769, [3001, 20, 2777], TILE), (3, 2, 20000, [9001, 50, 2777], GENERIC), (1, 4, 127, [3001, 50, 2777], None)]


@pytest.mark.parametrize("cplx", [False, True], ids=["FF", "FC"])
@pytest.mark.parametrize("L,M,T,chunks,route", CASES, ids=["tile", "generic", "fir"])
def test_resampler_object(cuda, gate, tmp_path, L, M, T, chunks, route, cplx):
    from gsdr_amd.stream import Resampler

    if route is not None:
        assert build_plan_program(tmp_path)([(L, M, T, 8 if cplx else 4, 1)])[0]["route"] == route
    assert min(chunks) < -(-T // L) - 1
    taps = slot(cuda, "taps", T, L + M)
    xs = [slot(cuda, "c" if cplx else "f", c, 10 * k + T) for k, c in enumerate(chunks)]
    dtype = torch.complex64 if cplx else torch.float32
    outs = [torch.empty(c * L // M + 2, dtype=dtype, device=cuda) for c in chunks]
    # one object a phase (the state lives on the host), created before any gate (hipMalloc synchronises)
    objs = {phase: Resampler(taps[0], L, M, L - 1, complex_samples=cplx) for phase in ("reference", "gated")}
    written = {"reference": [], "gated": []}

    def step(k):
        def run(phase):
            written[phase].append(objs[phase].process(xs[k][0], out=outs[k]).numel())
        return run

    try:
        pairs = run_gated(cuda, gate, [taps] + xs, outs, [step(k) for k in range(len(chunks))])
    finally:
        torch.cuda.synchronize(cuda)
        for r in objs.values():
            r.close()
    what = f"resampler L={L} M={M} T={T} {dtype}"
    bad = mismatches(pairs)
    assert not bad, f"{what}: gated buffers {bad} of {len(pairs)} differ from the synchronised run"
    # every call, the short one included, wrote outputs, the same count in both runs
    assert written["reference"] == written["gated"] and min(written["gated"]) > 0, written
    for ref, _ in pairs:
        assert not bool((raw_bytes(ref) == raw_bytes(torch.full_like(ref, stream_sentinel(ref.dtype)))).all()), what
