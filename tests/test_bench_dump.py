"""bench.py's plain run and its --dump-outputs / --full options.

CPU: the dumped sample is fixed (same indices every time: edges + a seeded draw) and dump_outputs writes
exactly the tensor's values at those indices as float32. GPU: one plain run end to end -- the line carries
the headline fields and none of the legs that belong to --full, and the dump is, bit for bit, gsdrFirFC of
the batch the last timed step filtered."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_dump_indices_are_fixed():
    import bench

    idx = bench.dump_indices(bench.N_OUT)
    assert idx.dtype == np.int64 and np.array_equal(idx, bench.dump_indices(bench.N_OUT))
    assert np.all(np.diff(idx) > 0) and idx[0] == 0 and idx[-1] == bench.N_OUT - 1
    e = bench.DUMP_EDGE
    assert np.array_equal(idx[:e], np.arange(e)) and np.array_equal(idx[-e:], np.arange(bench.N_OUT - e, bench.N_OUT))
    assert bench.DUMP_SAMPLE // 2 < idx.size <= bench.DUMP_SAMPLE + 2 * e
    assert 2 * idx.size * (4 + 4) <= 64 << 20  # both files together, far below the 64 MB a dump may take
    small = bench.dump_indices(1000)  # fewer outputs than the sample: every output, once
    assert np.array_equal(small, np.arange(1000))


def test_dump_outputs_writes_the_values(tmp_path):
    import bench

    n = 3 * bench.DUMP_EDGE
    y = torch.view_as_complex(torch.arange(2 * n, dtype=torch.float32).reshape(n, 2) / 7)
    bench.dump_outputs(torch, str(tmp_path / "d"), "y", y)
    vals, idx = np.load(tmp_path / "d" / "y.npy"), np.load(tmp_path / "d" / "y_index.npy")
    assert vals.dtype == np.float32 and idx.dtype == np.float64
    assert np.array_equal(idx, bench.dump_indices(n).astype(np.float64))
    assert vals.tobytes() == torch.view_as_real(y).numpy()[idx.astype(np.int64)].tobytes()


@pytest.mark.gpu
def test_plain_run_line_and_dump(cuda, tmp_path):
    import bench
    from gsdr_amd import ops
    from gsdr_amd.signals import lowpass_taps

    steps = 4  # the last timed step filters batch (4 - 1) % 3 = 0: the first draw of the channel's generator
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", str(steps), "--warmup",
                        "2", "--settle-max", "0", "--dump-outputs", str(tmp_path)], cwd=ROOT, capture_output=True,
                       text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout
    line = json.loads(lines[0])
    assert line["steps"] == steps and line["full"] is False and line["n_gpus"] == 1
    assert line["metric"] == bench.METRIC and line["unit"] == "Msamples/s" and line["higher_is_better"] is True
    assert line["dtype"] == "f32" and line["ms_per_step"] > 0
    assert line["value"] == pytest.approx(bench.N_IN / (line["ms_per_step"] * 1e-3) / 1e6, rel=1e-2)
    # what takes runs of its own belongs to --full
    assert "secondary" not in line and "cpu_baseline" not in line
    assert not {"one_output_buffer", "staging_ceiling", "measured_copy_gbps"} & set(line["roofline"])
    assert sorted(os.listdir(tmp_path)) == ["fir_fc_out.npy", "fir_fc_out_index.npy"]
    vals, idx = np.load(tmp_path / "fir_fc_out.npy"), np.load(tmp_path / "fir_fc_out_index.npy")
    assert vals.dtype == np.float32 and np.array_equal(idx.astype(np.int64), bench.dump_indices(bench.N_OUT))
    taps = torch.from_numpy(lowpass_taps(bench.TAPS, 0.1)).to(cuda)
    g = torch.Generator(device=cuda).manual_seed(bench.channel_seed(0))
    x = (torch.rand(2 * bench.N_IN, device=cuda, generator=g) * 2 - 1).view(torch.complex64)
    y = ops.fir(taps, x, bench.DECIM, bench.N_OUT)
    want = torch.view_as_real(y[torch.from_numpy(idx.astype(np.int64)).to(cuda)]).cpu().numpy()
    assert vals.tobytes() == want.tobytes()
