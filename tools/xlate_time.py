"""Call time of gsdrxXlatingFir at config 3's shape (development tool): 127 taps, D = 4, 2^24 outputs, complex
float input, against
  (a) gsdrAmDemod on the same input (the same staging, mix and MACs; 4 instead of 8 output bytes), and
  (b) the three-pass route without the fused call: gsdrMultiplyCC by a precomputed phasor buffer, then gsdrFirFC.
(a) and (b) come from --ref-lib (another build of the library, e.g. the parent commit's) when given, else from the
library under test. The legs alternate within each round and the input buffers rotate, so every call streams its
input from HBM; HIP events around `reps` calls a leg.

    python tools/xlate_time.py [--ref-lib PATH] [--rounds 5] [--reps 20]
"""
import argparse
import ctypes
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from gsdr_amd import abi  # noqa: E402
from gsdr_amd.signals import lowpass_taps  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--ref-lib", default=None)
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--reps", type=int, default=20)
ap.add_argument("--outputs", type=int, default=1 << 24)
# firstSampleIndex of every call: 4 puts output 0 one output into its tile (tile_shift 1: the anchored tiles'
# stores are then 8 bytes off their 16-byte alignment and leave one output at a time)
ap.add_argument("--first-sample-index", type=int, default=0)
opt = ap.parse_args()


def load(path):
    h = ctypes.CDLL(path)
    for name in ("gsdrAmDemod", "gsdrMultiplyCC", "gsdrFirFC"):
        fn = getattr(h, name)
        fn.restype, fn.argtypes = abi.SIGNATURES[name]
    return h


ref = load(opt.ref_lib) if opt.ref_lib else abi.lib
D, T, N = 4, 127, opt.outputs
L = (N - 1) * D + T
FS, TUNE, CHAN = 1e6, 0.0, 1e5
N0 = opt.first_sample_index
dev = torch.device("cuda", 0)
stream = torch.cuda.current_stream(dev).cuda_stream
taps = torch.from_numpy(lowpass_taps(T, 0.1)).to(dev)
g = torch.Generator(device=dev).manual_seed(3)
xs = [(torch.rand(2 * L, device=dev, generator=g) * 2 - 1).view(torch.complex64) for _ in range(3)]
# (b)'s phasor buffer: any unit phasors do for the timing
ph = torch.polar(torch.ones(L, device=dev), torch.rand(L, device=dev, generator=g) * 6.2831853)
tmp = torch.empty(L, dtype=torch.complex64, device=dev)
yc = [torch.empty(N, dtype=torch.complex64, device=dev) for _ in range(2)]
yf = [torch.empty(N, dtype=torch.float32, device=dev) for _ in range(2)]
tp = taps.data_ptr()


def xlate(k):
    return abi.lib.gsdrxXlatingFir(FS, TUNE, CHAN, D, N0, tp, T, xs[k % 3].data_ptr(), yc[k % 2].data_ptr(), N, 0, stream)


def am(k):
    return ref.gsdrAmDemod(FS, TUNE, CHAN, D, N0, tp, T, xs[k % 3].data_ptr(), yf[k % 2].data_ptr(), N, 0, stream)


def three_pass(k):
    e = ref.gsdrMultiplyCC(xs[k % 3].data_ptr(), ph.data_ptr(), tmp.data_ptr(), L, 0, stream)
    return e or ref.gsdrFirFC(D, tp, T, tmp.data_ptr(), yc[k % 2].data_ptr(), N, 0, stream)


def timed(fn, reps):
    for k in range(3):
        assert fn(k) == 0
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for k in range(reps):
        fn(k)
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps * 1e3


legs = [("am_demod (a)", am), ("xlating_fir", xlate), ("am_demod (a) again", am), ("multiply + fir (b)", three_pass)]
times = {name: [] for name, _ in legs}
for _ in range(opt.rounds):
    for name, fn in legs:
        times[name].append(timed(fn, opt.reps))
print("outputs %d, taps %d, D %d, firstSampleIndex %d; reference legs from %s" %
      (N, T, D, N0, opt.ref_lib or "the library under test"))
for name, _ in legs:
    v = times[name]
    print("%-20s median %8.1f us  (min %8.1f, max %8.1f; rounds: %s)" %
          (name, statistics.median(v), min(v), max(v), " ".join("%.1f" % t for t in v)))
a = statistics.median(times["am_demod (a)"])
a2 = statistics.median(times["am_demod (a) again"])
x = statistics.median(times["xlating_fir"])
b = statistics.median(times["multiply + fir (b)"])
print("xlating_fir / am_demod = %.3f (expected <= 1.11 + spread); spread of (a) between its two legs %.3f; "
      "(b) / xlating_fir = %.2f" % (x / a, abs(a - a2) / a, b / x))
