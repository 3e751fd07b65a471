#!/usr/bin/env python3
"""Bit comparison of the IIR entry points of two builds (development tool):
    python tools/iir_bits.py <other libgsdr.so> <other libgsdr_probes.so>
Every case calls the other build's and the working tree's library on the same input with the same random input and
output histories and compares y and both history buffers byte for byte. Both formulations are deterministic (fixed
scan trees, no floating-point atomics), so equality is the bar. One line per case; exit status 1 on any difference.
Multi-pass scan (gsdrIirFF / CC of libgsdr.so): orders 1, 2, 3, 4, 8 (order 3: K - 1 below the compiled state size)
at the tile edges and with a partial group at every level; orders 9, 16, 31 (the unfused routes); order 4 at 2^25 + 1
real samples (the per-level route past k_iir_scan_upper). Single pass (gsdrxIirFFSinglePass / CC of
libgsdr_probes.so): orders 1, 2, 4, 8 around one tile, five tiles and the first superblock edge. Real and complex,
each with the buffers 16-byte aligned and one sample off."""
import ctypes
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
p, sz, u32, i32 = ctypes.c_void_p, ctypes.c_size_t, ctypes.c_uint32, ctypes.c_int32
MAX_POLLS = 1 << 22


def load(path, single):
    lib = ctypes.CDLL(path)
    for name in ("gsdrxIirFFSinglePass", "gsdrxIirCCSinglePass") if single else ("gsdrIirFF", "gsdrIirCC"):
        fn = getattr(lib, name)
        fn.restype = ctypes.c_int
        fn.argtypes = [p, p, sz, p, p, p, p, sz] + ([u32] if single else []) + [i32, p]
    if single:
        lib.gsdrxIirSinglePassStatus.restype = ctypes.c_int
        lib.gsdrxIirSinglePassStatus.argtypes = [i32, p]
    return lib


def design(order):
    rng = np.random.default_rng(order)
    a = np.poly(rng.uniform(-0.8, 0.8, order) if order <= 8 else rng.uniform(-0.5, 0.5, order))
    return rng.uniform(-0.5, 0.5, order + 1).astype(np.float32), a.astype(np.float32)


def off_by(t, off):
    """a copy of t in fresh memory, `off` samples past a 16-byte boundary"""
    buf = torch.empty(t.numel() + 4, dtype=t.dtype, device=t.device)
    assert buf.data_ptr() % 16 == 0
    v = buf[off:off + t.numel()]
    v.copy_(t)
    return v


def run(lib, single, cplx, bd, ad, x, xh, yh, off, dev, st):
    xd, xhd, yhd = off_by(x, off), xh.clone(), yh.clone()
    y = off_by(torch.zeros_like(x), off)
    K = bd.numel()
    if single:
        fn = lib.gsdrxIirCCSinglePass if cplx else lib.gsdrxIirFFSinglePass
        rc = fn(bd.data_ptr(), ad.data_ptr(), K, xhd.data_ptr(), yhd.data_ptr(), xd.data_ptr(), y.data_ptr(), x.numel(),
                MAX_POLLS, dev.index, st)
        rc = rc or lib.gsdrxIirSinglePassStatus(dev.index, st)
    else:
        fn = lib.gsdrIirCC if cplx else lib.gsdrIirFF
        rc = fn(bd.data_ptr(), ad.data_ptr(), K, xhd.data_ptr(), yhd.data_ptr(), xd.data_ptr(), y.data_ptr(), x.numel(),
                dev.index, st)
    torch.cuda.synchronize()
    return rc, [t.contiguous().view(torch.uint8) for t in (y, xhd, yhd)]


def main():
    other = {False: load(sys.argv[1], False), True: load(sys.argv[2], True)}
    tree = {False: load(os.path.join(ROOT, "gsdr_amd", "libgsdr.so"), False),
            True: load(os.path.join(ROOT, "build", "probes", "libgsdr_probes.so"), True)}
    dev = torch.device("cuda", 0)
    st = torch.cuda.current_stream(dev).cuda_stream
    g = torch.Generator(device=dev).manual_seed(11)
    T = 8192  # real samples a single-pass tile
    cases = [(False, o, n, c) for o in (1, 2, 3, 4, 8) for n in (1, 31, 32, 33, 2048, 2049, 4096, 4097, 131105)
             for c in (False, True)]
    cases += [(False, o, n, c) for o in (9, 16, 31) for n in (33, 4101, 131105) for c in (False, True)]
    cases += [(False, 4, (1 << 25) + 1, False)]
    cases += [(True, o, n, c) for o in (1, 2, 4, 8) for n in (1, T - 1, T, T + 1, 5 * T + 17, 256 * T + 1)
              for c in (False, True)]
    bad = 0
    for single, order, n, cplx in cases:
        b, a = design(order)
        bd, ad = torch.from_numpy(b).to(dev), torch.from_numpy(a).to(dev)
        dt = torch.complex64 if cplx else torch.float32

        def rand(m):
            v = torch.rand((2 if cplx else 1) * m, device=dev, generator=g) * 2 - 1
            return v.view(dt) if cplx else v

        x, xh, yh = rand(n), rand(order), rand(order)
        for off in (0, 1):
            ro, want = run(other[single], single, cplx, bd, ad, x, xh, yh, off, dev, st)
            rt, got = run(tree[single], single, cplx, bd, ad, x, xh, yh, off, dev, st)
            same = [torch.equal(w, t) for w, t in zip(want, got)]
            ok = ro == 0 and rt == 0 and all(same)
            bad += not ok
            print(f"{'single' if single else 'scan':6s} order {order:2d} {'complex' if cplx else 'real':7s} n {n:9d} "
                  f"off {off}  rc {ro} {rt}  y {'same' if same[0] else 'DIFF'}  xh {'same' if same[1] else 'DIFF'}  "
                  f"yh {'same' if same[2] else 'DIFF'}", flush=True)
    print(f"{len(cases) * 2} cases, {bad} differ")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
