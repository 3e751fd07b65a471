"""GPU: the chain modes -- IQ (gsdrxXlatingFir), AM and FM -- on every complex-sample tile shape of the FIR engine
(rows C1 ... C64 of GSDR_FIR_ROWS) and on the runtime-decimation tile, each at its own tap-chunk and tile edges
(tests/fir_sweep.py; test_fir_sweep_plan.py proves on the host that each call here reaches the row it names).

The chains run the polyphase core without the FIR mode's round-8 changes (another carried-row path), mix through the
NCO while staging, and place their tiles on an absolute output grid: firstSampleIndex = 0, D and D (S - 1) put
output 0 first in its tile, second, and last (the tile before it all negative indices). Per (row, mode), for 1, 2 and
3 tap chunks, full and with a last chunk of one tap, and for one output, one short of a tile stride S, S, S + 1 and
2 S + 3: the bars of the existing chain tests against the C oracle (IQ normwise, AM absolute, FM wrapped angle, all
1e-5), and the N-output call bit-identical to the first N outputs of the largest. IQ outputs are written between
guard elements. Measured maxima: DESIGN.md section 6.
"""
import numpy as np
import pytest
import torch

import fir_sweep as sw
from helpers import FLOAT_TOL, bound, check_guards, guarded, normwise_err, wrapped_angle_err
from oracle import oracle as o

pytestmark = pytest.mark.gpu

FS, TUNE, CHAN, DEV = 1.0e6, 0.0, 1.0e5, 2.0e4
SENTINEL = complex(-7.5, 1234.5)


def fm_gain():
    return float(np.float32(FS) / (np.float32(2.0) * np.float32(np.pi) * np.float32(DEV)))


def dev(a, cuda):
    return torch.from_numpy(np.ascontiguousarray(a)).to(cuda)


def bits(t):
    return (torch.view_as_real(t) if t.is_complex() else t).view(torch.int32)


def same_bits(a, b):
    return a.shape == b.shape and torch.equal(bits(a), bits(b))


def taps_for(T):
    from gsdr_amd.signals import lowpass_taps

    return lowpass_taps(T, 0.1 if T > 1 else 0.5)


def samples_for(mode, D, T, N):
    """Input samples N outputs read: FM pairs output N - 1 with FIR output N."""
    return (N if mode == sw.FM else N - 1) * D + T


def signal(mode, L, seed):
    from gsdr_amd.signals import fm_test_signal, uniform_iq

    if mode == sw.FM:
        return fm_test_signal(L, fs=FS, noise=0.05, seed=seed)
    return (0.7 * uniform_iq(L, seed=seed)).astype(np.complex64)


def call(cuda, mode, xd, td, D, first, N):
    """The mode's entry point; IQ into a guarded buffer, whose guards are checked."""
    from gsdr_amd import ops

    if mode == sw.FM:
        return ops.fm_demod(xd, td, FS, TUNE, CHAN, DEV, D, first, N)
    if mode == sw.AM:
        return ops.am_demod(xd, td, FS, TUNE, CHAN, D, first, N)
    buf, out = guarded(cuda, torch.complex64, N, 0, SENTINEL)
    got = ops.xlating_fir(xd, td, FS, TUNE, CHAN, D, first, N, out=out)
    assert got.data_ptr() == out.data_ptr()
    check_guards(buf, out, SENTINEL, what=f"D={D} firstSampleIndex={first} N={N}")
    return out


def reference(mode, x, taps, D, first, N):
    if mode == sw.FM:
        return o.fm_demod(x, taps, FS, TUNE, CHAN, DEV, D, first, N)
    if mode == sw.AM:
        return o.am_demod(x, taps, FS, TUNE, CHAN, D, first, N)
    return o.chain_fir(x, taps, FS, TUNE, CHAN, D, first, N)


def error(mode, got, ref, taps, x, D):
    """The mode's error figure, to be held against FLOAT_TOL."""
    if mode == sw.FM:
        return wrapped_angle_err(got, ref, fm_gain())
    if mode == sw.AM:
        return float(np.max(np.abs(got - ref)))
    return normwise_err(got, ref, bound(taps, x, D, len(ref)))


def sweep(cuda, name, family, mode, D, ts, ns, firsts):
    worst = 0.0
    nmax = ns[-1]
    for T in ts:
        taps = taps_for(T)
        x = signal(mode, samples_for(mode, D, T, nmax), seed=D * 1000 + T)
        td, xd = dev(taps, cuda), dev(x, cuda)
        for first in firsts:
            ref = reference(mode, x, taps, D, first, nmax)
            full = call(cuda, mode, xd, td, D, first, nmax)
            for N in ns:
                y = call(cuda, mode, xd[:samples_for(mode, D, T, N)], td, D, first, N)
                where = f"{name} T={T} firstSampleIndex={first} N={N}"
                assert same_bits(y, full[:N]), f"{where}: not the first outputs of the {nmax}-output call"
                err = error(mode, y.cpu().numpy(), ref[:N], taps, x, D)
                worst = max(worst, err)
                assert err <= FLOAT_TOL, f"{where}: error {err:.3e}"
    print(f"SWEEP {sw.MODE_NAMES[mode]} family={family} case={name} max_err={worst:.3e}")


@pytest.mark.parametrize("param", sw.CHAIN_PARAMS, ids=sw.chain_id)
def test_row_tap_and_tile_edges(cuda, param):
    row, mode = param
    ts, ns, firsts = sw.chain_grid(row, mode)
    sweep(cuda, sw.chain_id(param), sw.FAMILY_NAMES[row.kernel], mode, row.D, ts, ns, firsts)


@pytest.mark.parametrize("param", sw.RT_CHAIN_PARAMS, ids=sw.rt_chain_id)
def test_runtime_d_tap_and_tile_edges(cuda, param):
    D, mode = param
    ts, ns, firsts = sw.rt_chain_grid(D, mode)
    sweep(cuda, sw.rt_chain_id(param), "runtime-D", mode, D, ts, ns, firsts)


@pytest.mark.parametrize("mode", [sw.IQ, sw.AM], ids=["iq", "am"])
def test_d4_512_output_tiles(cuda, mode):
    """D = 4 one output past the 256-output tiles' range: the 512-output tiles (C4R2) in chain mode. Its head, a window
    across a middle tile edge and its tail equal 515-output calls starting there (firstSampleIndex moved along) bit
    for bit, and the oracle within the bar."""
    D, T, W, first = 4, sw.D4_CHAIN_T, sw.D4_WINDOW, sw.D4_CHAIN_FIRST
    cus = torch.cuda.get_device_properties(cuda).multi_processor_count
    N = sw.d4_n_r2(cus)
    taps = taps_for(T)
    x = signal(mode, samples_for(mode, D, T, N), seed=mode)
    td, xd = dev(taps, cuda), dev(x, cuda)
    y = call(cuda, mode, xd, td, D, first, N)
    worst = 0.0
    for k0 in sw.big_windows(N, 512):
        lo, hi = k0 * D, k0 * D + samples_for(mode, D, T, W)
        part = call(cuda, mode, xd[lo:hi], td, D, first + k0 * D, W)
        assert same_bits(part, y[k0:k0 + W]), f"window at output {k0}"
        ref = reference(mode, x[lo:hi], taps, D, first + k0 * D, W)
        worst = max(worst, error(mode, part.cpu().numpy(), ref, taps, x[lo:hi], D))
    print(f"SWEEP {sw.MODE_NAMES[mode]} family=polyphase case=C4R2-by-size max_err={worst:.3e}")
    assert worst <= FLOAT_TOL
