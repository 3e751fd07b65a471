"""GPU parity: gsdrFmDemod / gsdrAmDemod (fused NCO + FIR + decimation + demod) vs the C oracle.

Reference: src/fm.cu:21-69, 181-218; src/am.cu:21-81; NCO re-specified in SURVEY.md App. A.3
(the reference's k_AdjustFrequency never returns its value, adjustFrequency.cu:56).
Bars: FM -- wrapped-angle error <= 1e-5 of full scale (pi * g) on a constant-envelope signal;
AM -- absolute error <= 1e-5 (outputs in [-1, 1]); the FIR stage itself is checked normwise via AM.
"""
import numpy as np
import pytest
import torch

from helpers import FLOAT_TOL, wrapped_angle_err
from oracle import oracle as o

pytestmark = pytest.mark.gpu

FS, TUNE, CHAN, DEV = 1.0e6, 0.0, 1.0e5, 2.0e4


def fm_gain():
    return float(np.float32(FS) / (np.float32(2.0) * np.float32(np.pi) * np.float32(DEV)))


def dev(a, cuda):
    return torch.from_numpy(np.ascontiguousarray(a)).to(cuda)


@pytest.mark.parametrize("n0", [0, 987654321, (1 << 32) + 5])
@pytest.mark.parametrize("T", [1, 31, 127])
@pytest.mark.parametrize("D", [1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 12, 13, 16, 20, 24, 32, 40, 48, 50, 64])
def test_fm_demod_parity(cuda, D, T, n0):
    from gsdr_amd import ops
    from gsdr_amd.signals import fm_test_signal, lowpass_taps

    N = 2 * 4096 + 11
    x = fm_test_signal(N * D + T, fs=FS, noise=0.05, seed=D + T, n0=n0 % (1 << 20))
    taps = lowpass_taps(T, 0.1 if T > 1 else 0.5)
    out = ops.fm_demod(dev(x, cuda), dev(taps, cuda), FS, TUNE, CHAN, DEV, D, n0, N)
    torch.cuda.synchronize()
    ref = o.fm_demod(x, taps, FS, TUNE, CHAN, DEV, D, n0, N)
    assert wrapped_angle_err(out.cpu().numpy(), ref, fm_gain()) <= FLOAT_TOL


@pytest.mark.parametrize("n0", [0, (1 << 32) + 5])
@pytest.mark.parametrize("T", [1, 31, 127])
@pytest.mark.parametrize("D", [1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 12, 13, 16, 20, 24, 32, 40, 48, 50, 64])
def test_am_demod_parity(cuda, D, T, n0):
    from gsdr_amd import ops
    from gsdr_amd.signals import lowpass_taps, uniform_iq

    N = 2 * 4096 + 11
    x = (0.7 * uniform_iq((N - 1) * D + T, seed=D * T)).astype(np.complex64)
    taps = lowpass_taps(T, 0.1 if T > 1 else 0.5)
    out = ops.am_demod(dev(x, cuda), dev(taps, cuda), FS, TUNE, CHAN, D, n0, N)
    torch.cuda.synchronize()
    ref = o.am_demod(x, taps, FS, TUNE, CHAN, D, n0, N)
    assert float(np.max(np.abs(out.cpu().numpy() - ref))) <= FLOAT_TOL


def test_nco_against_golden_increment(cuda):
    from gsdr_amd import ops

    assert ops.nco_phase_increment(FS, TUNE, CHAN) == o.nco_inc(FS, TUNE, CHAN)


@pytest.mark.parametrize("D", [4, 1, 3, 5])
def test_fm_streaming_chunks_equal_monolithic(cuda, D):
    """Streaming contract (fm.h:26, firstSampleIndex fm.h:48): K chunked calls with numLowPassTaps of
    overlap reproduce one call bit for bit -- the NCO phase is a function of the absolute index and
    each FIR output is computed by the same arithmetic wherever its tile falls. Odd D puts chunks at
    8-byte-aligned addresses (shifted staging, odd-start NCO pairs)."""
    from gsdr_amd import ops
    from gsdr_amd.signals import fm_test_signal, lowpass_taps

    T, N = 127, 30000
    x = dev(fm_test_signal(N * D + T, fs=FS, seed=3), cuda)
    taps = dev(lowpass_taps(T, 0.1), cuda)
    whole = ops.fm_demod(x, taps, FS, TUNE, CHAN, DEV, D, 1000, N)
    parts, m = [], 0
    for n in (7000, 1, 12345, N - 7000 - 1 - 12345):
        xs = x[m * D:(m + n) * D + T]
        parts.append(ops.fm_demod(xs, taps, FS, TUNE, CHAN, DEV, D, 1000 + m * D, n))
        m += n
    torch.cuda.synchronize()
    assert torch.equal(torch.cat(parts), whole)


@pytest.mark.parametrize("D", [2, 4])
@pytest.mark.parametrize("kind", ["fm", "am"])
def test_chain_split_straddles_2_pow_32_outputs(cuda, kind, D):
    """The split-invariance contract where the absolute output index firstSampleIndex / D crosses 2^32: the
    anchored tiles' NCO cell grid is q0 mod the tile stride, and the FM strides (255 / 510 / 1020
    at D = 4, 1016 at D = 2) do not divide 2^32, so q0 has to be carried in 64 bits. Chunks on both sides of the
    boundary (the second ends exactly at output 2^32) reproduce one call bit for bit; a call wholly above the
    boundary meets the oracle and its own two-chunk split."""
    from gsdr_amd import ops
    from gsdr_amd.signals import fm_test_signal, lowpass_taps, uniform_iq

    T, N = 31, 4096
    fm = kind == "fm"
    L = (N if fm else N - 1) * D + T
    x_np = fm_test_signal(L, fs=FS, seed=D) if fm else (0.7 * uniform_iq(L, seed=D)).astype(np.complex64)
    taps_np = lowpass_taps(T, 0.1)
    x, taps = dev(x_np, cuda), dev(taps_np, cuda)

    def call(xs, n0, n):
        if fm:
            return ops.fm_demod(xs, taps, FS, TUNE, CHAN, DEV, D, n0, n)
        return ops.am_demod(xs, taps, FS, TUNE, CHAN, D, n0, n)

    def chunked(n0, sizes):
        parts, m = [], 0
        for n in sizes:
            parts.append(call(x[m * D:(m + (n if fm else n - 1)) * D + T], n0 + m * D, n))
            m += n
        assert m == N
        return torch.cat(parts)

    n0 = D * ((1 << 32) - 2048) + 1
    whole = call(x, n0, N)
    assert torch.equal(chunked(n0, (1000, 1048, 1, 2047)), whole)

    n0 = D * ((1 << 32) + 777)
    above = call(x, n0, N)
    torch.cuda.synchronize()
    if fm:
        ref = o.fm_demod(x_np, taps_np, FS, TUNE, CHAN, DEV, D, n0, N)
        assert wrapped_angle_err(above.cpu().numpy(), ref, fm_gain()) <= FLOAT_TOL
    else:
        ref = o.am_demod(x_np, taps_np, FS, TUNE, CHAN, D, n0, N)
        assert float(np.max(np.abs(above.cpu().numpy() - ref))) <= FLOAT_TOL
    assert torch.equal(chunked(n0, (1500, N - 1500)), above)


def misaligned(x):
    """The same samples one sample (8 bytes) off 16-byte alignment (run_fir's construction, test_gpu_fir.py)."""
    y = torch.cat([torch.zeros(1, dtype=x.dtype, device=x.device), x])[1:]
    assert x.data_ptr() % 16 == 0 and y.data_ptr() % 16 == 8
    return y


def d4_outputs(cuda, tiles):
    """An output count that reaches launch_poly_d4's tile shape `tiles` on this device: "tiles256" (256-output
    tiles, three NCO cells), "tiles512" (140,001 outputs, or more on a device with more CUs), "tiles1024" (just
    inside the 1,024-output tiles)."""
    slots = 4 * torch.cuda.get_device_properties(cuda).multi_processor_count
    n256, n512, n1024 = 3 * 1020 + 7, max(140_001, 256 * (slots // 2) + 1), 3 * slots * 1024 + 1
    assert 2 * -(-n256 // 256) <= slots < 2 * -(-n512 // 256), (n256, n512, slots)
    assert -(-n512 // 1024) < 3 * slots <= -(-n1024 // 1024), (n512, n1024, slots)
    return {"tiles256": n256, "tiles512": n512, "tiles1024": n1024}[tiles]


@pytest.mark.parametrize("D,N", [(1, 2 * 4096 + 11), (3, 2 * 4096 + 11), (2, 2 * 4096 + 11), (4, "tiles256"),
                                 (4, "tiles512"), (6, 2 * 4096 + 11), (8, 2 * 4096 + 11), (20, 2 * 4096 + 11)])
@pytest.mark.parametrize("kind", ["fm", "am"])
def test_chain_float_misaligned_bit_identical(cuda, kind, D, N):
    """Float FM / AM with the input 8 bytes off 16-byte alignment (the shifted staging of complex samples: for the
    anchored polyphase tiles the previous lane's phasor chain beside the thread's own; for the absolute mixer of
    D = 1, 3 the odd-start pairs) equals the aligned call bit for bit, and the aligned call meets the oracle.
    n0 = 1333 D + 1 puts output 0 inside its tile (at D = 4: tile shift 58 (FM) / 53 (AM) in sub-tile 1 of its NCO
    cell), so the first tile starts before the buffer and drops off the shifted path, and the odd n0 starts the
    absolute mixer on the odd parity. D = 4 runs its 256-output (SUBS = 4, three cells) and 512-output (SUBS = 2)
    tile shapes."""
    from gsdr_amd import ops
    from gsdr_amd.signals import fm_test_signal, lowpass_taps, uniform_iq

    T, n0, fm = 31, D * 1333 + 1, kind == "fm"
    if isinstance(N, str):
        N = d4_outputs(cuda, N)
    L = (N if fm else N - 1) * D + T
    x_np = fm_test_signal(L, fs=FS, noise=0.05, seed=D) if fm else (0.7 * uniform_iq(L, seed=D)).astype(np.complex64)
    taps_np = lowpass_taps(T, 0.1)
    x, taps = dev(x_np, cuda), dev(taps_np, cuda)

    def call(xs):
        if fm:
            return ops.fm_demod(xs, taps, FS, TUNE, CHAN, DEV, D, n0, N)
        return ops.am_demod(xs, taps, FS, TUNE, CHAN, D, n0, N)

    aligned, shifted = call(x), call(misaligned(x))
    torch.cuda.synchronize()
    got = aligned.cpu().numpy()
    assert shifted.cpu().numpy().tobytes() == got.tobytes()
    if fm:
        err = wrapped_angle_err(got, o.fm_demod(x_np, taps_np, FS, TUNE, CHAN, DEV, D, n0, N), fm_gain())
    else:
        err = float(np.max(np.abs(got - o.am_demod(x_np, taps_np, FS, TUNE, CHAN, D, n0, N))))
    print(f"{kind} D={D} N={N}: error {err:.3e} (bar {FLOAT_TOL:.1e})")
    assert err <= FLOAT_TOL


def test_chain_float_misaligned_bit_identical_1024_tiles(cuda):
    """The same at D = 4, FM, on the 1,024-output tiles (a call just past launch_poly_d4's threshold): misaligned
    against aligned bytes only."""
    from gsdr_amd import ops
    from gsdr_amd.signals import lowpass_taps

    D, T, n0 = 4, 31, 4 * 1333 + 1
    N = d4_outputs(cuda, "tiles1024")
    gen = torch.Generator(device=cuda).manual_seed(4)
    x = torch.view_as_complex(torch.rand(N * D + T, 2, device=cuda, generator=gen) - 0.5)
    taps = dev(lowpass_taps(T, 0.1), cuda)
    aligned = ops.fm_demod(x, taps, FS, TUNE, CHAN, DEV, D, n0, N)
    shifted = ops.fm_demod(misaligned(x), taps, FS, TUNE, CHAN, DEV, D, n0, N)
    assert torch.equal(aligned.view(torch.int32), shifted.view(torch.int32))


def test_fm_pure_tone_known_answer(cuda):
    """A noiseless FM carrier at a constant offset f from the channel discriminates to the constant
    g * 2 pi f D'/fs where the discriminator sees decimated samples: arg step = 2 pi f D / fs."""
    from gsdr_amd import ops
    from gsdr_amd.signals import lowpass_taps

    D, T, N = 4, 127, 5000
    f = 1.0e5 + 2000.0  # 2 kHz above the channel centre
    n = np.arange(N * D + T)
    x = np.exp(2j * np.pi * f / FS * n).astype(np.complex64)
    out = ops.fm_demod(dev(x, cuda), dev(lowpass_taps(T, 0.1), cuda), FS, TUNE, CHAN, DEV, D, 0, N)
    torch.cuda.synchronize()
    want = fm_gain() * 2 * np.pi * 2000.0 * D / FS
    assert np.max(np.abs(out.cpu().numpy() - want)) < 1e-4 * abs(want) + 1e-6


def test_fm_full_config(cuda):
    """BASELINE config 3: NCO + 127-tap FIR (D = 4) + FM over 67,108,987 samples; oracle spot checks."""
    from gsdr_amd import ops
    from gsdr_amd.signals import fm_test_signal, lowpass_taps

    D, T, N = 4, 127, (1 << 24) - 1
    L = N * D + T
    x_np = fm_test_signal(L, fs=FS, noise=0.05, seed=0x5EED)
    taps = lowpass_taps(T, 0.1)
    x = dev(x_np, cuda)
    out = ops.fm_demod(x, dev(taps, cuda), FS, TUNE, CHAN, DEV, D, 0, N)
    torch.cuda.synchronize()
    got = out.cpu().numpy()
    for m0 in (0, N // 3, N - 3000):
        m1 = m0 + 3000
        ref = o.fm_demod(x_np, taps, FS, TUNE, CHAN, DEV, D, 0, N, m0, m1)
        assert wrapped_angle_err(got[m0:m1], ref[m0:m1], fm_gain()) <= FLOAT_TOL
    assert np.all(np.isfinite(got))
