"""GPU: the frequency-translating FIR (gsdrxXlatingFir / Int8 / Multi, GSDRX_STREAM_XLATE) -- the tuned, filtered,
decimated complex baseband signal, i.e. the FIR stage of gsdrAmDemod with the NCO's absolute phase kept.

Bars: parity with the oracle's chain_fir at the project's float bar (normwise 1e-5, helpers.py); every split of a
stream into calls, the streaming object, the multi-channel call and the int8 front end bit for bit. The outputs are
written into the middle of a larger buffer whose guard elements must stay untouched: the anchored polyphase tiles'
first tile starts before output 0.
"""
import numpy as np
import pytest
import torch

from helpers import FLOAT_TOL, bound, check_guards, guarded, normwise_err
from oracle import oracle as o

pytestmark = pytest.mark.gpu

FS, TUNE, CHAN = 1.0e6, 0.0, 1.0e5
N_SMALL = 2 * 4096 + 11  # at least three NCO cells at every tiled decimation
SENTINEL = complex(-7.5, 1234.5)


def dev(a, cuda):
    return torch.from_numpy(np.ascontiguousarray(a)).to(cuda)


def taps_for(T):
    from gsdr_amd.signals import lowpass_taps

    return lowpass_taps(T, 0.1 if T > 1 else 0.5)


def signal(L, seed):
    from gsdr_amd.signals import uniform_iq

    return (0.7 * uniform_iq(L, seed=seed)).astype(np.complex64)


def guarded_call(cuda, x, taps, D, n0, N):
    """ops.xlating_fir into the middle of a sentinel-filled buffer; returns the outputs after checking the guards."""
    from gsdr_amd import ops

    buf, out = guarded(cuda, torch.complex64, N, 0, SENTINEL)
    got = ops.xlating_fir(x, taps, FS, TUNE, CHAN, D, n0, N, out=out)
    torch.cuda.synchronize()
    assert got.data_ptr() == out.data_ptr()
    check_guards(buf, out, SENTINEL)
    return out.cpu().numpy()


@pytest.mark.parametrize("n0", [0, 987654321, (1 << 32) + 5])
@pytest.mark.parametrize("T", [1, 31, 127])
@pytest.mark.parametrize("D", [1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 12, 13, 16, 20, 24, 32, 40, 48, 50, 64])
def test_parity_with_oracle(cuda, D, T, n0):
    """Every decimation with a row of its own (contiguous absolute D = 1, 3, 5, 7; anchored polyphase with R > 1
    (2, 4, 6, 8, 10, 12, 16) and R = 1 (20, 24, 32, 40, 48, 64)) and runtime-D 9, 13, 50 against oracle.chain_fir.
    Measured maximum over all cases: see DESIGN.md section 6."""
    N = N_SMALL
    x = signal((N - 1) * D + T, seed=D * T)
    taps = taps_for(T)
    got = guarded_call(cuda, dev(x, cuda), dev(taps, cuda), D, n0, N)
    ref = o.chain_fir(x, taps, FS, TUNE, CHAN, D, n0, N)
    err = normwise_err(got, ref, bound(taps, x, D, N))
    print(f"xlate parity D={D} T={T} n0={n0}: normwise error {err:.3e} (bar {FLOAT_TOL:.1e})")
    assert err <= FLOAT_TOL


def nco_phase(n0, L, inc):
    """P(n) = (n0 + n) inc mod 2^32 for n in [0, L), in exact integers, as float64 turns."""
    n = np.arange(L, dtype=np.uint64) + np.uint64(n0 % (1 << 32))
    p = (n * np.uint64(inc)) & np.uint64(0xFFFFFFFF)  # (uint64 products wrap mod 2^64, which keeps the low 32 bits)
    # check a few against Python integers
    for k in (0, 1, L // 2, L - 1):
        assert int(p[k]) == ((n0 + k) * inc) % (1 << 32)
    return p.astype(np.float64) / 2.0 ** 32


@pytest.mark.parametrize("D", [2, 4, 8])
def test_absolute_phase_across_cells(cuda, D):
    """The tone the NCO cancels exactly, x[n] = a exp(-j 2 pi P(n) / 2^32): the output is the constant a (the taps
    have unit DC gain) -- but only with each cell's anchor phase restored; left in the anchored frame the output's
    phase would jump at every cell boundary. Reference: a float64 restatement of the definition with the same
    integer phase, applied to the float32-rounded input."""
    from gsdr_amd import ops

    T, N, n0, a = 31, N_SMALL, 987654321, 0.7
    L = (N - 1) * D + T
    inc = ops.nco_phase_increment(FS, TUNE, CHAN)
    turns = nco_phase(n0, L, inc)
    x = (a * np.exp(-2j * np.pi * turns)).astype(np.complex64)
    taps = taps_for(T)
    z = x.astype(np.complex128) * np.exp(2j * np.pi * turns)
    ref = np.correlate(z, taps.astype(np.float64), mode="valid")[::D][:N]
    assert ref.size == N and np.max(np.abs(ref - a)) < 1e-6  # the tone is cancelled: a constant
    got = guarded_call(cuda, dev(x, cuda), dev(taps, cuda), D, n0, N)
    err = normwise_err(got, ref, bound(taps, x, D, N))
    print(f"xlate cancelled tone D={D}: normwise error {err:.3e} (bar {FLOAT_TOL:.1e})")
    assert err <= FLOAT_TOL


@pytest.mark.parametrize("D", [4, 3])
def test_no_taps_writes_zeros(cuda, D):
    """numTaps == 0 (null taps allowed): every output is zero, and nothing outside the output is written."""
    N = 1000
    x = dev(signal((N - 1) * D + 1, seed=D), cuda)
    taps = torch.empty(0, dtype=torch.float32, device=cuda)
    got = guarded_call(cuda, x, taps, D, 12345, N)
    assert np.all(got == 0)


@pytest.mark.parametrize("D", [4, 2, 1])
def test_input_8_bytes_off_alignment_bit_identical(cuda, D):
    """The shifted staging (input one sample off 16-byte alignment), with output 0 inside its tile (n0 = 1333 D + 1:
    the first tile starts before the buffer), equals the aligned call bit for bit."""
    from gsdr_amd import ops

    T, N, n0 = 31, N_SMALL, D * 1333 + 1
    x = dev(signal((N - 1) * D + T, seed=D), cuda)
    taps = dev(taps_for(T), cuda)
    y = torch.cat([torch.zeros(1, dtype=x.dtype, device=cuda), x])[1:]
    assert x.data_ptr() % 16 == 0 and y.data_ptr() % 16 == 8
    aligned = ops.xlating_fir(x, taps, FS, TUNE, CHAN, D, n0, N)
    shifted = ops.xlating_fir(y, taps, FS, TUNE, CHAN, D, n0, N)
    torch.cuda.synchronize()
    assert torch.equal(aligned.view(torch.int32), shifted.view(torch.int32))


def chunked(call, x, D, T, n0, sizes):
    parts, m = [], 0
    for n in sizes:
        parts.append(call(x[m * D:(m + n - 1) * D + T], n0 + m * D, n))
        m += n
    return torch.cat(parts), m


@pytest.mark.parametrize("D", [4, 1, 3, 5, 2])
def test_hand_cut_chunks_equal_one_call(cuda, D):
    """Chunked calls, each given its own firstSampleIndex, reproduce one call bit for bit: the per-sample phasors
    and each cell's anchor phasor are functions of absolute indices alone."""
    from gsdr_amd import ops

    T, N, n0 = 127, 30000, 1000
    x = dev(signal((N - 1) * D + T, seed=3), cuda)
    taps = dev(taps_for(T), cuda)

    def call(xs, first, n):
        return ops.xlating_fir(xs, taps, FS, TUNE, CHAN, D, first, n)

    whole = call(x, n0, N)
    got, m = chunked(call, x, D, T, n0, (7000, 1, 12345, N - 7000 - 1 - 12345))
    torch.cuda.synchronize()
    assert m == N
    assert torch.equal(got.view(torch.int32), whole.view(torch.int32))


@pytest.mark.parametrize("D", [2, 4])
def test_split_straddles_2_pow_32_outputs(cuda, D):
    """Split invariance where the absolute output index firstSampleIndex / D crosses 2^32 (the second chunk ends
    exactly at output 2^32), and a call wholly above the boundary against the oracle and its own split."""
    from gsdr_amd import ops

    T, N = 31, 4096
    x_np = signal((N - 1) * D + T, seed=D)
    taps_np = taps_for(T)
    x, taps = dev(x_np, cuda), dev(taps_np, cuda)

    def call(xs, first, n):
        return ops.xlating_fir(xs, taps, FS, TUNE, CHAN, D, first, n)

    n0 = D * ((1 << 32) - 2048) + 1
    whole = call(x, n0, N)
    got, m = chunked(call, x, D, T, n0, (1000, 1048, 1, 2047))
    assert m == N and torch.equal(got.view(torch.int32), whole.view(torch.int32))

    n0 = D * ((1 << 32) + 777)
    above = call(x, n0, N)
    got, m = chunked(call, x, D, T, n0, (1500, N - 1500))
    torch.cuda.synchronize()
    assert m == N and torch.equal(got.view(torch.int32), above.view(torch.int32))
    ref = o.chain_fir(x_np, taps_np, FS, TUNE, CHAN, D, n0, N)
    assert normwise_err(above.cpu().numpy(), ref, bound(taps_np, x_np, D, N)) <= FLOAT_TOL


def stream_chunks(total, seed, W):
    """Random chunk sizes including 0, 1, shorter than the window and several tiles (as test_gpu_stream.py)."""
    rng = np.random.default_rng(seed)
    sizes = []
    while sum(sizes) < total:
        sizes.append(int(rng.choice([0, 1, 2, W - 1, W + 3, int(rng.integers(1, 3 * W)), int(rng.integers(1, 40000))])))
    sizes[-1] -= sum(sizes) - total
    return sizes


def int8_iq(L, seed):
    return np.random.default_rng(seed).integers(-128, 128, 2 * L, dtype=np.int8)


@pytest.mark.parametrize("D", [1, 3, 4, 8])
@pytest.mark.parametrize("int8", [False, True])
def test_stream_equals_one_call(cuda, D, int8):
    """GSDRX_STREAM_XLATE on the one-launch path (D = 1, 3, 4, 8 are all tiled kernels) and, for chunks whose
    outputs all lie in the seam, through the same launch's history reads."""
    from gsdr_amd import ops
    from gsdr_amd.stream import Stream

    T, n0 = 127, 4_000_000_123
    L = 150_000 + 7 * D
    xd = dev(int8_iq(L, seed=D) if int8 else signal(L, seed=D), cuda)
    per = 2 if int8 else 1
    taps = dev(taps_for(T), cuda)
    want = ops.xlating_fir(xd, taps, FS, TUNE, CHAN, D, n0)
    s = Stream("xlate", taps, D, FS, TUNE, CHAN, first_sample_index=n0, int8=int8)
    parts, pos = [], 0
    for m in stream_chunks(L, seed=D * 10 + int8, W=T):
        parts.append(s.process(xd[pos * per:(pos + m) * per]).clone())
        pos += m
    s.close()
    got = torch.cat(parts)
    torch.cuda.synchronize()
    assert got.dtype == torch.complex64 and got.numel() == want.numel() == (L - T) // D + 1
    assert torch.equal(got.view(torch.int32), want.view(torch.int32))


@pytest.mark.parametrize("D", [9, 13])
def test_stream_seam_path_equals_one_call(cuda, D):
    """Decimations on the runtime-D kernel have no one-launch step: the stream's seam plan (gather, seam outputs,
    direct outputs) calls gsdrxXlatingFir itself."""
    from gsdr_amd import ops
    from gsdr_amd.stream import Stream

    T, n0, L = 31, 12345, 40_000
    xd = dev(signal(L, seed=D), cuda)
    taps = dev(taps_for(T), cuda)
    want = ops.xlating_fir(xd, taps, FS, TUNE, CHAN, D, n0)
    s = Stream("xlate", taps, D, FS, TUNE, CHAN, first_sample_index=n0)
    parts, pos = [], 0
    for m in (0, 1, T - 1, 5, 3 * T, 17001, L - 17001 - 4 * T - 5):
        parts.append(s.process(xd[pos:pos + m]).clone())
        pos += m
    s.close()
    torch.cuda.synchronize()
    assert pos == L
    assert torch.equal(torch.cat(parts).view(torch.int32), want.view(torch.int32))


def channel_list(C):
    return [float(v) for v in np.linspace(-0.35, 0.35, C) * FS]


@pytest.mark.parametrize("int8", [False, True])
@pytest.mark.parametrize("D,C", [(4, 3), (4, 17), (2, 5), (8, 2), (3, 4)])
def test_multi_equals_single(cuda, D, C, int8):
    """gsdrxXlatingFirMulti: the grouped kernel (D = 2, 4, 8; 17 channels = two launches) and the per-channel
    fallback (D = 3); channel c's row at c * numOutputs complex elements."""
    from gsdr_amd import ops

    T, N, n0 = 127, N_SMALL, 987654321
    L = (N - 1) * D + T
    x = dev(int8_iq(L, seed=C) if int8 else signal(L, seed=C), cuda)
    taps = dev(taps_for(T), cuda)
    chans = channel_list(C)
    multi = ops.xlating_fir_multi(x, taps, FS, TUNE, chans, D, n0, N)
    assert multi.shape == (C, N) and multi.dtype == torch.complex64
    for c in range(C):
        one = ops.xlating_fir(x, taps, FS, TUNE, chans[c], D, n0, N)
        assert torch.equal(multi[c].view(torch.int32), one.view(torch.int32)), c


def test_multi_stream_equals_single_calls(cuda):
    from gsdr_amd import ops
    from gsdr_amd.stream import Stream

    D, C, T, n0, L = 4, 3, 127, 4_000_000_123, 100_003
    x = dev(signal(L, seed=5), cuda)
    taps = dev(taps_for(T), cuda)
    chans = channel_list(C)
    s = Stream("xlate", taps, D, FS, TUNE, chans, first_sample_index=n0)
    parts, pos = [], 0
    for m in stream_chunks(L, seed=43, W=T):
        parts.append(s.process(x[pos:pos + m]).clone())
        pos += m
    s.close()
    got = torch.cat(parts, dim=1)
    torch.cuda.synchronize()
    assert got.shape == (C, (L - T) // D + 1)
    for c in range(C):
        one = ops.xlating_fir(x, taps, FS, TUNE, chans[c], D, n0)
        assert torch.equal(got[c].contiguous().view(torch.int32), one.view(torch.int32)), c


@pytest.mark.parametrize("T", [31, 127, 133])
@pytest.mark.parametrize("D", [1, 2, 4, 5])
def test_int8_equals_converted_float(cuda, D, T):
    """gsdrxXlatingFirInt8 = gsdrInt8ToNormFloat, then gsdrxXlatingFir, bit for bit -- at D = 4 too (no matrix-core
    form; T = 133 is past the matrix-core chains' tap limit, where FM / AM also take the float tiles)."""
    from gsdr_amd import ops

    N, n0 = N_SMALL, 987654321
    L = (N - 1) * D + T
    x8 = dev(int8_iq(L, seed=D * T), cuda)
    taps = dev(taps_for(T), cuda)
    xf = torch.view_as_complex(ops.int8_to_norm_float(x8).view(L, 2))
    got = ops.xlating_fir(x8, taps, FS, TUNE, CHAN, D, n0, N)
    want = ops.xlating_fir(xf, taps, FS, TUNE, CHAN, D, n0, N)
    torch.cuda.synchronize()
    assert torch.equal(got.view(torch.int32), want.view(torch.int32))


@pytest.mark.parametrize("D", [4, 3])
def test_consistent_with_am_demod(cuda, D):
    """gsdrAmDemod is the envelope 2 saturate(|y|) - 1 of this call's output y (am.h): gsdrMagnitude of y, mapped the
    same way, is within the AM parity bar (1e-5 absolute) of gsdrAmDemod on the same arguments; so is
    gsdrQuadAmDemod, the library's own envelope of a complex baseband signal."""
    from gsdr_amd import ops

    T, N, n0 = 127, N_SMALL, 987654321
    x = dev(signal((N - 1) * D + T, seed=D), cuda)
    taps = dev(taps_for(T), cuda)
    y = ops.xlating_fir(x, taps, FS, TUNE, CHAN, D, n0, N)
    am = ops.am_demod(x, taps, FS, TUNE, CHAN, D, n0, N)
    env = 2.0 * ops.magnitude(y).clamp(0.0, 1.0) - 1.0
    torch.cuda.synchronize()
    assert float((env - am).abs().max()) <= 1e-5
    assert float((ops.quad_am_demod(y) - am).abs().max()) <= 1e-5


@pytest.mark.parametrize("D", [4, 1])
def test_nonfinite_samples_stay_in_their_windows(cuda, D):
    """One Inf and one NaN sample, mid-tile and at a tile edge: outputs whose window holds neither equal the run
    with those samples zeroed bit for bit; the others are non-finite in at least one component, as the oracle's."""
    from gsdr_amd import ops

    T, N, n0 = 31, N_SMALL, 0
    L = (N - 1) * D + T
    x = signal(L, seed=D + 40)
    # tiles of 1,024 (D = 4, 256-output sub-tiles) and 2,048 (D = 1) outputs: output 2048 starts a tile at both
    bad = {2048 * D: np.inf, 2048 * D - 1: np.nan, 700 * D + 1: np.nan, 5000 * D + 2: -np.inf}
    xz = x.copy()
    for s, v in bad.items():
        x[s] = np.complex64(complex(v, 0.25))
        xz[s] = 0
    taps_np = taps_for(T)
    taps = dev(taps_np, cuda)
    got = ops.xlating_fir(dev(x, cuda), taps, FS, TUNE, CHAN, D, n0, N).cpu().numpy()
    clean = ops.xlating_fir(dev(xz, cuda), taps, FS, TUNE, CHAN, D, n0, N).cpu().numpy()
    m = np.arange(N)
    hit = np.zeros(N, dtype=bool)
    for s in bad:
        hit |= (m * D <= s) & (s < m * D + T)
    assert hit.sum() >= 4 and (~hit).sum() > N // 2
    assert got[~hit].tobytes() == clean[~hit].tobytes()
    assert np.all(~(np.isfinite(got[hit].real) & np.isfinite(got[hit].imag)))
    ref = o.chain_fir(x, taps_np, FS, TUNE, CHAN, D, n0, N)
    assert np.all(~(np.isfinite(ref[hit].real) & np.isfinite(ref[hit].imag)))
    assert np.all(np.isfinite(ref[~hit].real) & np.isfinite(ref[~hit].imag))


def test_tuned_output_feeds_the_qpsk_demodulator(cuda):
    """End to end: QPSK symbols held 4 samples each on a carrier the NCO cancels, tuned with a 4-tap boxcar at
    D = 4 (each output = the sum of one symbol's 4 samples), demodulated by gsdrQpskDemodulate: the sent bits."""
    from gsdr_amd import ops
    from gsdr_amd.signals import random_bytes

    S, D, n0 = 4096, 4, 987654321
    bits = dev(random_bytes(S // 4, seed=7), cuda)
    sym = ops.qpsk_modulate(bits, S, 0.5).cpu().numpy()
    inc = ops.nco_phase_increment(FS, TUNE, CHAN)
    turns = nco_phase(n0, S * D, inc)
    x = (np.repeat(sym, D).astype(np.complex128) * np.exp(-2j * np.pi * turns)).astype(np.complex64)
    taps = dev(np.full(D, 0.25, dtype=np.float32), cuda)
    y = ops.xlating_fir(dev(x, cuda), taps, FS, TUNE, CHAN, D, n0, S)
    back = ops.qpsk_demodulate(y, S)
    torch.cuda.synchronize()
    assert np.max(np.abs(y.cpu().numpy() - sym)) < 1e-4
    assert torch.equal(back, bits)
