"""GPU parity of the FM, AM and frequency-translating (IQ) chains across the NCO's frequency range and at long
filters. Every other oracle comparison of a chain runs at one increment (tune - chan = -0.1 fs) and at most 127 taps
(int8: 132); only the increment and the (int32) phase -> float conversion differ from frequency to frequency, and
chain_ref.FREQS holds the increments that are special to this implementation: 0, +-1, Nyquist, +-fs/4 and +-fs/8,
the ones that make the anchored mixer's row factor exactly 1, |tune - chan| > fs, a tuned, float-rounded difference.

Bars (the project's own): FM wrapped-angle error, AM maximum absolute error, IQ normwise error, each <= FLOAT_TOL
against the C oracle; the long-filter test compares with the float64 restatement instead (two fp32 summation orders
may each sit 3e-6 from the truth; test_nco_increment.py holds the oracle to 0.3 of the bar against the same
restatement). Each case asks the host launch plan (fir_plan.hpp, compiled as in test_fir_plan.py) which kernel
family it reaches and asserts it, so a change of the shape table cannot silently move a case to another kernel."""
import numpy as np
import pytest
import torch

from chain_ref import (FREQ_BY_NAME, FREQ_IDS, FREQS, am64, bound64, chain_fir64, deviation, fm64, fm_gain, inputs,
                       signed_inc, to_int8)
from helpers import FLOAT_TOL, bound, normwise_err, wrapped_angle_err
from oracle import oracle as o
from test_fir_plan import (AM, COMPLEX, COMPLEX_ROWS, CONTIG, FM, GENERIC, I8_CHAIN, IQ, IQ8, POLY, RT, TILED,
                           build_plan_program, case)
from test_gpu_chains import d4_outputs

pytestmark = pytest.mark.gpu

MODES = {"fm": FM, "am": AM, "iq": IQ}
N_SMALL = 2 * 4096 + 11


def dev(a, cuda):
    return torch.from_numpy(np.ascontiguousarray(a)).to(cuda)


def first_index(D):
    """Both parities of the first sample and a 64-bit index."""
    return 987654321 if D % 2 else (1 << 32) + 6


@pytest.fixture(scope="module")
def planner(tmp_path_factory, cuda):
    """plan(mode, D, T, N, n0, sample) -> the launch plan of that call on this device, aligned pointers."""
    run, _ = build_plan_program(tmp_path_factory.mktemp("chain_freq_plan"))
    cus = torch.cuda.get_device_properties(cuda).multi_processor_count

    def plan(mode, D, T, N, n0, sample=COMPLEX):
        q0 = n0 // D
        return run([case(sample=sample, mode=MODES[mode], D=D, T=T, N=N, q0=q0, phase=q0 & 15, cus=cus)])[0]

    return plan


def run_chain(cuda, mode, row, x, taps, D, n0, N):
    """The library's chain of `mode` at FREQS row `row`; x, taps: numpy arrays or device tensors. Returns numpy."""
    from gsdr_amd import ops

    _, fs, tune, chan, _ = row
    xd = x if torch.is_tensor(x) else dev(x, cuda)
    td = taps if torch.is_tensor(taps) else dev(taps, cuda)
    if mode == "fm":
        out = ops.fm_demod(xd, td, fs, tune, chan, deviation(fs), D, n0, N)
    elif mode == "am":
        out = ops.am_demod(xd, td, fs, tune, chan, D, n0, N)
    else:
        out = ops.xlating_fir(xd, td, fs, tune, chan, D, n0, N)
    torch.cuda.synchronize()
    return out.cpu().numpy()


def oracle_chain(mode, row, x, taps, D, n0, N):
    _, fs, tune, chan, _ = row
    if mode == "fm":
        return o.fm_demod(x, taps, fs, tune, chan, deviation(fs), D, n0, N)
    if mode == "am":
        return o.am_demod(x, taps, fs, tune, chan, D, n0, N)
    return o.chain_fir(x, taps, fs, tune, chan, D, n0, N)


def chain_err(mode, row, got, ref, x, taps, D, s=None):
    """The mode's error measure; `s`: the IQ normwise bounds where helpers.bound would be too slow."""
    if mode == "fm":
        return wrapped_angle_err(got, ref, fm_gain(row[1], deviation(row[1])))
    if mode == "am":
        return float(np.max(np.abs(got.astype(np.float64) - ref)))
    return normwise_err(got, ref, bound(taps, x, D, got.size) if s is None else s)


# ------------------------------------------------------------------------------------------------
# a. every frequency through every mixer family
# ------------------------------------------------------------------------------------------------
# absolute mixer (contiguous tiles) 1, 3; anchored mixer (polyphase tiles) with WG 128 / R 8 (2), WG 256 / R 1 of the
# short D = 4 call (4), WG 256 / R 2 (8), WG 128 / R 2 (16), WG 256 / R 1 (20), WG 64 / R 1 (64); the runtime-D tile
# unpaired (9) and paired (14); the generic kernel (T <= D at 100)
SWEEP_D = [1, 2, 3, 4, 8, 9, 14, 16, 20, 64, 100]


def assert_sweep_family(p, D):
    if D in (9, 14):
        assert p["family"] == RT and p["wg"] == 256 and p["paired"] == (1 if D % 2 == 0 else 0), p
    elif D == 100:
        assert p["family"] == GENERIC, p
    else:
        assert p["family"] == (CONTIG if D in (1, 3) else POLY), p
        if D == 4:
            assert (p["R"], p["SUBS"], p["WG"]) == (1, 4, 256), p
        else:
            assert (p["kernel"], p["R"], p["chunk"], p["WG"]) == COMPLEX_ROWS[D], p


@pytest.mark.parametrize("D", SWEEP_D)
@pytest.mark.parametrize("mode", ["fm", "am", "iq"])
@pytest.mark.parametrize("row", FREQS, ids=FREQ_IDS)
def test_frequency_sweep_vs_oracle(cuda, planner, row, mode, D):
    """Measured maxima: DESIGN.md section 6."""
    T, N, n0 = 31, N_SMALL, first_index(D)
    assert_sweep_family(planner(mode, D, T, N, n0), D)
    x, taps = inputs(mode, row, D, T, N, n0)
    got = run_chain(cuda, mode, row, x, taps, D, n0, N)
    err = chain_err(mode, row, got, oracle_chain(mode, row, x, taps, D, n0, N), x, taps, D)
    print(f"chain_freq sweep {mode} {row[0]} D={D}: error {err:.3e} (bar {FLOAT_TOL:.1e})")
    assert err <= FLOAT_TOL


# ------------------------------------------------------------------------------------------------
# b. the D = 4 tile shapes
# ------------------------------------------------------------------------------------------------
SHAPE_FREQS = ["nyquist", "f_one_wg256", "eighth", "third", "step_up"]


@pytest.mark.parametrize("mode", ["fm", "am", "iq"])
@pytest.mark.parametrize("name", SHAPE_FREQS)
def test_d4_512_output_tiles_vs_oracle(cuda, planner, name, mode):
    row = FREQ_BY_NAME[name]
    D, T, n0 = 4, 31, first_index(4)
    N = d4_outputs(cuda, "tiles512")
    p = planner(mode, D, T, N, n0)
    assert p["family"] == POLY and (p["R"], p["SUBS"], p["WG"]) == (2, 2, 256), p
    x, taps = inputs(mode, row, D, T, N, n0)
    got = run_chain(cuda, mode, row, x, taps, D, n0, N)
    err = chain_err(mode, row, got, oracle_chain(mode, row, x, taps, D, n0, N), x, taps, D)
    print(f"chain_freq tiles512 {mode} {name}: error {err:.3e} (bar {FLOAT_TOL:.1e})")
    assert err <= FLOAT_TOL


def device_signal(cuda, mode, row, L, n0, seed):
    """chain_ref.inputs' signals made on the device (12.6 M samples): the same construction, torch's generators."""
    gen = torch.Generator(device=cuda).manual_seed(seed)
    if mode != "fm":
        return torch.view_as_complex((torch.rand(L, 2, device=cuda, generator=gen) * 2.0 - 1.0) * 0.7)
    carrier = -signed_inc(row[4]) / 2.0 ** 32
    first = n0 % (1 << 20)
    idx = torch.arange(first, first + L, dtype=torch.float64, device=cuda)
    ph = 2.0 * np.pi * carrier * idx + 20.0 * torch.sin(2.0 * np.pi * 0.001 * idx)
    del idx
    x = torch.view_as_real(torch.polar(torch.ones_like(ph), ph).to(torch.complex64))
    del ph
    x += torch.randn(L, 2, dtype=torch.float32, device=cuda, generator=gen) * 0.05
    return torch.view_as_complex(x)


@pytest.mark.parametrize("mode", ["fm", "am", "iq"])
@pytest.mark.parametrize("name", SHAPE_FREQS)
def test_d4_1024_output_tiles_vs_oracle_windows(cuda, planner, name, mode):
    """Oracle windows of 3,000 outputs at the head, in the middle (three or more NCO cells of 1,020 / 1,024 outputs,
    so two cell boundaries at least) and at the tail."""
    from gsdr_amd.signals import lowpass_taps

    row = FREQ_BY_NAME[name]
    D, T, n0, W = 4, 31, first_index(4), 3000
    N = d4_outputs(cuda, "tiles1024")
    p = planner(mode, D, T, N, n0)
    assert p["family"] == POLY and (p["R"], p["SUBS"], p["WG"]) == (4, 1, 256), p
    taps = lowpass_taps(T, 0.1)
    x = device_signal(cuda, mode, row, N * D + T, n0, seed=len(name) + len(mode))
    got = run_chain(cuda, mode, row, x, taps, D, n0, N)
    for m0 in (0, N // 2 - W // 2, N - W):
        xs = x[m0 * D:(m0 + W) * D + T].cpu().numpy()
        ref = oracle_chain(mode, row, xs, taps, D, n0 + m0 * D, W)
        err = chain_err(mode, row, got[m0:m0 + W], ref, xs, taps, D)
        print(f"chain_freq tiles1024 {mode} {name} outputs {m0}..{m0 + W}: error {err:.3e} (bar {FLOAT_TOL:.1e})")
        assert err <= FLOAT_TOL
    assert np.all(np.isfinite(got.view(np.float32)))


# ------------------------------------------------------------------------------------------------
# c. int8 I/Q: the matrix-core chain (NCO folded into complex taps, the left-out rotation added back), its last tap
# count, and the exact float rows
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", [1023, N_SMALL])
@pytest.mark.parametrize("D,T", [(4, 127), (4, 132), (4, 133), (2, 31)])
@pytest.mark.parametrize("mode", ["fm", "am"])
@pytest.mark.parametrize("row", FREQS, ids=FREQ_IDS)
def test_int8_chains_vs_oracle(cuda, planner, row, mode, D, T, N):
    n0 = 4_000_000_123
    p = planner(mode, D, T, N, n0, sample=IQ8)
    assert p["family"] == (I8_CHAIN if D == 4 and T <= 132 else POLY), p
    x, taps = inputs(mode, row, D, T, N, n0)
    x8 = to_int8(x)
    xf = o.int8_to_float(x8).view(np.complex64)
    got = run_chain(cuda, mode, row, x8, taps, D, n0, N)
    ref = oracle_chain(mode, row, xf, taps, D, n0, N)
    err = chain_err(mode, row, got, ref, xf, taps, D)
    print(f"chain_freq int8 {mode} {row[0]} D={D} T={T} N={N}: error {err:.3e} (bar {FLOAT_TOL:.1e})")
    assert err <= FLOAT_TOL
    if mode == "fm" and row[0] in ("eighth", "minus_eighth"):
        # 4 inc = 2^31: the rotation the folded taps leave out sits at the wrap point -pi, so every angle is wrapped
        # after it is added. The wrapped measure forgives a wrong branch (a 2 pi g disagreement); away from +-pi g
        # the plain difference must meet the bar as well
        _, fs, _, _, inc = row
        g = fm_gain(fs, deviation(fs))
        ref64 = fm64(xf, taps, inc, fs, deviation(fs), D, n0, N)
        clear = np.abs(np.abs(ref64) - np.pi * g) > 1e-3 * np.pi * g
        assert clear.sum() > N // 2
        plain = float(np.max(np.abs(got.astype(np.float64) - ref)[clear])) / (np.pi * g)
        print(f"chain_freq int8 {mode} {row[0]} D={D} T={T} N={N}: unwrapped error {plain:.3e}")
        assert plain <= FLOAT_TOL


# ------------------------------------------------------------------------------------------------
# d. long filters in chain mode: the last tiled tap count and the first generic one, from the launch plan
# ------------------------------------------------------------------------------------------------
def largest_t(pred, lo=32, hi=1 << 16):
    """The largest T in [lo, hi) with pred(T), for a predicate that holds up to some T and not past it."""
    assert pred(lo) and not pred(hi)
    while hi - lo > 1:
        mid = (lo + hi) // 2
        lo, hi = (mid, hi) if pred(mid) else (lo, mid)
    return lo


LONG_CASES = [(D, which) for D in (1, 4, 8, 13, 20, 64) for which in ("last_tiled", "first_generic")] + \
    [(13, "wg128"), (13, "wg64"), (4, "last_tiled_512")]
# Frequency `third`; D = 64 (workgroups of 64, the longest phasor chain: about 60 rows of 64 granules at its last
# tiled tap count) at `positive`, where a probe over every row of FREQS at D = 16, 32 and 64 measured the largest error
LONG_FREQ = {64: "positive"}


@pytest.mark.parametrize("D,which", LONG_CASES)
@pytest.mark.parametrize("mode", ["fm", "am", "iq"])
def test_long_filters_vs_float64(cuda, planner, mode, D, which):
    """The chain modes leave the LDS budget at other tap counts than FIR mode (the exchange row), the anchored
    phasor chain grows by one multiply a staged row of halo, the runtime-D tile narrows to 128 and 64 outputs, and
    past the last tiled tap count the generic kernel takes over: none of the tap counts is written down here."""
    row = FREQ_BY_NAME[LONG_FREQ.get(D, "third")]
    _, fs, _, _, inc = row
    n0 = first_index(D)
    N = d4_outputs(cuda, "tiles512") if which == "last_tiled_512" else 3000 + D

    def plan(T):
        return planner(mode, D, T, N, n0)

    def tiled(T):
        return plan(T)["family"] in TILED

    if which == "last_tiled_512":
        T = largest_t(lambda t: tiled(t) and (plan(t)["R"], plan(t)["SUBS"]) == (2, 2))
        assert T > 133 and plan(T)["family"] == POLY
    elif which in ("last_tiled", "first_generic"):
        last = largest_t(tiled)
        assert last > 133 and plan(last + 1)["family"] == GENERIC
        T = last + (1 if which == "first_generic" else 0)
    else:
        t256 = largest_t(lambda t: tiled(t) and plan(t)["wg"] == 256)
        t128 = largest_t(lambda t: tiled(t) and plan(t)["wg"] >= 128)
        t64 = largest_t(tiled)
        assert t256 < t128 < t64
        T = (t256 + 1 + t128) // 2 if which == "wg128" else (t128 + 1 + t64) // 2
        assert plan(T)["family"] == RT and plan(T)["wg"] == (128 if which == "wg128" else 64)
    x, taps = inputs(mode, row, D, T, N, n0)
    got = run_chain(cuda, mode, row, x, taps, D, n0, N)
    if mode == "fm":
        ref = fm64(x, taps, inc, fs, deviation(fs), D, n0, N)
    elif mode == "am":
        ref = am64(x, taps, inc, D, n0, N)
    else:
        ref = chain_fir64(x, taps, inc, D, n0, N)
    err = chain_err(mode, row, got, ref, x, taps, D, s=bound64(x, taps, D, N))
    p = plan(T)
    print(f"chain_freq long {mode} D={D} {which}: T={T} N={N} family {p['family']} wg {p['wg']}: error {err:.3e} "
          f"against float64 (bar {FLOAT_TOL:.1e})")
    assert err <= FLOAT_TOL


# ------------------------------------------------------------------------------------------------
# e. split invariance at each frequency
# ------------------------------------------------------------------------------------------------
SPLIT_FREQS = ["nyquist", "f_one_wg256", "step_down", "tuned"]


@pytest.mark.parametrize("mode", ["fm", "iq"])
@pytest.mark.parametrize("D", [3, 4])
@pytest.mark.parametrize("name", SPLIT_FREQS)
def test_hand_cut_chunks_equal_one_call(cuda, name, D, mode):
    """As test_fm_streaming_chunks_equal_monolithic: chunks of (7000, 1, 12345, rest) outputs, each call given its own
    firstSampleIndex, reproduce one call of 30,000 outputs bit for bit."""
    row = FREQ_BY_NAME[name]
    T, N, n0 = 127, 30000, 1000
    x_np, taps_np = inputs(mode, row, D, T, N, n0, seed=3)
    x, taps = dev(x_np, cuda), dev(taps_np, cuda)
    more = 0 if mode == "fm" else -1     # (FM reads one FIR output past its last)
    whole = run_chain(cuda, mode, row, x, taps, D, n0, N)
    parts, m = [], 0
    for n in (7000, 1, 12345, N - 7000 - 1 - 12345):
        parts.append(run_chain(cuda, mode, row, x[m * D:(m + n + more) * D + T], taps, D, n0 + m * D, n))
        m += n
    assert m == N
    assert np.concatenate(parts).tobytes() == whole.tobytes()


@pytest.mark.parametrize("D", [3, 4])
@pytest.mark.parametrize("name", SPLIT_FREQS)
def test_fm_stream_equals_one_call(cuda, name, D):
    """The same through the streaming object, with chunk lengths that are not multiples of D."""
    from gsdr_amd import ops
    from gsdr_amd.stream import Stream

    row = FREQ_BY_NAME[name]
    _, fs, tune, chan, _ = row
    T, N, n0 = 127, 30000, 1000
    x_np, taps_np = inputs("fm", row, D, T, N, n0, seed=3)
    x, taps = dev(x_np, cuda), dev(taps_np, cuda)
    want = ops.fm_demod(x, taps, fs, tune, chan, deviation(fs), D, n0)
    s = Stream("fm", taps, D, fs, tune, chan, deviation(fs), first_sample_index=n0)
    parts, pos = [], 0
    for m in (1, 125, 5003, 17003, 2, x.numel()):
        m = min(m, x.numel() - pos)
        assert m == x.numel() - pos or m % D != 0
        parts.append(s.process(x[pos:pos + m]).clone())
        pos += m
    s.close()
    got = torch.cat(parts)
    torch.cuda.synchronize()
    assert pos == x.numel() and want.numel() == N and got.numel() == N
    assert got.cpu().numpy().tobytes() == want.cpu().numpy().tobytes()
