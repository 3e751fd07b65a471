"""CPU: gsdrNcoPhaseIncrement (pure host code: the library loads without a device) against the oracle and an exact
restatement, at the increments that are special to the kernels (chain_ref.FREQS) and on random triples; and the
float64 restatement of the chains (chain_ref.py) against the oracle, which is what lets test_gpu_chain_freq.py
compare long filters with float64 at the project's bar: the reference alone has to stay well inside it."""
import numpy as np
import pytest

from chain_ref import FREQ_IDS, FREQS, am64, chain_fir64, deviation, fm64, fm_gain, inputs, nco_inc_exact
from helpers import FLOAT_TOL, bound, normwise_err, wrapped_angle_err
from oracle import oracle as o

REF_SHARE = 0.3 * FLOAT_TOL   # the part of the bar the reference may use (measured: <= 7.2e-7)


@pytest.mark.parametrize("row", FREQS, ids=FREQ_IDS)
def test_increment_table(row):
    from gsdr_amd import ops

    _, fs, tune, chan, want = row
    got = (ops.nco_phase_increment(fs, tune, chan), o.nco_inc(fs, tune, chan), nco_inc_exact(fs, tune, chan))
    assert got == (want, want, want), [hex(v) for v in got]


def test_increment_random_triples():
    """|tune - chan| up to six sample rates (the fmod branch on both signs), tune itself up to 1e3 fs (a float-rounded
    difference), and exact multiples and halves of fs / 2^k."""
    from gsdr_amd import ops

    rng = np.random.default_rng(0x1C0)
    rates = (48.0e3, 2.4e5, 1.0e6, 2.4e6, 2.0 ** 24, 6.144e7)
    triples = []
    for k in range(1000):
        fs = rates[k % len(rates)]
        span = (0.5, 1.0, 3.0, 6.0)[(k // len(rates)) % 4]
        tune = float(rng.uniform(-span, span)) * fs * (1000.0 if k % 7 == 0 else 1.0)
        chan = tune + float(rng.uniform(-span, span)) * fs
        if k % 5 == 0:   # a difference that is an exact dyadic fraction of fs
            tune, chan = 0.0, fs * float(rng.integers(-6 * 64, 6 * 64 + 1)) / 64.0
        triples.append((fs, tune, chan))
    reached = max(abs(float(np.float32(t) - np.float32(c))) / fs for fs, t, c in triples)
    assert reached > 4.0
    seen = set()
    for fs, tune, chan in triples:
        a, b, c = ops.nco_phase_increment(fs, tune, chan), o.nco_inc(fs, tune, chan), nco_inc_exact(fs, tune, chan)
        assert a == b == c, (fs, tune, chan, hex(a), hex(b), hex(c))
        seen.add(a)
    assert len(seen) > 700


def test_fft_route_of_the_restatement_equals_the_direct_sum():
    """chain_ref.correlate_valid switches to an FFT for the long-filter cases: the same numbers to 1e-12."""
    from chain_ref import correlate_valid
    from gsdr_amd.signals import lowpass_taps, uniform_iq

    z = uniform_iq(20000, seed=9).astype(np.complex128)
    for T in (1, 2, 127, 2001):
        taps = lowpass_taps(T, 0.1).astype(np.float64)
        direct, fft = np.correlate(z, taps, "valid"), correlate_valid(z, taps, direct_limit=0)
        assert fft.shape == direct.shape and float(np.max(np.abs(fft - direct))) <= 1e-12


@pytest.mark.parametrize("D,T", [(1, 31), (4, 127), (64, 31)])
@pytest.mark.parametrize("row", FREQS, ids=FREQ_IDS)
def test_float64_restatement_agrees_with_the_oracle(row, D, T):
    """o.fm_demod, o.am_demod and o.chain_fir on the inputs of test_gpu_chain_freq.py against chain_ref, within 0.3 of
    the bar. A case that misses this has an ill-conditioned input: the margin is not the thing to move."""
    name, fs, tune, chan, inc = row
    N, n0 = 1500, 987654321 if D % 2 else (1 << 32) + 6
    x, taps = inputs("fm", row, D, T, N, n0)
    g = fm_gain(fs, deviation(fs))
    fm = wrapped_angle_err(o.fm_demod(x, taps, fs, tune, chan, deviation(fs), D, n0, N),
                           fm64(x, taps, inc, fs, deviation(fs), D, n0, N), g)
    x, taps = inputs("am", row, D, T, N, n0)
    am = float(np.max(np.abs(o.am_demod(x, taps, fs, tune, chan, D, n0, N) - am64(x, taps, inc, D, n0, N))))
    iq = normwise_err(o.chain_fir(x, taps, fs, tune, chan, D, n0, N), chain_fir64(x, taps, inc, D, n0, N),
                      bound(taps, x, D, N))
    print(f"{name} D={D} T={T}: oracle against float64: fm {fm:.2e} am {am:.2e} iq {iq:.2e} (share {REF_SHARE:.1e})")
    assert fm <= REF_SHARE and am <= REF_SHARE and iq <= REF_SHARE
