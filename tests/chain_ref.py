"""Reference for the chains' frequency tests (gsdrFmDemod, gsdrAmDemod, gsdrxXlatingFir); a helper, not a test module.

    inc    = round_half_away(trunc_mod(((float32)(tune - chan) / fs) 2^32, 2^32)) mod 2^32
    P(n)   = (n0 + n) inc mod 2^32                                  (exact integers)
    y[m]   = sum_i taps[i] x[m D + i] exp(2 pi j P(m D + i) / 2^32)  (float64 / complex128)
    fm[m]  = g arg(y[m + 1] conj y[m]),  g = fs / (2 pi dev) in float32
    am[m]  = 2 clip(|y[m]|, 0, 1) - 1

test_nco_increment.py ties it to the project's oracle at every row of FREQS. FREQS holds the NCO increments that
are special to this implementation (gsdr_amd/csrc/fir_nco.hpp nco_direct, stage_anchored's row factor F,
fir_i8_mfma.hpp's left-out rotation dphi); `inputs` builds the signals both test files feed the chains."""
from fractions import Fraction

import numpy as np

TWO32 = 1 << 32

# (name, fs, tune, chan, expected increment). What each row meets:
#   zero                 every phasor exactly 1
#   step_up / step_down  increment +-1: phases a few ulps of the float conversion from 0
#   nyquist(_pos)        (int32)0x80000000 = -0.5 revolutions, from a negative and a positive difference
#   below / above_nyquist  the closest a float32 difference comes to +-fs/2
#   (minus_)quarter      the cosine of every odd sample exactly 0
#   (minus_)eighth       the int8 chain's 4 inc = 2^31: its left-out rotation sits at the wrap point -pi
#   f_one_wg256/128/64   the anchored chain's row factor F = E(2 WG inc) exactly 1 at that workgroup size
#   alias                |tune - chan| > fs: the fmod branch
#   tuned                tune != 0, a float-rounded difference
#   third, positive, audio  ordinary increments, a positive difference, another sample rate
FREQS = [
    ("zero", 1.0e6, 1.0e5, 1.0e5, 0x00000000),
    ("step_up", 2.0 ** 24, 0.0, -2.0 ** -8, 0x00000001),
    ("step_down", 2.0 ** 24, 0.0, 2.0 ** -8, 0xFFFFFFFF),
    ("nyquist", 1.0e6, 0.0, 5.0e5, 0x80000000),
    ("nyquist_pos", 1.0e6, 5.0e5, 0.0, 0x80000000),
    ("below_nyquist", 2.0 ** 24, 0.0, -8388607.5, 0x7FFFFF80),
    ("above_nyquist", 2.0 ** 24, 0.0, 8388607.5, 0x80000080),
    ("quarter", 1.0e6, 0.0, -2.5e5, 0x40000000),
    ("minus_quarter", 1.0e6, 0.0, 2.5e5, 0xC0000000),
    ("eighth", 1.0e6, 0.0, -1.25e5, 0x20000000),
    ("minus_eighth", 1.0e6, 0.0, 1.25e5, 0xE0000000),
    ("f_one_wg256", 2.0 ** 20, 0.0, -2048.0, 0x00800000),
    ("f_one_wg128", 2.0 ** 20, 0.0, 4096.0, 0xFF000000),
    ("f_one_wg64", 2.0 ** 20, 0.0, -8192.0, 0x02000000),
    ("alias", 1.0e6, 0.0, -1.3e6, 0x4CCCCCCD),
    ("tuned", 2.4e6, 1.007e8, 1.0123e8, 0xC7777777),
    ("third", 1.0e6, 0.0, -1.0e6 / 3.0, 0x55555582),
    ("positive", 1.0e6, 4.7e5, 1.0e5, 0x5EB851EC),
    ("audio", 48000.0, 0.0, 1234.5, 0xF96A7EFA),
]
FREQ_BY_NAME = {row[0]: row for row in FREQS}
FREQ_IDS = [row[0] for row in FREQS]


def nco_inc_exact(fs, tune, chan):
    """The increment in exact arithmetic: the float32 difference, one double division, then rationals."""
    df = np.float32(tune) - np.float32(chan)
    turns = float(df) / float(np.float32(fs))             # the one rounded double operation
    scaled = Fraction(turns) * TWO32
    whole = abs(scaled) // TWO32                           # reduce toward zero (fmod keeps the dividend's sign)
    reduced = scaled - whole * TWO32 if scaled >= 0 else scaled + whole * TWO32
    mag = abs(reduced)
    r = mag.numerator // mag.denominator
    if mag - r >= Fraction(1, 2):                          # half away from zero
        r += 1
    return (r if reduced >= 0 else -r) % TWO32


def signed_inc(inc):
    """The increment as the int32 the kernels convert: in [-2^31, 2^31)."""
    return inc - TWO32 if inc >= 1 << 31 else inc


def fm_gain(fs, dev):
    """The discriminator gain in float32, as fm_gain() of test_gpu_chains.py (reference src/fm.cu:203)."""
    return float(np.float32(fs) / (np.float32(2.0) * np.float32(np.pi) * np.float32(dev)))


def nco_turns(n0, L, inc):
    """P(n) / 2^32 for n in [0, L): exact integers (uint64 products wrap mod 2^64, which keeps the low 32 bits)."""
    n = np.arange(L, dtype=np.uint64) + np.uint64(n0 % TWO32)
    p = (n * np.uint64(inc)) & np.uint64(TWO32 - 1)
    for k in (0, L // 2, L - 1):
        assert int(p[k]) == ((n0 + k) * inc) % TWO32
    return p.astype(np.float64) / 2.0 ** 32


def correlate_valid(z, taps, direct_limit=1 << 25):
    """np.correlate(z, taps, "valid") for real taps; past `direct_limit` products through a float64 FFT (error
    ~1e-15 of |taps|_2 |z|_2 / sqrt(len), far below anything compared here; test_nco_increment.py checks it against
    the direct sum)."""
    if z.size * taps.size <= direct_limit:
        return np.correlate(z, taps, "valid")
    n = 1 << int(z.size + taps.size - 1).bit_length()
    full = np.fft.ifft(np.fft.fft(z, n) * np.fft.fft(taps[::-1], n))
    return full[taps.size - 1:z.size]


def chain_fir64(x, taps, inc, D, n0, N):
    """np.correlate(z, taps, "valid")[::D][:N] with z = x exp(2 pi j P / 2^32) in complex128."""
    taps = np.asarray(taps, np.float64)
    L = (N - 1) * D + taps.size
    assert x.size >= L
    z = np.asarray(x[:L]).astype(np.complex128) * np.exp(2j * np.pi * nco_turns(n0, L, inc))
    return correlate_valid(z, taps)[::D][:N]


def bound64(x, taps, D, N):
    """helpers.bound (S_k = sum_i |t_i| |x_{kD+i}|) through correlate_valid: usable at thousands of taps."""
    taps = np.abs(np.asarray(taps, np.float64))
    L = (N - 1) * D + taps.size
    return np.real(correlate_valid(np.abs(np.asarray(x[:L]).astype(np.complex128)), taps))[::D][:N]


def fm64(x, taps, inc, fs, dev, D, n0, N):
    y = chain_fir64(x, taps, inc, D, n0, N + 1)
    return fm_gain(fs, dev) * np.angle(y[1:] * np.conj(y[:-1]))


def am64(x, taps, inc, D, n0, N):
    return 2.0 * np.clip(np.abs(chain_fir64(x, taps, inc, D, n0, N)), 0.0, 1.0) - 1.0


def deviation(fs):
    """The frequencyDeviation argument of the FM calls."""
    return 0.02 * fs


def inputs(mode, row, D, T, N, n0, seed=None):
    """(x complex64, taps float32) for mode "fm" / "am" / "iq" at FREQS row `row`. FM: a constant-envelope signal
    whose carrier the NCO moves to 0 Hz (an out-of-band channel would filter noise only, whose angles are
    ill-conditioned for any summation order), N + 1 FIR outputs' worth; AM / IQ: 0.7 uniform I/Q."""
    from gsdr_amd.signals import fm_test_signal, lowpass_taps, uniform_iq

    _, fs, _, _, inc = row
    seed = D * 131 + T if seed is None else seed
    if mode == "fm":
        x = fm_test_signal(N * D + T, fs=fs, carrier=-signed_inc(inc) / 2.0 ** 32, noise=0.05, seed=seed,
                           n0=n0 % (1 << 20))
    else:
        x = (0.7 * uniform_iq((N - 1) * D + T, seed=seed)).astype(np.complex64)
    return x, lowpass_taps(T, 0.1)


def to_int8(x):
    """The quantisation of test_chain_int8_mfma_parity: round(100 x) clipped to int8, interleaved I/Q."""
    return np.clip(np.round(np.stack([x.real, x.imag], 1).ravel() * 100), -128, 127).astype(np.int8)
