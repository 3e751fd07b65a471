"""CPU: the channelizer's public surface (gsdr_ext.h gsdrxChannelizer) -- declared, exported, bound, validating its
arguments before any device work -- and the tests' float64 reference (channelizer_ref.py) tied to the project's
oracle: row c is oracle.chain_fir with rfSampleRate = M, tuningFrequency = 0, channelFrequency = c. No compute call
is made on a device here. (The reference-against-oracle cases exercise only channelizer_ref.py and the oracle, so
they alone among the channelizer's tests do not depend on the library's new symbol.)"""
import ctypes
import subprocess

import numpy as np
import pytest

from channelizer_ref import channelizer_bound, channelizer_ref
from helpers import normwise_err_strict
from test_abi import HIP_ERROR_INVALID_VALUE, HIP_SUCCESS, declared_symbols

NAME, NARGS = "gsdrxChannelizer", 11
CF32, CS8 = 0, 1


@pytest.fixture(scope="module")
def abi():
    from gsdr_amd import abi

    return abi


def test_header_declares_and_library_exports_the_entry_point(abi):
    out = subprocess.run(["nm", "-D", "--defined-only", abi.LIB_PATH], capture_output=True, text=True,
                         check=True).stdout
    exported = {line.split()[-1] for line in out.splitlines() if " T " in line}
    assert declared_symbols().get(NAME) == NARGS
    assert NAME in exported
    assert len(abi.SIGNATURES[NAME][1]) == NARGS


def test_ops_name_is_present(abi):
    from gsdr_amd import ops

    assert callable(ops.channelizer) and "channelizer" in ops.__all__


def test_validation_without_device_work(abi):
    fn = abi.lib.gsdrxChannelizer
    null = None
    dummy = ctypes.c_void_p(16)
    big = (1 << 64) - 1
    # nothing to do: success whatever the other arguments are
    assert fn(0, 0, 5, null, 127, 7, null, null, 0, 0, null) == HIP_SUCCESS
    assert fn(12, 8, 0, null, 31, CF32, null, null, 0, 0, null) == HIP_SUCCESS
    assert fn(16, 8, 0, dummy, 31, CS8, dummy, dummy, 0, 0, null) == HIP_SUCCESS
    bad = [
        (0, 8, 0, dummy, 31, CF32, dummy, dummy, 16),             # a bad M
        (1, 1, 0, dummy, 31, CF32, dummy, dummy, 16),
        (3, 3, 0, dummy, 31, CF32, dummy, dummy, 16),
        (12, 6, 0, dummy, 31, CF32, dummy, dummy, 16),
        (128, 64, 0, dummy, 31, CF32, dummy, dummy, 16),
        (1 << 31, 8, 0, dummy, 31, CF32, dummy, dummy, 16),
        (16, 0, 0, dummy, 31, CF32, dummy, dummy, 16),            # D == 0
        (16, 8, 0, dummy, 31, CF32, null, dummy, 16),             # null input
        (16, 8, 0, dummy, 31, CS8, dummy, null, 16),              # null output
        (16, 8, 0, null, 31, CF32, dummy, dummy, 16),             # null taps with numTaps > 0
        (16, 8, 0, dummy, 0, CF32, null, dummy, 16),              # null input, no taps
        (16, 8, 0, dummy, 0, CF32, dummy, null, 16),
        (16, 8, 0, dummy, 31, 2, dummy, dummy, 16),               # an unknown format
        (16, 8, 0, dummy, 31, -1, dummy, dummy, 16),
        (16, 1 << 31, 0, dummy, 31, CF32, dummy, dummy, 1 << 33),  # (numOutputs - 1) * D >= 2^63
        (16, 8, 0, dummy, big, CF32, dummy, dummy, 16),           # ... + numTaps wraps
        (16, 8, 0, dummy, (1 << 63) - 120, CF32, dummy, dummy, 16),  # the sum is exactly 2^63
        (64, 1, 0, dummy, 1, CF32, dummy, dummy, 1 << 57),        # M * numOutputs is exactly 2^63
        (2, 1, 0, dummy, 1, CF32, dummy, dummy, 1 << 63),
        (16, 8, 0, dummy, 31, CF32, dummy, dummy, 1 << 35),       # more output times than one launch takes
        (16, 5, 0, dummy, 31, CS8, dummy, dummy, 1 << 35),        # ... on the generic route too
    ]
    for args in bad:
        assert fn(*args, 0, null) == HIP_ERROR_INVALID_VALUE, args


#          M   D    T    n0
SHAPES = [(4, 4, 33, 0), (16, 8, 127, 12345), (64, 48, 300, 7), (8, 3, 5, (1 << 32) + 5)]


@pytest.mark.parametrize("M,D,T,n0", SHAPES)
def test_reference_is_the_oracle_chain_fir_per_channel(M, D, T, n0):
    """Row c of the reference against oracle.chain_fir(fs = M, tune = 0, chan = c): the NCO increment c 2^32 / M is
    exact. Channels above M / 2 are named once as c and once as c - M (the same increment). Bar: the oracle's own
    fp32 bar, 1e-5 normwise."""
    from oracle import oracle as orc

    N = 300
    rng = np.random.default_rng(M * 1000 + D)
    need = (N - 1) * D + T
    x = (rng.uniform(-1, 1, need) + 1j * rng.uniform(-1, 1, need)).astype(np.complex64)
    h = rng.uniform(-1, 1, T).astype(np.float32)
    ref = channelizer_ref(h, x, M, D, n0, N)
    s = channelizer_bound(h, x, D, N)
    assert ref.shape == (M, N) and s.shape == (N,) and np.all(s > 0)
    for c in sorted({0, 1, M // 2, M - 1}):
        names = [c] if c <= M // 2 else [c, c - M]
        for chan in names:
            want = orc.chain_fir(x, h, float(M), 0.0, float(chan), D, n0, N)
            err = normwise_err_strict(ref[c], want, s)
            assert err <= 1e-5, (M, D, T, n0, c, chan, err)
    # a block of the stream computed on its own (m0) equals that block of the whole
    assert np.array_equal(channelizer_ref(h, x, M, D, n0, 100, m0=150), ref[:, 150:250])
