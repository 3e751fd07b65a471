"""CPU: the rational resampler's public surface (gsdr_ext.h gsdrxResampleFF / FC / InputsFor) -- declared, exported,
bound, validating its arguments before any device work -- and the tests' float64 reference (resample_ref.py) tied
to the project's oracle: it is oracle.fir with decimation M over the zero-stuffed input. No compute call is made
on a device here. (The reference-against-oracle cases exercise only resample_ref.py and the oracle, so they alone
among the resampler's tests do not depend on the library's new symbols.)"""
import ctypes
import subprocess

import numpy as np
import pytest

from helpers import normwise_err_strict
from resample_ref import inputs_for, resample_bound, resample_ref, zero_stuff
from test_abi import HIP_ERROR_INVALID_VALUE, HIP_SUCCESS, declared_symbols

ENTRY_POINTS = {"gsdrxResampleFF": 10, "gsdrxResampleFC": 10, "gsdrxResampleInputsFor": 5}


@pytest.fixture(scope="module")
def abi():
    from gsdr_amd import abi

    return abi


def test_headers_declare_and_library_exports_the_entry_points(abi):
    names = declared_symbols()
    out = subprocess.run(["nm", "-D", "--defined-only", abi.LIB_PATH], capture_output=True, text=True,
                         check=True).stdout
    exported = {line.split()[-1] for line in out.splitlines() if " T " in line}
    for name, nargs in ENTRY_POINTS.items():
        assert names.get(name) == nargs, name
        assert name in exported, name
        assert len(abi.SIGNATURES[name][1]) == nargs, name


def test_validation_without_device_work(abi):
    lib = abi.lib
    null = None
    dummy = ctypes.c_void_p(16)
    big = (1 << 64) - 1
    for fn in (lib.gsdrxResampleFF, lib.gsdrxResampleFC):
        # nothing to do: success whatever the other arguments are
        assert fn(0, 0, 5, null, 127, null, null, 0, 0, null) == HIP_SUCCESS
        assert fn(3, 2, 0, null, 31, null, null, 0, 0, null) == HIP_SUCCESS
        bad = [
            (0, 2, 0, dummy, 31, dummy, dummy, 16),            # interpolation == 0
            (3, 0, 0, dummy, 31, dummy, dummy, 16),            # decimation == 0
            (3, 2, 3, dummy, 31, dummy, dummy, 16),            # phase >= interpolation
            (3, 2, 7, dummy, 31, dummy, dummy, 16),
            (1, 2, 1, dummy, 31, dummy, dummy, 16),            # ... also on the path that forwards to the FIR
            (3, 2, 0, dummy, 31, null, dummy, 16),             # null input
            (3, 2, 0, dummy, 31, dummy, null, 16),             # null output
            (3, 2, 0, null, 31, dummy, dummy, 16),             # null taps with numTaps > 0
            (1, 2, 0, null, 31, dummy, dummy, 16),
            (1, 2, 0, dummy, 31, null, dummy, 16),
            (3, 2, 0, dummy, 0, null, dummy, 16),              # null input, no taps
            (3, 2, 0, dummy, 0, dummy, null, 16),
            (3, 1 << 31, 0, dummy, 31, dummy, dummy, 1 << 33),  # (numOutputs - 1) * decimation >= 2^63
            (3, 2, 2, dummy, big, dummy, dummy, 16),           # ... + numTaps wraps
            (3, 2, 2, dummy, (1 << 63) - 32, dummy, dummy, 16),  # the sum is exactly 2^63
            (3, 1, 0, dummy, 1, dummy, dummy, 1 << 63),        # 2^63 - 1 + 1
            (3, 2, 0, dummy, 31, dummy, dummy, 1 << 35),       # more workgroups than one launch takes
        ]
        for args in bad:
            assert fn(*args, 0, null) == HIP_ERROR_INVALID_VALUE, args


def test_inputs_for_matches_the_formula(abi):
    f = abi.lib.gsdrxResampleInputsFor
    shapes = [(1, 1), (1, 4), (2, 1), (4, 1), (3, 2), (2, 3), (5, 6), (24, 125), (125, 24), (147, 160), (160, 147),
              (7, 3), (2, 100001), (3, 4000000), (4096, 4099), ((1 << 32) - 1, (1 << 32) - 1)]
    for L, M in shapes:
        for T in {1, 2, max(1, L - 1), L, L + 1, 4 * L + 3, 16 * L}:   # T < L, T = 1 included
            for q in {0, L // 2, L - 1}:
                for N in (1, 2, 3, 1000, (1 << 20) + 1024):
                    want = (q + (N - 1) * M + T - 1) // L + 1
                    assert f(L, M, q, T, N) == want == inputs_for(L, M, q, T, N), (L, M, T, q, N)
    # no outputs, or arguments the calls reject
    assert f(3, 2, 0, 31, 0) == 0
    assert f(0, 2, 0, 31, 16) == 0 and f(3, 0, 0, 31, 16) == 0 and f(3, 2, 3, 31, 16) == 0
    assert f(3, 1 << 31, 0, 31, 1 << 33) == 0 and f(3, 2, 2, (1 << 63) - 32, 16) == 0
    assert f(3, 2, 2, (1 << 63) - 33, 16) == ((1 << 63) - 2) // 3 + 1   # the largest extent, 2^63 - 1
    # no taps: the same formula, and nothing at all when nothing is spanned
    assert f(3, 2, 1, 0, 5) == (1 + 8 - 1) // 3 + 1 and f(3, 2, 0, 0, 1) == 0


def test_ops_names_are_present(abi):
    from gsdr_amd import ops

    assert callable(ops.resample) and callable(ops.resample_inputs_for)
    assert "resample" in ops.__all__ and "resample_inputs_for" in ops.__all__
    assert ops.resample_inputs_for(24, 125, 7, 383, 100) == inputs_for(24, 125, 7, 383, 100)
    # arguments the C types cannot hold are rejected like the others: 0, no exception
    for args in [(1 << 32, 2, 0, 31, 16), (3, 1 << 32, 0, 31, 16), (3, 2, 0, 1 << 64, 16), (3, 2, 0, 31, 1 << 64),
                 (3, 2, -1, 31, 16), (3, 2, 0, 31, -1)]:
        assert ops.resample_inputs_for(*args) == 0, args


#            L    M    T     q    complex
SHAPES = [(24, 125, 383, 7, True), (3, 2, 31, 1, False), (147, 160, 1769, 100, False), (5, 1, 23, 3, False),
          (7, 3, 5, 2, False)]


@pytest.mark.parametrize("L,M,T,q,cplx", SHAPES)
def test_reference_is_the_oracle_fir_over_the_zero_stuffed_input(L, M, T, q, cplx):
    from oracle import oracle as orc

    N = 500
    rng = np.random.default_rng(L * 1000 + M)
    need = inputs_for(L, M, q, T, N)
    x = rng.uniform(-1, 1, need).astype(np.float32)
    if cplx:
        x = (x + 1j * rng.uniform(-1, 1, need).astype(np.float32)).astype(np.complex64)
    h = rng.uniform(-1, 1, T).astype(np.float32)
    u = zero_stuff(x, L)
    assert u.size >= q + (N - 1) * M + T   # the input count covers every window
    assert (need - 1) * L < q + (N - 1) * M + T   # ... and its last sample is inside the last window
    want = orc.fir(h, u[q:], M, N)
    got = resample_ref(h, x, L, M, q, N)
    s = resample_bound(h, x, L, M, q, N)
    assert normwise_err_strict(got, want, s) <= 1e-5
    if T < L:   # empty windows: exactly zero in both, and there are some
        empty = s == 0
        assert empty.any() and not empty.all()
        assert np.all(got[empty] == 0) and np.all(np.asarray(want)[empty] == 0)
    # a block of the stream computed on its own (m0) equals that block of the whole
    assert np.array_equal(resample_ref(h, x, L, M, q, 100, m0=250), got[250:350])
