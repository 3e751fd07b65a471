"""CPU: the frequency-translating FIR's public surface (gsdr_ext.h gsdrxXlatingFir / Int8 / Multi, stream.h
GSDRX_STREAM_XLATE) -- declared, exported, bound, and its stream validating its arguments before any device work (the
entry points' own validation table: test_chain_host.py). No compute call is made here."""
import ctypes
import os
import re
import subprocess

import pytest

from test_abi import HIP_ERROR_INVALID_VALUE, declared_symbols

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

ENTRY_POINTS = {"gsdrxXlatingFir": 12, "gsdrxXlatingFirInt8": 12, "gsdrxXlatingFirMulti": 14}


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


def test_stream_kind_value():
    text = open(os.path.join(ROOT, "include", "gsdr", "stream.h")).read()
    kinds = {m.group(1): int(m.group(2)) for m in re.finditer(r"#define\s+GSDRX_STREAM_(\w+)\s+(\d+)", text)}
    assert kinds == {"FIR": 0, "FM": 1, "AM": 2, "XLATE": 4}  # 3 is unassigned (test_abi.py pins it as invalid)
    from gsdr_amd.stream import KINDS

    assert KINDS["xlate"] == 4 and 3 not in KINDS.values()


def test_stream_create_validation_without_device_work(abi):
    lib = abi.lib
    null = None
    dummy = ctypes.c_void_p(16)
    XLATE = 4
    h = ctypes.c_void_p()
    chans = (ctypes.c_float * 2)(1e5, 2e5)
    for fmt in (0, 1):
        assert lib.gsdrxStreamCreate(null, XLATE, fmt, 4, dummy, 127, 1e6, 0.0, 1e5, 1.0, 0, 0) == \
            HIP_ERROR_INVALID_VALUE
        assert lib.gsdrxStreamCreate(ctypes.byref(h), XLATE, fmt, 4, null, 127, 1e6, 0.0, 1e5, 1.0, 0, 0) == \
            HIP_ERROR_INVALID_VALUE
        assert h.value is None
        # the deviations may be null for this kind: the null taps / handle are what is rejected
        assert lib.gsdrxStreamCreateMulti(null, XLATE, fmt, 4, dummy, 127, 1e6, 0.0, chans, null, 2, 0, 0) == \
            HIP_ERROR_INVALID_VALUE
        assert lib.gsdrxStreamCreateMulti(ctypes.byref(h), XLATE, fmt, 4, null, 127, 1e6, 0.0, chans, null, 2, 0,
                                          0) == HIP_ERROR_INVALID_VALUE
        assert h.value is None


def test_ops_entry_points_are_callable(abi):
    from gsdr_amd import ops

    assert callable(ops.xlating_fir) and callable(ops.xlating_fir_multi)
    assert "xlating_fir" in ops.__all__ and "xlating_fir_multi" in ops.__all__
