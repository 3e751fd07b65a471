"""CPU: every chain entry point (FM, AM and the frequency-translating FIR; complex float, int8 I/Q and multi-channel)
validates its arguments before any device work, and accepts empty work whatever the other arguments are. One fault
per row; no compute call is made here."""
import ctypes

import pytest

from test_abi import HIP_ERROR_INVALID_VALUE, HIP_SUCCESS

NULL = None
DUMMY = ctypes.c_void_p(16)
INF, NAN = float("inf"), float("nan")

# entry point -> takes a frequency deviation (FM)
SINGLE = {"gsdrFmDemod": True, "gsdrxFmDemodInt8": True, "gsdrAmDemod": False, "gsdrxAmDemodInt8": False,
          "gsdrxXlatingFir": False, "gsdrxXlatingFirInt8": False}
MULTI = {"gsdrxFmDemodMulti": True, "gsdrxAmDemodMulti": False, "gsdrxXlatingFirMulti": False}

# what every entry point rejects, one fault per row
COMMON_FAULTS = [
    dict(D=0),
    dict(inp=NULL),
    dict(out=NULL),
    dict(taps=NULL),                 # with numTaps > 0
    dict(fs=0.0), dict(fs=-1e6),     # sample rate not positive
    dict(fs=INF), dict(fs=NAN),      # ... or not finite
    dict(tune=INF), dict(tune=NAN),  # frequency difference not finite
]


@pytest.fixture(scope="module")
def lib():
    from gsdr_amd import abi

    return abi.lib


def call_single(fn, fm, **kw):
    a = dict(fs=1e6, tune=0.0, chan=1e5, dev=2e4, D=4, first=0, taps=DUMMY, T=127, inp=DUMMY, out=DUMMY, n=16)
    a.update(kw)
    dev = (a["dev"],) if fm else ()
    return fn(a["fs"], a["tune"], a["chan"], *dev, a["D"], a["first"], a["taps"], a["T"], a["inp"], a["out"], a["n"],
              0, NULL)


def call_multi(fn, fm, **kw):
    a = dict(fs=1e6, tune=0.0, chans=(ctypes.c_float * 2)(1e5, 2e5), devs=(ctypes.c_float * 2)(2e4, 3e4), C=2, D=4,
             first=0, taps=DUMMY, T=127, fmt=0, inp=DUMMY, out=DUMMY, n=16)
    a.update(kw)
    devs = (a["devs"],) if fm else ()
    return fn(a["fs"], a["tune"], a["chans"], *devs, a["C"], a["D"], a["first"], a["taps"], a["T"], a["fmt"],
              a["inp"], a["out"], a["n"], 0, NULL)


def test_validation_without_device_work(lib):
    nothing = dict(taps=NULL, inp=NULL, out=NULL)
    for name, fm in SINGLE.items():
        fn = getattr(lib, name)
        # nothing to do: success whatever the other arguments are
        assert call_single(fn, fm, n=0, **nothing) == HIP_SUCCESS, name
        faults = COMMON_FAULTS + [dict(chan=INF), dict(chan=NAN), dict(tune=INF, chan=INF)]
        for fault in faults:
            assert call_single(fn, fm, **fault) == HIP_ERROR_INVALID_VALUE, (name, fault)
    for name, fm in MULTI.items():
        fn = getattr(lib, name)
        assert call_multi(fn, fm, n=0, **nothing) == HIP_SUCCESS, name                         # numOutputs == 0
        assert call_multi(fn, fm, n=0, chans=NULL, devs=NULL, **nothing) == HIP_SUCCESS, name
        assert call_multi(fn, fm, C=0, chans=NULL, devs=NULL, **nothing) == HIP_SUCCESS, name  # numChannels == 0
        assert call_multi(fn, fm, C=0) == HIP_SUCCESS, name
        assert call_multi(fn, fm, C=0, fmt=1) == HIP_SUCCESS, name
        faults = COMMON_FAULTS + [
            dict(chans=NULL),
            dict(fmt=2), dict(fmt=7), dict(fmt=-1),  # unknown sample formats
            dict(fmt=1, D=0), dict(fmt=1, inp=NULL), dict(fmt=1, out=NULL), dict(fmt=1, taps=NULL),
            dict(fmt=1, fs=0.0), dict(fmt=1, tune=NAN),
            # one channel of the array not finite
            dict(chans=(ctypes.c_float * 2)(1e5, INF)), dict(chans=(ctypes.c_float * 2)(NAN, 2e5)),
            dict(fmt=1, chans=(ctypes.c_float * 2)(1e5, NAN)),
        ]
        if fm:
            faults.append(dict(devs=NULL))
        for fault in faults:
            assert call_multi(fn, fm, **fault) == HIP_ERROR_INVALID_VALUE, (name, fault)
