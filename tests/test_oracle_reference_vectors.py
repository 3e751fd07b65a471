"""CPU: the C oracle and the float64 restatement of make_golden.py against the reference-run vectors
(tests/golden/ref_*.npz): what the reference's OWN kernel text computes, compiled for the host by
oracle/refhost/ with (`contract`) and without (`nocontract`) contraction of a * b + c. The oracle and
make_golden.py are two restatements this project wrote from one reading of the reference; these vectors are
the reference itself, so a misreading (tap orientation, operand order, a conjugate, a clamp, a bit order, a
table entry) fails here.

"Bit-identical" below is helpers.same_values: every bit, the sign of a zero included, with any NaN equal to
any NaN (IEEE 754 leaves a produced NaN's sign and payload open).
"""
import hashlib
import importlib.util
import json
import os

import numpy as np
import pytest

from helpers import (FLOAT_TOL, REF_BUILDS, finite_elements, normwise_err, ref_pick, ref_vectors, same_specials,
                     same_values, wrapped_angle_err)
from oracle import oracle as o

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def _module(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(GOLD, name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


gen = _module("make_reference_vectors")
golden = _module("make_golden")
STEMS = sorted(gen.FILES)
FIR_GRID = [(D, T) for D in gen.FIR_DS for T in gen.FIR_TS]


def outputs_of(g):
    prov = json.loads(str(g["provenance"]))
    return prov, [k for k in g.files if k.split("__")[0] in prov]


# ------------------------------------------------------------------------------------------ the files

def test_inventory_and_size_budget():
    """Every file of the generator is committed, within 100 KB each and 700 KB together, and records where each
    output came from, the reference files' hashes and the compile flags of both builds."""
    total = 0
    for stem in STEMS:
        size = os.path.getsize(os.path.join(GOLD, stem + ".npz"))
        assert size <= 100_000, stem
        total += size
        g = ref_vectors(stem)
        prov, stored = outputs_of(g)
        assert prov and {k.split("__")[0] for k in stored} == set(prov), stem
        for name, where in prov.items():
            assert where.startswith("src/") and ".cu:k_" in where, (stem, name, where)
            assert (name in g.files) != all(f"{name}__{b}" in g.files for b in REF_BUILDS), (stem, name)
        sha, flags = json.loads(str(g["reference_sha256"])), json.loads(str(g["flags"]))
        assert all(len(v) == 64 for v in sha.values()) and {w.split(":")[0] for w in prov.values()} <= set(sha)
        assert "-ffp-contract=fast" in flags["contract"] and "-ffp-contract=off" in flags["nocontract"]
    assert total <= 700_000
    committed = {f[:-4] for f in os.listdir(GOLD) if f.startswith("ref_") and f.endswith(".npz")}
    assert committed == set(STEMS)


@pytest.mark.skipif(not gen.available(), reason="oracle/_ref is not built here (no reference or CUDA headers)")
@pytest.mark.parametrize("stem", STEMS)
def test_provenance_fresh_run_reproduces_the_vectors(stem):
    """Where the reference-run libraries exist, running them on the stored inputs gives every stored output
    array byte for byte, under the same names (so the same split into builds that agree and differ), from the
    recorded flags and, where the reference itself is readable, from files with the recorded hashes."""
    g = ref_vectors(stem)
    prov, stored = outputs_of(g)
    inputs = {k: g[k] for k in g.files if k not in stored and k not in gen.META}
    fresh, fresh_prov = gen.outputs(stem, inputs)
    assert fresh_prov == prov
    assert sorted(fresh) == sorted(stored)
    for name in stored:
        want = g[name]
        assert fresh[name].dtype == want.dtype and fresh[name].shape == want.shape, name
        assert fresh[name].tobytes() == want.tobytes(), name
    m = gen.manifest()
    assert m["flags"] == json.loads(str(g["flags"]))
    recorded = json.loads(str(g["reference_sha256"]))
    assert m["reference_sha256"] == recorded
    root = os.environ.get("GSDR_REFERENCE_DIR", "/root/reference")
    for rel, digest in recorded.items():
        path = os.path.join(root, rel)
        if os.access(path, os.R_OK):
            with open(path, "rb") as f:
                assert hashlib.sha256(f.read()).hexdigest() == digest, rel


# ------------------------------------------------------------------------------------------------ FIR

def fir_cases(tt):
    """(label, taps, x, D, N, output name) of every case of one type: the grid and the special-sample case."""
    g = ref_vectors(f"ref_fir_{tt}")
    N = int(g["N"])
    for D, T in FIR_GRID:
        yield g, f"D{D} T{T}", g[f"taps_T{T}"], g["x"][:(N - 1) * D + T], D, N, f"y_D{D}_T{T}"
    D, T = (int(v) for v in g["special_DT"])
    yield g, f"specials D{D} T{T}", g[f"taps_T{T}"], g["xs"], D, N, "ys"


def tile_cases():
    g = ref_vectors("ref_fir_tiles")
    for key, (tt, D, T) in gen.TILE_CASES.items():
        yield tt, g, f"tile {tt} D{D} T{T}", g[f"{key}_taps"], g[f"{key}_x"], D, int(g["N"]), f"{key}_y"


@pytest.mark.parametrize("tt", ["FF", "FC", "CF"])
def test_fir_oracle_bit_identical_to_contracted_reference(tt):
    """fir.cu k_Fir / k_FirDecimate as nvcc builds them (a * b + c contracted): one fmaf per component, taps
    ascending from a zero accumulator -- the oracle's documented order, so every bit agrees, at every D and T,
    on +-0 / Inf / NaN samples and across a 1,024-output tile."""
    cases = list(fir_cases(tt)) + [c[1:] for c in tile_cases() if c[0] == tt]
    assert len(cases) >= len(FIR_GRID) + 1
    for g, label, taps, x, D, N, name in cases:
        assert same_values(o.fir(taps, x, D, N), ref_pick(g, name, "contract")) == 0, (tt, label)


def _f64(taps, x, D, N):
    return golden.fir64(taps, x, D, N), golden.bound64(taps, x, D, N)



def test_fir_cc_oracle_within_twice_the_reference_builds_own_error():
    """FIR CC is not bit-identical to either build: the oracle chains one fmaf per real product, the reference
    forms the cuCmulf expression (cuComplexOperatorOverloads.cuh:25-27) and then adds (:57-62). All three are
    roundings of one T-term sum in one order, so their errors have one distribution: the oracle's normwise
    distance from the float64 value of the stored inputs may be at most twice the larger of the two builds'
    distances on the same case. Measured values: DESIGN.md section 4."""
    for g, label, taps, x, D, N, name in fir_cases("CC"):
        refs = [ref_pick(g, name, b) for b in REF_BUILDS]
        ok = finite_elements(refs[0])
        with np.errstate(invalid="ignore"):
            want, s = _f64(taps, x, D, N)
        assert ok.sum() > N // 2 and np.all(finite_elements(want[ok])), label
        y = o.fir(taps, x, D, N)
        for r in refs:
            assert same_specials(y, r), label
        d_oracle = normwise_err(y[ok], want[ok], s[ok])
        d_ref = [normwise_err(r[ok], want[ok], s[ok]) for r in refs]
        print(f"FIR CC {label}: oracle {d_oracle:.3e}, contract {d_ref[0]:.3e}, nocontract {d_ref[1]:.3e}, "
              f"oracle vs contract {normwise_err(y[ok], refs[0][ok], s[ok]):.3e}")
        assert d_oracle <= 2.0 * max(d_ref), label


@pytest.mark.parametrize("tt", ["FF", "FC", "CC", "CF"])
def test_golden_fir64_agrees_with_reference_run(tt):
    """The float64 restatement behind the older fixtures (make_golden.fir64) against the reference-run FIR
    vectors of both builds, within FLOAT_TOL normwise on every finite output: ties the FIR stage of the chain
    fixtures to the reference."""
    cases = list(fir_cases(tt)) + [c[1:] for c in tile_cases() if c[0] == tt]
    for g, label, taps, x, D, N, name in cases:
        with np.errstate(invalid="ignore"):
            want, s = _f64(taps, x, D, N)
        for b in REF_BUILDS:
            r = ref_pick(g, name, b)
            ok = finite_elements(r)   # fir64 multiplies in complex128, which makes NaN of Inf * (t + 0j): finite rows only
            assert ok.sum() > N // 2 and np.all(finite_elements(want[ok])), (label, b)
            assert normwise_err(r[ok], want[ok], s[ok]) <= FLOAT_TOL, (label, b)


def test_contraction_distance_of_the_reference_builds():
    """The two builds of fir.cu differ by roundings only: normwise within FLOAT_TOL of each other on every case
    (the measured distances are recorded in DESIGN.md section 4)."""
    worst = {}
    for tt in gen.FIR_TYPES:
        for g, label, taps, x, D, N, name in fir_cases(tt):
            a, b = (ref_pick(g, name, bld) for bld in REF_BUILDS)
            ok = finite_elements(a) & finite_elements(b)
            assert same_specials(a, b)
            worst[tt] = max(worst.get(tt, 0.0), normwise_err(a[ok], b[ok], golden.bound64(taps, x, D, N)[ok]))
    print("contract vs nocontract, worst normwise distance per type:", worst)
    assert max(worst.values()) <= FLOAT_TOL


# ------------------------------------------------------------------------ discriminators, element-wise

def close(got, want, bar, relative=False):
    """The non-finite pattern agrees and the finite elements are within `bar` (absolute, or relative to |want|)."""
    assert same_specials(got, want)
    ok = finite_elements(want)
    d = np.abs(got[ok].astype(np.complex128) - want[ok])
    if relative:
        d = d / np.maximum(np.abs(want[ok]), 1e-30)
    return float(np.max(d)) if d.size else 0.0


def test_quad_fm_oracle_vs_reference():
    """quad_demod.cu k_quadFmDemod (x[k+1] conj(x[k]), gain atan2f). Bit-identical to the uncontracted build:
    the oracle rounds each product of the conjugate multiply. Against the contracted build the atan2f argument
    moves by a rounding: the discriminator bar of the existing tests, helpers.wrapped_angle_err <= 1e-5."""
    g = ref_vectors("ref_quad")
    gain = float(g["gain"])
    fm = o.quad_fm(g["x"], gain)
    assert same_values(fm, g["fm__nocontract"]) == 0
    want = g["fm__contract"]
    ok = np.isfinite(want)
    assert same_specials(fm, want) and 0 < ok.sum() < ok.size
    assert wrapped_angle_err(fm[ok], want[ok], gain) <= FLOAT_TOL


def test_quad_am_and_magnitude_oracle_vs_reference():
    """k_quadAmDemod (2 saturate(hypotf) - 1: |x| > 1 clamps to 1, NaN to -1) and magnitude.cu k_Magnitude go
    through libm's hypotf: the bars of test_oracle_golden.test_quad_oracle_vs_golden, 1e-6 absolute for the
    envelope and 1e-6 relative for the magnitude."""
    g = ref_vectors("ref_quad")
    x = g["x"][:gen.EW_N]
    assert np.count_nonzero(np.abs(x) > 1) > 100   # the clamp is exercised
    assert close(o.quad_am(x), g["am"], 1e-6) <= 1e-6
    assert close(o.magnitude(x), g["mag"], 1e-6, relative=True) <= 1e-6


def test_add_const_abs_oracle_bit_identical():
    """add_const.cu k_AddConst in its four type combinations (CF adds to the real part only, FC yields the
    constant's imaginary part) and magnitude.cu k_Abs: no product, so both builds agree; bit-identical."""
    g = ref_vectors("ref_add")
    x, xc, cf, cc = g["x"], g["xc"], float(g["cf"]), complex(g["cc"])
    for name, got in (("add_ff", o.add_const(x, cf)), ("add_cc", o.add_const(xc, cc)), ("add_cf", o.add_const(xc, cf)),
                      ("add_fc", o.add_const(x, cc)), ("abs", o.abs_(x))):
        assert name in g.files, name   # the two builds agree
        assert same_values(got, g[name]) == 0, name


def test_add_to_magnitude_oracle_vs_reference():
    """k_AddToMagnitude divides by hypotf: the bar of test_gpu_arith.test_add_to_magnitude, 1e-6 relative; a zero
    sample gives NaN (0 / |0|) as in the reference."""
    g = ref_vectors("ref_add")
    got = o.add_to_magnitude(g["xc"], float(g["a2m_c"]))
    want = ref_pick(g, "a2m", "nocontract")
    assert np.all(np.isnan(want[:2].view(np.float32)))
    for b in REF_BUILDS:
        assert close(got, ref_pick(g, "a2m", b), 1e-6, relative=True) < 1e-6


def test_multiply_oracle_bit_identical_to_uncontracted_reference():
    """multiply.cu k_Multiply CC (cuCmulf), FF and CF: bit-identical to the uncontracted build, which is how the
    library and the oracle are built (-ffp-contract=off) and what test_gpu_arith compares bit for bit."""
    g = ref_vectors("ref_multiply")
    for name, got in (("mul_cc", o.multiply(g["xc"], g["yc"])), ("mul_ff", o.multiply(g["x"], g["y"])),
                      ("mul_cf", o.multiply(g["xc"], g["y"]))):
        assert same_values(got, ref_pick(g, name, "nocontract")) == 0, name


def test_int8_conversion_oracle_bit_identical():
    """conversion.cu k_int8ToFloat on all 256 values and random ones: max(-1, x / 127)."""
    g = ref_vectors("ref_maps")
    assert np.array_equal(g["i8"][:256], np.arange(-128, 128))
    assert same_values(o.int8_to_float(g["i8"]), g["conv"]) == 0


def test_cosine_oracle_vs_reference():
    """trig.cu k_ComplexCosine / k_RealCosine through libm's sincosf / cosf: the bar of
    test_gpu_arith.test_cosine, 1e-6 absolute, against the contracted build -- the phase phi + k * step as nvcc
    forms it, one fmaf, which the oracle and the library restate. The uncontracted build rounds k * step first, so
    its phase differs by up to one ulp of the largest phase (2^-18 = 3.8e-6 at |phase| in [32, 64)), and
    |cos a - cos b| <= |a - b|: there the bar is 1e-6 plus that ulp."""
    g = ref_vectors("ref_maps")
    n, (phi0, phi1) = int(g["n"]), g["phi"]
    ulp = float(np.spacing(np.float32(max(abs(float(phi0)), abs(float(phi1))))))
    for b, bar in (("contract", 1e-6), ("nocontract", 1e-6 + ulp)):
        d_c = float(np.max(np.abs(o.cosine(phi0, phi1, n, True) - ref_pick(g, "cos_c", b))))
        d_f = float(np.max(np.abs(o.cosine(phi0, phi1, n, False) - ref_pick(g, "cos_f", b))))
        print(f"cosine vs {b}: complex {d_c:.3e}, real {d_f:.3e} (bar {bar:.3e})")
        assert d_c < bar and d_f < bar, b


# ------------------------------------------------------------------------------------------ QPSK, QPSK256

@pytest.mark.parametrize("stem", ["ref_qpsk_lo", "ref_qpsk_hi"])
def test_qpsk_modulation_oracle_bit_identical(stem):
    """qpsk.cu k_QpskModulate, k_QpskModulate4x and k_QpskModulateTemplated<1, 2, 4, 8> at 4,099 symbols (a
    partial last byte) and amplitudes {0.5, 1, 2, 10}: symbol k is bit pair k & 3 of byte k >> 2, low pairs
    first; bit 0 negates I, bit 1 negates Q. Stream s of the consolidated layout starts at byte s (n / 4 + 1)."""
    g = ref_vectors(stem)
    n, bits = int(g["n"]), g["bits"]
    stride = n // 4 + 1
    assert n == 4099 and n % 4
    for a in (float(v) for v in g["amps"]):
        k = gen.amp_key(a)
        streams = [o.qpsk_mod(bits[s * stride:(s + 1) * stride], n, a) for s in range(8)]
        assert same_values(streams[0], g[f"mod_a{k}"]) == 0, a
        assert same_values(np.stack(streams[:4]), g[f"mod4x_a{k}"]) == 0, a
        for S in gen.QPSK_STREAMS:
            assert same_values(np.concatenate(streams[:S]), g[f"tmpl{S}_a{k}"]) == 0, (a, S)


@pytest.mark.parametrize("stem,ctype", [("ref_qpsk256_rect", 0), ("ref_qpsk256_circ", 1)])
def test_qpsk256_tables_and_modulation_oracle_bit_identical(stem, ctype):
    """qpsk256.cu k_InitQpsk256Rectangular / Circular at amplitudes {0.5, 1, 10}, and k_Qpsk256Modulate / 4x on
    all 256 byte values plus random ones: every table entry and every modulated symbol, bit for bit."""
    g = ref_vectors(stem)
    assert int(g["ctype"]) == ctype and np.array_equal(g["syms"][:256], np.arange(256))
    for a in (float(v) for v in g["amps"]):
        k = gen.amp_key(a)
        table = o.qpsk256_table(ctype, a)
        assert same_values(table, g[f"table_a{k}"]) == 0, a
        assert same_values(o.qpsk256_mod(table, g["syms"]), g[f"mod_a{k}"]) == 0, a
        assert same_values(np.stack([o.qpsk256_mod(table, s) for s in g["syms4"]]), g[f"mod4x_a{k}"]) == 0, a
