"""GPU parity against the reference-run vectors (tests/golden/ref_*.npz): every entry point whose reference
kernel could be run (oracle/README.md) through gsdr_amd.ops, the C ABI, compared with what the reference's own
kernel text computed on the stored inputs -- not with the oracle. `contract` / `nocontract` are the two builds of
the reference (a * b + c contracted as nvcc does by default, or not). Only tests/golden is read.

Bars: those of the existing test of each op (named per test). "Bit-identical" is helpers.same_values: every bit,
the sign of a zero included, any NaN equal to any NaN.
"""
import numpy as np
import pytest
import torch

from helpers import (FLOAT_TOL, REF_BUILDS, bound, finite_elements, normwise_err, ref_pick, ref_vectors, same_specials,
                     same_values, wrapped_angle_err)

pytestmark = pytest.mark.gpu

FIR_DS, FIR_TS = (1, 3, 4), (1, 8, 63, 127)
TILE_CASES = {"fc": ("FC", 4, 127), "ff": ("FF", 1, 63)}
QPSK_STREAMS = (1, 2, 4, 8)


def dev(a, cuda):
    return torch.from_numpy(np.ascontiguousarray(a)).to(cuda)


def host(t):
    torch.cuda.synchronize()
    return t.cpu().numpy()


def amp_key(a):
    return ("%g" % a).replace(".", "p")


def assert_same_specials(got, want):
    """As test_gpu_nonfinite.assert_same_specials: NaN pattern, Inf pattern and signs, signs of the zeros."""
    assert same_specials(got, want), "NaN / Inf pattern"
    g = np.ascontiguousarray(got).view(np.float32)
    w = np.ascontiguousarray(want).view(np.float32)
    z = w == 0
    assert np.all(g[z] == 0) and np.array_equal(np.signbit(g[z]), np.signbit(w[z])), "zero signs"


def fir_cases(tt):
    g = ref_vectors(f"ref_fir_{tt}")
    N = int(g["N"])
    for D in FIR_DS:
        for T in FIR_TS:
            yield g, f"D{D} T{T}", g[f"taps_T{T}"], g["x"][:(N - 1) * D + T], D, N, f"y_D{D}_T{T}"
    D, T = (int(v) for v in g["special_DT"])
    yield g, f"specials D{D} T{T}", g[f"taps_T{T}"], g["xs"], D, N, "ys"
    t = ref_vectors("ref_fir_tiles")
    for key, (ttype, D, T) in TILE_CASES.items():
        if ttype == tt:
            yield t, f"tile D{D} T{T}", t[f"{key}_taps"], t[f"{key}_x"], D, int(t["N"]), f"{key}_y"


@pytest.mark.parametrize("tt", ["FF", "FC", "CC", "CF"])
def test_fir_vs_reference_run(cuda, tt):
    """gsdrFirFF / FC / CC / CF against fir.cu k_Fir (D = 1) and k_FirDecimate: FLOAT_TOL normwise with
    helpers.bound against both builds (the summation order is free on the GPU); on the +-0 / Inf / NaN samples
    the non-finite pattern and the zero signs of test_gpu_nonfinite.assert_same_specials."""
    from gsdr_amd import ops

    count = 0
    for g, label, taps, x, D, N, name in fir_cases(tt):
        y = host(ops.fir(dev(taps, cuda), dev(x, cuda), D, N))
        s = bound(taps, x, D, N)
        for b in REF_BUILDS:
            want = ref_pick(g, name, b)
            assert y.dtype == want.dtype and y.shape == want.shape
            assert_same_specials(y, want)
            ok = finite_elements(want)
            assert ok.sum() > N // 2
            assert normwise_err(y[ok], want[ok], s[ok]) <= FLOAT_TOL, (tt, label, b)
        count += 1
    assert count >= len(FIR_DS) * len(FIR_TS) + 1


def test_quad_fm_vs_reference_run(cuda):
    """gsdrQuadFmDemod against quad_demod.cu k_quadFmDemod: the discriminator bar of test_gpu_elementwise,
    helpers.wrapped_angle_err <= 1e-5, on the finite outputs of both builds; the same NaN pattern."""
    from gsdr_amd import ops

    g = ref_vectors("ref_quad")
    gain = float(g["gain"])
    got = host(ops.quad_fm_demod(dev(g["x"], cuda), gain))
    for b in REF_BUILDS:
        want = ref_pick(g, "fm", b)
        ok = np.isfinite(want)
        assert np.array_equal(np.isnan(got), np.isnan(want)) and 0 < ok.sum() < ok.size
        assert wrapped_angle_err(got[ok], want[ok], gain) <= FLOAT_TOL, b


def test_quad_am_and_magnitude_vs_reference_run(cuda):
    """gsdrQuadAmDemod / gsdrMagnitude against k_quadAmDemod / k_Magnitude: the bars of
    test_gpu_elementwise.test_quad_am_and_magnitude_parity (FLOAT_TOL absolute, FLOAT_TOL relative), with the
    clamp at |x| > 1, NaN -> -1 and the Inf / NaN magnitudes in place."""
    from gsdr_amd import ops

    g = ref_vectors("ref_quad")
    x = g["x"][:g["am"].size]
    xt = dev(x, cuda)
    am, mag = host(ops.quad_am_demod(xt)), host(ops.magnitude(xt))
    assert np.count_nonzero(np.abs(x) > 1) > 100 and np.isnan(x.view(np.float32)).any()
    assert np.all(np.isfinite(g["am"])) and np.max(np.abs(am - g["am"])) <= FLOAT_TOL
    want = g["mag"]
    assert same_specials(mag, want)
    ok = np.isfinite(want)
    assert np.max(np.abs(mag[ok] - want[ok]) / np.maximum(want[ok], 1e-30)) <= FLOAT_TOL


def test_add_const_abs_bit_identical_to_reference_run(cuda):
    """gsdrAddConstFF / CC / CF / FC and gsdrAbs, compared bit for bit as in test_gpu_arith."""
    from gsdr_amd import ops

    g = ref_vectors("ref_add")
    x, xc, cf, cc = g["x"], g["xc"], float(g["cf"]), complex(g["cc"])
    for name, inp, c in (("add_ff", x, cf), ("add_cc", xc, cc), ("add_cf", xc, cf), ("add_fc", x, cc)):
        assert same_values(host(ops.add_const(dev(inp, cuda), c)), ref_pick(g, name, "nocontract")) == 0, name
    assert same_values(host(ops.abs_(dev(x, cuda))), ref_pick(g, "abs", "nocontract")) == 0


def test_add_to_magnitude_vs_reference_run(cuda):
    """gsdrAddToMagnitude against k_AddToMagnitude: the bar of test_gpu_arith.test_add_to_magnitude (1e-6
    relative) on the finite outputs, NaN where the reference gives NaN (a zero or infinite sample)."""
    from gsdr_amd import ops

    g = ref_vectors("ref_add")
    got = host(ops.add_to_magnitude(dev(g["xc"], cuda), float(g["a2m_c"])))
    for b in REF_BUILDS:
        want = ref_pick(g, "a2m", b)
        assert same_specials(got, want)
        ok = finite_elements(want)
        assert np.max(np.abs(got[ok] - want[ok]) / np.abs(want[ok])) < 1e-6, b


def test_multiply_bit_identical_to_uncontracted_reference_run(cuda):
    """gsdrMultiplyCC / FF / CF, bit for bit as in test_gpu_arith, with the build that rounds every product."""
    from gsdr_amd import ops

    g = ref_vectors("ref_multiply")
    for name, p, q in (("mul_cc", g["xc"], g["yc"]), ("mul_ff", g["x"], g["y"]), ("mul_cf", g["xc"], g["y"])):
        got = host(ops.multiply(dev(p, cuda), dev(q, cuda)))
        assert same_values(got, ref_pick(g, name, "nocontract")) == 0, name


def test_int8_conversion_and_cosine_vs_reference_run(cuda):
    """gsdrInt8ToNormFloat bit for bit (all 256 values and random ones); gsdrCosineC / F within the 1e-6 of
    test_gpu_arith.test_cosine of the contracted build (the phase as one fmaf, as nvcc and the library form it);
    the uncontracted build's phase is up to one ulp of the largest phase away, and |cos a - cos b| <= |a - b|,
    so there the bar is 1e-6 plus that ulp (test_oracle_reference_vectors.test_cosine_oracle_vs_reference)."""
    from gsdr_amd import ops

    g = ref_vectors("ref_maps")
    assert same_values(host(ops.int8_to_norm_float(dev(g["i8"], cuda))), g["conv"]) == 0
    n, (phi0, phi1) = int(g["n"]), (float(v) for v in g["phi"])
    got_c = host(ops.cosine(phi0, phi1, n, complex_out=True, device=cuda))
    got_f = host(ops.cosine(phi0, phi1, n, complex_out=False, device=cuda))
    ulp = float(np.spacing(np.float32(max(abs(float(v)) for v in g["phi"]))))
    for b, bar in (("contract", 1e-6), ("nocontract", 1e-6 + ulp)):
        assert np.max(np.abs(got_c - ref_pick(g, "cos_c", b))) < bar, b
        assert np.max(np.abs(got_f - ref_pick(g, "cos_f", b))) < bar, b


@pytest.mark.parametrize("stem", ["ref_qpsk_lo", "ref_qpsk_hi"])
def test_qpsk_modulation_bit_identical_to_reference_run(cuda, stem):
    """gsdrQpskModulate, gsdrQpskModulate4x and gsdrQpskModulateTemplated with 1, 2, 4, 8 streams against
    k_QpskModulate, k_QpskModulate4x and k_QpskModulateTemplated<S>: 4,099 symbols, a partial last byte."""
    from gsdr_amd import ops

    g = ref_vectors(stem)
    n, bits = int(g["n"]), g["bits"]
    stride = n // 4 + 1
    bd = dev(bits, cuda)
    for a in (float(v) for v in g["amps"]):
        k = amp_key(a)
        assert same_values(host(ops.qpsk_modulate(bd[:stride], n, a)), g[f"mod_a{k}"]) == 0, a
        outs = [torch.empty(n, dtype=torch.complex64, device=cuda) for _ in range(4)]
        ops.qpsk_modulate_4x([bd[s * stride:(s + 1) * stride] for s in range(4)], outs, n, a)
        assert same_values(host(torch.stack(outs)), g[f"mod4x_a{k}"]) == 0, a
        for S in QPSK_STREAMS:
            out = torch.zeros(S * n, dtype=torch.complex64, device=cuda)
            ops.qpsk_modulate_templated(bd, out, n, a, S)
            assert same_values(host(out), g[f"tmpl{S}_a{k}"]) == 0, (a, S)


@pytest.mark.parametrize("stem,ctype", [("ref_qpsk256_rect", 0), ("ref_qpsk256_circ", 1)])
def test_qpsk256_tables_and_modulation_bit_identical_to_reference_run(cuda, stem, ctype):
    """gsdrQpsk256InitConstellation + gsdrQpsk256Modulate / 4x against k_InitQpsk256Rectangular / Circular +
    k_Qpsk256Modulate / 4x: the first 256 symbols are the byte values 0 .. 255, so every table entry shows."""
    from gsdr_amd import ops

    g = ref_vectors(stem)
    syms = g["syms"]
    assert np.array_equal(syms[:256], np.arange(256))
    for a in (float(v) for v in g["amps"]):
        k = amp_key(a)
        ops.qpsk256_init(ctype, a)
        got = host(ops.qpsk256_modulate(dev(syms, cuda), ctype, a))
        assert same_values(got[:256], g[f"table_a{k}"]) == 0, a
        assert same_values(got, g[f"mod_a{k}"]) == 0, a
        n4 = g["syms4"].shape[1]
        outs = [torch.empty(n4, dtype=torch.complex64, device=cuda) for _ in range(4)]
        ops.qpsk256_modulate_4x([dev(s, cuda) for s in g["syms4"]], outs, n4, ctype, a)
        assert same_values(host(torch.stack(outs)), g[f"mod4x_a{k}"]) == 0, a
