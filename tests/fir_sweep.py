"""The case tables of the FIR row sweep: every compile-time tile shape of the FIR engine (GSDR_FIR_ROWS,
gsdr_amd/csrc/fir_plan.hpp) and the runtime-decimation tile, each at its own tap-chunk and tile edges.

No GPU and no compiler here. test_fir_sweep_plan.py checks on the host that the table below is the header's and that
every launch listed here plans to the row it names; test_gpu_fir_rows.py (FIR mode) and test_gpu_chain_rows.py (FM,
AM, IQ) run the same grids on the GPU.

A row's chunk is ct taps (chunk * D for the polyphase rows, chunk for the contiguous-window rows), its tile
KT = WG * R outputs, and a mode's tiles start every S outputs. The tap counts are 1, 2 and 3 chunks, full and with a
last chunk of one tap; the output counts one output, one short of a tile, a tile, a tile plus one, and two tiles with
a ragged third.
"""
from collections import namedtuple

# fir_plan.hpp's enumerators (as tests/test_fir_plan.py spells them)
REAL_TAPS, COMPLEX_TAPS, ANY_TAPS = range(3)
REAL, COMPLEX, IQ8 = range(3)
FIR, FM, AM, IQ = range(4)
K_POLY, K_CONTIG = 0, 1
DEFAULT, SHORT, MULTI = 1, 2, 4

Row = namedtuple("Row", "name cls taps D kernel R chunk WG SUBS role")

# GSDR_FIR_ROWS, literally
ROWS = (
    Row("C1", 2, ANY_TAPS, 1, K_CONTIG, 8, 16, 256, 1, DEFAULT),
    Row("C2", 2, ANY_TAPS, 2, K_POLY, 8, 16, 128, 1, DEFAULT | MULTI),
    Row("C3", 2, ANY_TAPS, 3, K_CONTIG, 4, 24, 256, 1, DEFAULT),
    Row("C4", 2, ANY_TAPS, 4, K_POLY, 4, 16, 256, 1, DEFAULT | MULTI),
    Row("C4R2", 2, ANY_TAPS, 4, K_POLY, 2, 16, 256, 2, SHORT),
    Row("C4R1", 2, ANY_TAPS, 4, K_POLY, 1, 16, 256, 4, SHORT),
    Row("C5", 2, ANY_TAPS, 5, K_CONTIG, 4, 20, 128, 1, DEFAULT),
    Row("C6", 2, ANY_TAPS, 6, K_POLY, 2, 8, 256, 1, DEFAULT),
    Row("C7", 2, ANY_TAPS, 7, K_CONTIG, 4, 28, 128, 1, DEFAULT),
    Row("C8", 2, ANY_TAPS, 8, K_POLY, 2, 8, 256, 1, DEFAULT | MULTI),
    Row("C10", 2, ANY_TAPS, 10, K_POLY, 2, 8, 256, 1, DEFAULT),
    Row("C12", 2, ANY_TAPS, 12, K_POLY, 2, 8, 256, 1, DEFAULT),
    Row("C16", 2, ANY_TAPS, 16, K_POLY, 2, 8, 128, 1, DEFAULT),
    Row("C20", 2, ANY_TAPS, 20, K_POLY, 1, 8, 256, 1, DEFAULT),
    Row("C24", 2, ANY_TAPS, 24, K_POLY, 1, 8, 256, 1, DEFAULT),
    Row("C32", 2, ANY_TAPS, 32, K_POLY, 1, 8, 128, 1, DEFAULT),
    Row("C40", 2, ANY_TAPS, 40, K_POLY, 1, 8, 128, 1, DEFAULT),
    Row("C48", 2, ANY_TAPS, 48, K_POLY, 1, 8, 128, 1, DEFAULT),
    Row("C64", 2, ANY_TAPS, 64, K_POLY, 1, 8, 64, 1, DEFAULT),
    Row("R1", 4, REAL_TAPS, 1, K_CONTIG, 16, 32, 256, 1, DEFAULT),
    Row("R1C", 4, COMPLEX_TAPS, 1, K_CONTIG, 8, 16, 256, 1, DEFAULT),
    Row("R2", 4, ANY_TAPS, 2, K_CONTIG, 8, 16, 256, 1, DEFAULT),
    Row("R3", 4, ANY_TAPS, 3, K_CONTIG, 4, 36, 256, 1, DEFAULT),
    Row("R4", 4, ANY_TAPS, 4, K_POLY, 8, 8, 128, 1, DEFAULT),
    Row("R5", 4, ANY_TAPS, 5, K_CONTIG, 4, 40, 128, 1, DEFAULT),
    Row("R6", 4, ANY_TAPS, 6, K_CONTIG, 2, 36, 256, 1, DEFAULT),
    Row("R7", 4, ANY_TAPS, 7, K_CONTIG, 4, 28, 128, 1, DEFAULT),
    Row("R8", 4, ANY_TAPS, 8, K_POLY, 8, 8, 128, 1, DEFAULT),
    Row("R10", 4, ANY_TAPS, 10, K_CONTIG, 2, 40, 256, 1, DEFAULT),
    Row("R12", 4, ANY_TAPS, 12, K_POLY, 4, 8, 128, 1, DEFAULT),
    Row("R16", 4, ANY_TAPS, 16, K_POLY, 4, 8, 128, 1, DEFAULT),
    Row("R20", 4, ANY_TAPS, 20, K_POLY, 1, 8, 256, 1, DEFAULT),
    Row("R24", 4, ANY_TAPS, 24, K_POLY, 1, 8, 256, 1, DEFAULT),
    Row("R32", 4, ANY_TAPS, 32, K_POLY, 1, 8, 256, 1, DEFAULT),
    Row("R40", 4, ANY_TAPS, 40, K_POLY, 1, 8, 256, 1, DEFAULT),
    Row("R48", 4, ANY_TAPS, 48, K_POLY, 1, 8, 128, 1, DEFAULT),
    Row("R64", 4, ANY_TAPS, 64, K_POLY, 1, 8, 128, 1, DEFAULT),
)
ROW = {r.name: r for r in ROWS}
ROW_INDEX = {r.name: i for i, r in enumerate(ROWS)}

SAMPLE_BYTES = {REAL: 4, COMPLEX: 8, IQ8: 2}
SRC_ALIGN = {REAL: 16, COMPLEX: 16, IQ8: 4}
TAP_NAMES = {REAL_TAPS: "real", COMPLEX_TAPS: "complex"}
MODE_NAMES = {FIR: "fir", FM: "fm", AM: "am", IQ: "iq"}
FAMILY_NAMES = {K_POLY: "polyphase", K_CONTIG: "contiguous"}


def sample_of(row):
    return REAL if row.cls == 4 else COMPLEX


def tap_kinds(row):
    return (REAL_TAPS, COMPLEX_TAPS) if row.taps == ANY_TAPS else (row.taps,)


def ct(row):
    """Taps of one chunk."""
    return row.chunk * row.D if row.kernel == K_POLY else row.chunk


def kt(row):
    """Outputs of one tile."""
    return row.WG * row.R


def fm_tile_stride(sample, tile, D):
    """fir_plan.hpp fm_tile_stride: FM tiles overlap by one output, or by two where one would leave the staging
    alignment."""
    return tile - 1 if ((tile - 1) * D * SAMPLE_BYTES[sample]) % SRC_ALIGN[sample] == 0 else tile - 2


def stride(row, mode):
    """Outputs from one tile's start to the next."""
    if mode != FM:
        return kt(row)
    return kt(row) - row.R if row.kernel == K_POLY else fm_tile_stride(sample_of(row), kt(row), row.D)


def t_edges(chunk_taps):
    ts = (1, chunk_taps - 1, chunk_taps, chunk_taps + 1, 2 * chunk_taps, 2 * chunk_taps + 1)
    return sorted({t for t in ts if t > 0})


def n_edges(s):
    return sorted({n for n in (1, s - 1, s, s + 1, 2 * s + 3) if n > 0})


# ------------------------------------------------------------------------------------------------
# What the GPU modules run, and what each launch must plan to. A Launch is one call as the plan sees it; `expect` is
# ("row", name): that table row, routed; ("variant", number, name): the D = 4 tile named outright, which has that
# row's shape; ("rt", wg, paired): the runtime-decimation tile with that workgroup width.
# ------------------------------------------------------------------------------------------------
Launch = namedtuple("Launch", "taps sample mode D T N variant inm q0 expect")

# real taps, complex samples, FIR mode at D = 4: gsdrxFirFCVariant names the three tiles
D4_VARIANT = {"C4": 0, "C4R2": 25, "C4R1": 26}
D4_CUS = (64, 256, 304)         # CU counts the size-routed D = 4 cases are planned with
D4_BIG_T = (65, 129)
D4_WINDOW = 515                 # outputs of a window of a large D = 4 call (two C4R1 tiles and a ragged third)
D4_CHAIN_T = 129


def d4_n_r2(cus):
    """A D = 4 call one output past the 256-output tiles' range: the 512-output tiles (C4R2)."""
    return 512 * (cus + 1) + 1


def d4_n_r4(cus):
    """A D = 4 call of three rounds of 1,024-output tiles and one output: the default tile (C4)."""
    return 12288 * cus + 1


def is_d4_complex(row):
    return row.D == 4 and row.cls == 2


def routed_name(row):
    """The row a routed call of the sweep's sizes (at most 2,051 outputs) runs: its own, but at D = 4 on complex
    samples the 256-output short-call tile."""
    return "C4R1" if is_d4_complex(row) else row.name


def fir_grid(row):
    """(tap counts, output counts) of a row's FIR-mode sweep."""
    return t_edges(ct(row)), n_edges(kt(row))


def fir_offsets(sample):
    """Input pointers off 16-byte alignment, in samples: one complex sample; one and three floats."""
    return (1,) if sample == COMPLEX else (1, 3)


def fir_takes_int8(row, taps):
    """Rows whose FIR sweep adds the int8 I/Q front end: complex samples, real taps; at D = 4 only the default tile
    (variant 0), the others having no int8 form."""
    return row.cls == 2 and taps == REAL_TAPS and (row.D != 4 or row.name == "C4")


def fir_launches(row, taps):
    """Every launch of test_gpu_fir_rows.py for (row, tap kind) at the sweep's sizes."""
    sample, D = sample_of(row), row.D
    named = is_d4_complex(row) and taps == REAL_TAPS
    variant = D4_VARIANT[row.name] if named else -1
    expect = ("variant", variant, row.name) if named else ("row", routed_name(row))
    ts, ns = fir_grid(row)
    out = [Launch(taps, sample, FIR, D, T, N, variant, 0, 0, expect) for T in ts for N in ns]
    if named:  # the routed call and the other two tiles beside every one of them
        for T in ts:
            for N in ns:
                out.append(Launch(taps, sample, FIR, D, T, N, -1, 0, 0, ("row", "C4R1")))
                out += [Launch(taps, sample, FIR, D, T, N, v, 0, 0, ("variant", v, name))
                        for name, v in D4_VARIANT.items() if v != variant]
    t_top, n_top = ts[-1], ns[-1]
    for off in fir_offsets(sample):
        out.append(Launch(taps, sample, FIR, D, t_top, n_top, variant, off * SAMPLE_BYTES[sample], 0, expect))
    if fir_takes_int8(row, taps):
        out.append(Launch(taps, IQ8, FIR, D, t_top, n_top, variant, 0, 0, expect))
    out.append(Launch(taps, sample, FIR, D, ct(row) + 1, n_top, variant, 0, 0, expect))   # the padding poison
    return out


def d4_big_launches(cus):
    """gsdrFirCC at D = 4 reaches C4R2 and C4 by size alone: one call each, and their 515-output windows."""
    out = []
    for T in D4_BIG_T:
        out.append(Launch(COMPLEX_TAPS, COMPLEX, FIR, 4, T, d4_n_r2(cus), -1, 0, 0, ("row", "C4R2")))
        out.append(Launch(COMPLEX_TAPS, COMPLEX, FIR, 4, T, d4_n_r4(cus), -1, 0, 0, ("row", "C4")))
        out.append(Launch(COMPLEX_TAPS, COMPLEX, FIR, 4, T, D4_WINDOW, -1, 0, 0, ("row", "C4R1")))
    return out


def big_windows(n, tile):
    """First outputs of the three windows of a large call: head, across a tile edge in the middle, tail."""
    mid = (n // 2) // tile * tile - D4_WINDOW // 2
    return (0, mid, n - D4_WINDOW)


# The chain modes (FM, AM, IQ: real taps on complex samples through the NCO)
CHAIN_ROWS = tuple(r for r in ROWS if r.cls == 2)
CHAIN_MODES = (IQ, AM, FM)


def chain_first_indices(D, s):
    """firstSampleIndex values: q0 = firstSampleIndex / D puts output 0 first in its tile, second, and last."""
    return (0, D, D * (s - 1))


def chain_grid(row, mode):
    """(tap counts, output counts, firstSampleIndex values) of a row's sweep in a chain mode."""
    s = stride(row, mode)
    return t_edges(ct(row)), n_edges(s), chain_first_indices(row.D, s)


def chain_launches(row, mode):
    ts, ns, firsts = chain_grid(row, mode)
    expect = ("row", routed_name(row))
    return [Launch(REAL_TAPS, COMPLEX, mode, row.D, T, N, -1, 0, first // row.D, expect)
            for T in ts for N in ns for first in firsts]


D4_CHAIN_FIRST = 4 * 511        # output 0 last in its 512-output tile


def d4_chain_big_launches(cus):
    """IQ and AM at D = 4 on the 512-output tiles, and the 515-output calls at their windows."""
    n, out = d4_n_r2(cus), []
    for mode in (IQ, AM):
        out.append(Launch(REAL_TAPS, COMPLEX, mode, 4, D4_CHAIN_T, n, -1, 0, D4_CHAIN_FIRST // 4, ("row", "C4R2")))
        out += [Launch(REAL_TAPS, COMPLEX, mode, 4, D4_CHAIN_T, D4_WINDOW, -1, 0, D4_CHAIN_FIRST // 4 + k0,
                       ("row", "C4R1")) for k0 in big_windows(n, 512)]
    return out


# ------------------------------------------------------------------------------------------------
# The runtime-decimation tile (k_fir_rt): decimations without a row. Odd D reads its window unpaired, even D paired;
# the workgroup narrows from 256 to 128 and 64 outputs where the tile would not fit the LDS budget.
# ------------------------------------------------------------------------------------------------
RT_CHUNK = 16
RT_DS = (9, 50, 100)
RT_WG = {(COMPLEX, 9): 256, (COMPLEX, 50): 128, (COMPLEX, 100): 64, (REAL, 9): 256, (REAL, 50): 256, (REAL, 100): 128}
RT_CHAIN_DS = (9, 50)


def rt_ct16(D):
    return RT_CHUNK * -(-(D + 1) // RT_CHUNK)


def rt_ts(D):
    """Tap counts past D (at or below it the generic kernel runs): the least, whole chunks, a last chunk of one tap,
    and one more chunk."""
    c = rt_ct16(D)
    return sorted({D + 1, c, c + 1, c + 17})


def rt_poison_t(D):
    return rt_ct16(D) + 1       # 15 padding taps, the most


def rt_stride(sample, D, mode):
    wg = RT_WG[(sample, D)]
    return fm_tile_stride(sample, wg, D) if mode == FM else wg


def rt_expect(sample, D):
    return ("rt", RT_WG[(sample, D)], D % 2 == 0)


def rt_fir_grid(sample, D):
    return rt_ts(D), n_edges(rt_stride(sample, D, FIR))


def rt_fir_launches(sample, taps, D):
    ts, ns = rt_fir_grid(sample, D)
    expect = rt_expect(sample, D)
    out = [Launch(taps, sample, FIR, D, T, N, -1, 0, 0, expect) for T in ts for N in ns]
    out += [Launch(taps, sample, FIR, D, ts[-1], ns[-1], -1, off * SAMPLE_BYTES[sample], 0, expect)
            for off in fir_offsets(sample)]
    out.append(Launch(taps, sample, FIR, D, rt_poison_t(D), ns[-1], -1, 0, 0, expect))
    return out


def rt_chain_grid(D, mode):
    s = rt_stride(COMPLEX, D, mode)
    return rt_ts(D), n_edges(s), chain_first_indices(D, s)


def rt_chain_launches(D, mode):
    ts, ns, firsts = rt_chain_grid(D, mode)
    return [Launch(REAL_TAPS, COMPLEX, mode, D, T, N, -1, 0, first // D, rt_expect(COMPLEX, D))
            for T in ts for N in ns for first in firsts]


# ------------------------------------------------------------------------------------------------
# The parameter lists of the GPU modules
# ------------------------------------------------------------------------------------------------
FIR_PARAMS = [(r, k) for r in ROWS for k in tap_kinds(r)]
RT_FIR_PARAMS = [(s, k, D) for s in (COMPLEX, REAL) for k in (REAL_TAPS, COMPLEX_TAPS) for D in RT_DS]
CHAIN_PARAMS = [(r, m) for r in CHAIN_ROWS for m in CHAIN_MODES]
RT_CHAIN_PARAMS = [(D, m) for D in RT_CHAIN_DS for m in CHAIN_MODES]


def rows_with_cases():
    """Names of the rows some launch of the sweep expects to run."""
    names = set()
    launches = [l for r, k in FIR_PARAMS for l in fir_launches(r, k)]
    launches += [l for r, m in CHAIN_PARAMS for l in chain_launches(r, m)]
    launches += d4_big_launches(256) + d4_chain_big_launches(256)
    for l in launches:
        names.add(l.expect[1] if l.expect[0] == "row" else l.expect[2])
    return names


def fir_id(param):
    row, taps = param
    return f"{row.name}-{TAP_NAMES[taps]}"


def rt_fir_id(param):
    sample, taps, D = param
    return f"rt{D}-{'complex' if sample == COMPLEX else 'real'}-samples-{TAP_NAMES[taps]}-taps"


def chain_id(param):
    row, mode = param
    return f"{row.name}-{MODE_NAMES[mode]}"


def rt_chain_id(param):
    D, mode = param
    return f"rt{D}-{MODE_NAMES[mode]}"
