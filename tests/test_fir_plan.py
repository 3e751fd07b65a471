"""CPU: the FIR engine's launch plan (gsdr_amd/csrc/fir_plan.hpp, HIP-free) compiled into a small host program, and
what its numbers must satisfy for fir_dispatch.hpp to be safe and to keep its contract: tiles that cover every
output (and, in FM mode, every output's partner), LDS within the 64 KB budget and large enough for the tile, the
generic kernel only where nothing tiled applies, an NCO cell grid that depends on q0 alone, a route that depends on
the call's size only through the documented short-call switches, persistent grids within the slots of the chip,
multi-channel rows that are the single-channel rows, and the status of every refusal."""
import json
import os
import subprocess

import pytest

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "gsdr_amd", "csrc")

PLAN_PROGRAM = r"""
#include <cinttypes>
#include <cstdio>
#include <cstring>

#include "fir_plan.hpp"

using namespace gsdr::firplan;

int main(int argc, char** argv) {
  if (argc > 1 && std::strcmp(argv[1], "table") == 0) {
    for (int i = 0; i < kRowCount; ++i) {
      const Row& r = kRows[i];
      std::printf("{\"row\":%d,\"cls\":%d,\"taps\":%d,\"D\":%d,\"kernel\":%d,\"R\":%d,\"chunk\":%d,\"WG\":%d,\"SUBS\":%d,\"role\":%d}\n",
                  i, r.cls, r.taps, r.D, r.kernel, r.R, r.chunk, r.WG, r.SUBS, r.role);
    }
    return 0;
  }
  Call c;
  int stream_tiled = 0;
  while (std::scanf("%d %d %d %d %" SCNu64 " %" SCNu64 " %" SCNu64 " %d %d %u %" SCNu64 " %" SCNu64 " %u %" SCNu64
                    " %" SCNd64 " %d",
                    &c.entry, &c.taps, &c.sample, &c.mode, &c.D, &c.T, &c.N, &c.variant, &stream_tiled, &c.group, &c.in,
                    &c.out, &c.out_phase, &c.q0, &c.in_off, &c.cus) == 16) {
    c.stream_tiled = stream_tiled != 0;
    const Plan p = plan(c);
    std::printf("{\"status\":%d,\"family\":%d,\"row\":%d,\"variant\":%d,\"kernel\":%d,\"D\":%d,\"R\":%d,\"chunk\":%d,\"WG\":%d,"
                "\"SUBS\":%d,\"vec\":%d,\"sh\":%d,\"nch\":%u,\"lds\":%" PRIu64 ",\"stride\":%u,\"shift\":%u,\"sub0\":%u,"
                "\"tiles\":%" PRIu64 ",\"grid\":%u,\"wg\":%u,\"paired\":%d,\"NS\":%d,\"G\":%d,\"LM\":%d,\"OA\":%d,\"NCT\":%d,"
                "\"BPC\":%d,\"PF\":%d,\"ns\":%u}\n",
                p.status, p.family, p.row, p.variant, p.shape.kernel, p.shape.D, p.shape.R, p.shape.chunk, p.shape.WG,
                p.shape.SUBS, p.vec ? 1 : 0, p.sh, p.nch, p.lds, p.tile_stride, p.tile_shift, p.cell_sub0, p.tiles, p.grid,
                p.wg, p.paired ? 1 : 0, p.NS, p.G, p.LM, p.OA ? 1 : 0, p.NCT, p.BPC, p.PF, p.ns);
  }
  return 0;
}
"""

# fir_plan.hpp's enumerators
ENTRY_FIR, ENTRY_GENERIC, ENTRY_I8_FIR, ENTRY_I8_CHAIN = range(4)
REAL_TAPS, COMPLEX_TAPS, ANY_TAPS = range(3)
REAL, COMPLEX, IQ8 = range(3)
FIR, FM, AM, IQ = range(4)
OK, INVALID, NOT_SUPPORTED, NO_CUS = range(4)
NONE, POLY, GROUPED, CONTIG, RT, GENERIC, MFMA_BC, I8_FIR, I8_CHAIN, PROBE = range(10)
K_POLY, K_CONTIG = 0, 1
DEFAULT, SHORT, MULTI = 1, 2, 4

BUDGET = 64 * 1024
MAX_GRID = 0x7FFFFFFF
TILED = (POLY, GROUPED, CONTIG, RT)
G_OF = {REAL: 4, COMPLEX: 2, IQ8: 2}
BYTES_OF = {REAL: 4, COMPLEX: 8, IQ8: 2}
ALIGN_OF = {REAL: 16, COMPLEX: 16, IQ8: 4}
IN0, OUT0 = 0x7F0000100000, 0x7F0040000000

D_LIST = list(range(1, 14)) + [16, 20, 24, 32, 40, 48, 50, 64, 100, 127, 128, 200, 4096, 4097]
T_LIST = [1, 2, 8, 63, 127, 128, 132, 133, 196, 197, 1000, 8000, 20000, 1 << 26, (1 << 26) + 1]
N_LIST = [1, 2, 255, 256, 257, 1019, 1020, 1021, 1023, 1024, 1025, 131072, 131073, 1 << 24, 1 << 40]
# (taps, sample, mode): FF, FC, CF, CC and int8 in FIR mode; FC and int8 in the chain modes
TYPES = [(REAL_TAPS, REAL, FIR), (REAL_TAPS, COMPLEX, FIR), (COMPLEX_TAPS, REAL, FIR), (COMPLEX_TAPS, COMPLEX, FIR),
         (REAL_TAPS, IQ8, FIR)] + [(REAL_TAPS, s, m) for s in (COMPLEX, IQ8) for m in (FM, AM, IQ)]


def case(taps=REAL_TAPS, sample=COMPLEX, mode=FIR, D=4, T=127, N=131073, entry=ENTRY_FIR, variant=-1, stream_tiled=0,
         group=0, inm=0, outm=0, phase=0, q0=0, in_off=0, cus=256):
    return (entry, taps, sample, mode, D, T, N, variant, stream_tiled, group, IN0 + inm, OUT0 + outm, phase, q0, in_off,
            cus)


def build_plan_program(directory, extra_flags=()):
    """Compiles fir_plan.hpp into a host program in `directory`; returns (run(cases) -> one dict a case, table())."""
    src = os.path.join(str(directory), "fir_plan.cpp")
    exe = os.path.join(str(directory), "fir_plan" + ("_san" if extra_flags else ""))
    with open(src, "w") as f:
        f.write(PLAN_PROGRAM)
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", *extra_flags, "-I" + CSRC, src, "-o", exe],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]

    def run(cases):
        text = "".join(" ".join(str(v) for v in c) + "\n" for c in cases)
        out = subprocess.run([exe], input=text, capture_output=True, text=True)
        assert out.returncode == 0 and out.stderr == "", (out.returncode, out.stderr[-3000:])
        lines = out.stdout.splitlines()
        assert len(lines) == len(cases)
        return [json.loads(line) for line in lines]

    def table():
        out = subprocess.run([exe, "table"], capture_output=True, text=True)
        assert out.returncode == 0 and out.stderr == ""
        return [json.loads(line) for line in out.stdout.splitlines()]

    return run, table


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    return build_plan_program(tmp_path_factory.mktemp("fir_plan"))


@pytest.fixture(scope="module")
def planner(program):
    return program[0]


@pytest.fixture(scope="module")
def rows(program):
    return program[1]()


def sweep_cases():
    """Every type, decimation and tap count at a few sizes, single-channel, stream-tiled and grouped; then every other
    axis against one shape of every kernel family."""
    cases = []
    for taps, sample, mode in TYPES:
        q0 = 1019 if mode != FIR else 0
        for D in D_LIST:
            for T in T_LIST:
                for N in (1, 1025, 131073, 1 << 24):
                    cases.append(case(taps, sample, mode, D, T, N, q0=q0))
                    if sample != REAL:
                        cases.append(case(taps, sample, mode, D, T, N, q0=q0, stream_tiled=1, in_off=-126))
                    if mode != FIR:
                        cases += [case(taps, sample, mode, D, T, N, q0=q0, group=g) for g in (1, 8)]
        for D in (1, 3, 4, 8, 13, 100, 4097):
            for T in (8, 127, 197, 20000):
                for N in N_LIST + [3144704, 3144705, (1 << 39) + 1, (1 << 41) + 1, (1 << 43) + 1]:
                    for cus in (0, 64, 256):
                        cases.append(case(taps, sample, mode, D, T, N, q0=q0, cus=cus))
                for inm in (0, 1, 2, 4, 8, 12):
                    for outm in (0, 4, 8):
                        for phase in (0, 5, 15):
                            cases.append(case(taps, sample, mode, D, T, 131073, inm=inm, outm=outm, phase=phase, q0=q0))
                if mode != FIR:
                    for q in (0, 3, 1019, 1020, (1 << 32) + 5):
                        for N in (1021, 131073, 1 << 24):
                            cases.append(case(taps, sample, mode, D, T, N, q0=q))
                            cases.append(case(taps, sample, mode, D, T, N, q0=q, group=8, inm=8))
    for sample in (COMPLEX, IQ8):   # the tuning variants
        for v in (0, 1, 3, 4, 5, 7, 8, 9, 10, 11, 13, 14, 24, 25, 26, 28, 40, 41, 42, 43, 44, 45, 46, 2, 99, 100):
            for T in (8, 127, 132, 133, 144, 145, 196, 197, 20000):
                for N in (1, 1025, 3144705, (1 << 42) + 1):
                    for cus in (0, 256):
                        cases += [case(sample=sample, T=T, N=N, variant=v, cus=cus, outm=o, phase=5) for o in (0, 4)]
    for mode in (FIR, FM, AM):      # the int8 matrix-core stream steps
        entry = ENTRY_I8_FIR if mode == FIR else ENTRY_I8_CHAIN
        for T in (1, 127, 132, 133, 196, 197) if mode == FIR else (1, 127, 132):   # (the chain step's callers keep T <= 132)
            for N in N_LIST + [(1 << 42) + 1]:
                for cus in (0, 64, 256):
                    for inm in (0, 1, 2, 8):
                        for in_off in (0, -1, -126, 5):
                            cases.append(case(sample=IQ8, mode=mode, T=T, N=N, entry=entry, cus=cus, inm=inm, in_off=in_off,
                                              phase=5))
    for taps, sample, mode in TYPES:  # the generic kernel by name (the chains' T = 0)
        cases += [case(taps, sample, mode, D, 0, N, entry=ENTRY_GENERIC) for D in (1, 4, 13) for N in N_LIST + [1 << 39, (1 << 39) + 1]]
    return cases


@pytest.fixture(scope="module")
def sweep(planner):
    cases = sweep_cases()
    return list(zip(cases, planner(cases)))


def fields(c):
    return dict(zip(("entry", "taps", "sample", "mode", "D", "T", "N", "variant", "stream_tiled", "group", "in", "out",
                     "phase", "q0", "in_off", "cus"), c))


def tile_outputs(p, sample, mode):
    """FIR outputs one tile computes (its outputs, plus in FM mode the partners of its last ones)."""
    if p["family"] in (POLY, GROUPED, CONTIG, MFMA_BC):
        return p["WG"] * p["R"]
    if p["family"] in (RT, GENERIC):
        return p["wg"] + (1 if p["family"] == GENERIC and mode == FM else 0)
    if p["family"] == I8_FIR:
        return 4 * p["NCT"] * 128
    assert p["family"] == I8_CHAIN
    return 4 * p["NCT"] * 64


def tile_lds(G, D, R, WG, span, mode):
    """Bytes of LDS that hold a tile's samples [0, (KT - 1) D + span) as 16-byte granules, with one pad granule after
    every segment of SG = R D / G granules when SG is even (the kernels' image), plus the chains' exchange row."""
    granules = -(-((WG * R - 1) * D + span) // G)
    sg = R * D // G
    last = granules - 1
    image = (last + (last // sg if sg % 2 == 0 else 0) + 1) * 16
    return image + (WG * 8 if mode != FIR else 0)


def chunked_span(T, row, chunk):
    """T taps rounded up to whole chunks of `chunk` rows of `row` taps."""
    n = -(-(-(-T // row)) // chunk)
    return n, n * chunk * row


def test_every_case_has_a_documented_status_and_family(sweep):
    seen = set()
    for c, p in sweep:
        assert p["status"] in (OK, INVALID, NOT_SUPPORTED, NO_CUS), (c, p)
        if p["status"] != OK:
            # nothing to launch
            assert p["family"] == NONE and p["grid"] == 0 and p["tiles"] == 0 and p["lds"] == 0, (c, p)
        else:
            assert p["family"] != NONE, (c, p)
            seen.add(p["family"])
            if p["family"] != PROBE:
                assert 1 <= p["grid"] <= MAX_GRID and p["wg"] in (64, 128, 256), (c, p)
    assert seen == {POLY, GROUPED, CONTIG, RT, GENERIC, MFMA_BC, I8_FIR, I8_CHAIN, PROBE}


def test_tiles_cover_the_outputs_and_their_fm_partners(sweep):
    for c, p in sweep:
        f = fields(c)
        if p["status"] != OK or p["family"] == PROBE:
            continue
        N, mode = f["N"], f["mode"]
        if p["family"] in (I8_FIR, I8_CHAIN):
            stride = tile_outputs(p, f["sample"], mode) - (16 if (p["family"] == I8_CHAIN and mode == FM) else 0)
            lead = f["phase"] & 15          # the tile grid starts at output -phase
        else:
            stride, lead = (p["stride"], p["shift"]) if p["family"] != GENERIC else (256, 0)
        tiles = p["tiles"]
        assert stride >= 1 and lead < stride, (c, p)
        # tile t owns outputs [t stride - lead, (t + 1) stride - lead): the last tile is needed and reaches N
        assert (tiles - 1) * stride - lead < N <= tiles * stride - lead, (c, p)
        if mode == FM:
            # ... and computes the FIR output after its last one, the discriminator's partner
            assert tile_outputs(p, f["sample"], mode) >= stride + 1, (c, p)
        else:
            assert tile_outputs(p, f["sample"], mode) == stride, (c, p)
        if p["family"] == GROUPED:
            assert p["grid"] == -(-tiles // 8) * 8 * f["group"], (c, p)     # whole XCD rounds, times the channels
        elif p["family"] not in (I8_FIR, I8_CHAIN):
            assert p["grid"] == tiles, (c, p)


def test_lds_holds_the_tile_within_the_budget(sweep):
    for c, p in sweep:
        f = fields(c)
        if p["status"] != OK or p["family"] not in TILED + (MFMA_BC,):
            if p["status"] == OK and p["family"] != PROBE:
                assert p["lds"] == 0, (c, p)      # the generic and int8 matrix-core kernels take no dynamic LDS
            continue
        G, D, T = G_OF[f["sample"]], f["D"], f["T"]
        assert 0 < p["lds"] <= BUDGET and p["lds"] % 16 == 0, (c, p)
        kt = tile_outputs(p, f["sample"], f["mode"])
        # every sample the tile's outputs read, unpadded: a lower bound whatever the layout
        assert p["lds"] >= -(-((kt - 1) * D + T) // G) * 16, (c, p)
        if p["family"] in (POLY, GROUPED, CONTIG):
            assert p["D"] == D and (p["R"] * D) % G == 0
            nch, span = chunked_span(T, D if p["kernel"] == K_POLY else 1, p["chunk"])
            assert p["nch"] == nch and p["lds"] == tile_lds(G, D, p["R"], p["WG"], span, f["mode"]), (c, p)


def test_generic_only_where_nothing_tiled_applies(sweep, rows):
    """A call whose decimation has a row runs it unless its tile does not fit (or T > 2^26); one without runs the
    runtime-D kernel with the widest workgroup that fits, when taps overlap (T > D) and D <= 4096."""
    for c, p in sweep:
        f = fields(c)
        if f["entry"] != ENTRY_FIR or f["variant"] >= 0 or p["status"] == NO_CUS or p["family"] in (I8_FIR, I8_CHAIN):
            continue
        G, D, T, mode = G_OF[f["sample"]], f["D"], f["T"], f["mode"]
        mine = [r for r in rows if r["cls"] == G and r["D"] == D and r["taps"] in (ANY_TAPS, f["taps"])]
        if mine and T <= 1 << 26:
            fits = [r for r in mine if chunked_span(T, D if r["kernel"] == K_POLY else 1, r["chunk"])[1] <= 1 << 30 and
                    tile_lds(G, D, r["R"], r["WG"], chunked_span(T, D if r["kernel"] == K_POLY else 1, r["chunk"])[1],
                             mode) <= BUDGET]
            if f["group"] > 0 and not any(r["role"] & MULTI for r in mine):
                assert p["status"] == NOT_SUPPORTED, (c, p)
            elif p["status"] == OK and p["family"] in TILED:
                assert p["row"] in [r["row"] for r in fits], (c, p)
            elif p["status"] == OK:
                # (all of a decimation's shapes fit or fail together only roughly: the plan's own shape must not fit)
                assert p["family"] == GENERIC and f["group"] == 0 and not f["stream_tiled"], (c, p)
                assert len(fits) < len(mine), (c, p)
            elif p["status"] == NOT_SUPPORTED and p["tiles"] == 0 and f["N"] <= 1 << 40 and f["group"] * f["N"] < 1 << 38:
                assert (f["group"] > 0 or f["stream_tiled"]) and len(fits) < len(mine), (c, p)
        elif f["group"] > 0:
            assert p["status"] == NOT_SUPPORTED, (c, p)
        elif f["stream_tiled"]:
            assert p["status"] == NOT_SUPPORTED, (c, p)      # the runtime-D and generic kernels take no stream step
        elif p["status"] == OK:
            span = -(-T // 16) * 16
            need = {wg: -(-((wg - 1) * D + span) // G) * 16 + (wg * 8 if mode != FIR else 0) for wg in (256, 128, 64)}
            fitting = [wg for wg in (256, 128, 64) if need[wg] <= BUDGET]
            if T <= 1 << 26 and D < T and D <= 4096 and fitting:
                assert p["family"] == RT and p["wg"] == fitting[0] and p["lds"] == need[fitting[0]], (c, p)
                assert p["paired"] == (1 if D % 2 == 0 else 0) and p["sh"] == 0
            else:
                assert p["family"] == GENERIC, (c, p)


def test_nco_cell_grid_depends_on_q0_alone(sweep):
    by = {}
    for c, p in sweep:
        f = fields(c)
        if p["status"] != OK or p["family"] not in TILED:
            continue
        assert p["shift"] < p["stride"] and p["sub0"] < max(1, p["SUBS"]), (c, p)
        if p["family"] in (POLY, GROUPED) and f["mode"] != FIR:
            assert p["shift"] == f["q0"] % p["stride"] and p["sub0"] == f["q0"] // p["stride"] % p["SUBS"], (c, p)
            by.setdefault((p["row"], f["mode"], f["q0"]), set()).add((p["stride"], p["shift"], p["sub0"]))
        else:
            assert p["shift"] == 0 and p["sub0"] == 0, (c, p)   # FIR mode and the kernels tiled from output 0
    assert len(by) > 50 and all(len(v) == 1 for v in by.values())


def test_route_depends_on_the_size_only_through_the_short_call_switches(sweep):
    """(types, mode, D, T, residues, variant) fix the kernel family, shape and staging; the size moves only the D = 4
    tile of complex / int8 I/Q samples (with a known CU count) and the int8 matrix-core tile."""
    by = {}
    for c, p in sweep:
        f = fields(c)
        if p["status"] != OK:
            continue
        key = tuple(v for k, v in f.items() if k != "N")
        shape = [p[k] for k in ("family", "row", "variant", "kernel", "D", "R", "chunk", "WG", "SUBS", "vec", "sh", "nch",
                                "lds", "stride", "shift", "wg", "paired", "NS", "G", "LM", "OA", "NCT", "BPC", "PF", "ns")]
        by.setdefault(key, []).append((f, shape))
    sized = 0
    for key, plans in by.items():
        f = plans[0][0]
        if len({tuple(s) for _, s in plans}) == 1:
            continue
        sized += 1
        assert f["D"] == 4 and f["sample"] != REAL and f["cus"] > 0, key
        families = {s[0] for _, s in plans}
        assert families <= {POLY, GENERIC} or families <= {I8_FIR} or families <= {I8_CHAIN}, key
    assert sized > 20


def test_short_call_switches_flip_exactly_at_their_thresholds(planner):
    cus = 256
    # float tiles: 4 workgroups a CU. R 1 up to one 256-output tile for every second slot, R 2 below three rounds of
    # 1,024-output tiles
    for sample, mode, variant in ((COMPLEX, FIR, -1), (COMPLEX, FM, -1), (COMPLEX, AM, -1), (IQ8, IQ, -1), (IQ8, FM, 0)):
        ns = [131072, 131073, 3144704, 3144705]
        got = planner([case(sample=sample, mode=mode, N=n, variant=variant, cus=cus, q0=7) for n in ns])
        assert [(p["R"], p["SUBS"]) for p in got] == [(1, 4), (2, 2), (2, 2), (4, 1)], (sample, mode)
        cell = {p["stride"] * p["SUBS"] for p in got}
        assert cell == {1020 if mode == FM else 1024}      # one NCO cell for every D = 4 shape
        unknown = planner([case(sample=sample, mode=mode, N=n, variant=variant, cus=0, q0=7) for n in ns])
        assert all((p["R"], p["SUBS"], p["status"]) == (4, 1, OK) for p in unknown)
    # int8 matrix cores: 3 workgroups a CU, one C tile a wave below two rounds of slots
    # (tile strides with 4 C tiles and with 1: the FM chain's tiles overlap by 16 outputs)
    for mode, entry, big, small in ((FIR, ENTRY_FIR, 2048, 512), (FIR, ENTRY_I8_FIR, 2048, 512), (FM, ENTRY_FIR, 1008, 240),
                                    (AM, ENTRY_FIR, 1024, 256), (FM, ENTRY_I8_CHAIN, 1008, 240),
                                    (AM, ENTRY_I8_CHAIN, 1024, 256)):
        for phase in (0, 5):
            edge = 1535 * big - phase
            got = planner([case(sample=IQ8, mode=mode, entry=entry, N=n, phase=phase, cus=cus) for n in (edge - 1, edge, edge + 1)])
            assert [p["family"] for p in got] == [I8_FIR if mode == FIR else I8_CHAIN] * 3
            assert [p["NCT"] for p in got] == [1, 1, 4], (mode, entry, phase, got)
            assert [p["tiles"] for p in got] == [-(-(1535 * big - 1) // small), -(-1535 * big // small), 1536]
            assert all(p["grid"] == cus * 3 for p in got)


def test_persistent_grids_stay_within_the_slots(sweep):
    n = 0
    for c, p in sweep:
        f = fields(c)
        if p["status"] == OK and p["family"] in (I8_FIR, I8_CHAIN):
            n += 1
            assert p["BPC"] in (2, 3, 4) and p["grid"] == min(p["tiles"], f["cus"] * p["BPC"]), (c, p)
            assert p["wg"] == 256 and p["NCT"] in (1, 2, 4) and p["PF"] in (1, 2)
            assert p["ns"] * 32 >= (15 if p["family"] == I8_FIR else 7) * 4 + f["T"] and p["ns"] <= p["NS"], (c, p)
    assert n > 1000


def test_multi_channel_rows_are_the_single_channel_rows(planner, rows):
    multi = [r for r in rows if r["role"] & MULTI]
    assert sorted(r["D"] for r in multi) == [2, 4, 8]
    assert all(r["role"] & DEFAULT and r["cls"] == 2 and r["kernel"] == K_POLY and r["SUBS"] == 1 for r in multi)
    for mode in (FM, AM, IQ):
        for D in (2, 4, 8):
            for N in (1, 1025, 131073, 1 << 24):        # (D = 4: every short-call shape of the single channel)
                for q0 in (0, 3, 1019, (1 << 32) + 5):
                    one, grouped = planner([case(mode=mode, D=D, N=N, q0=q0), case(mode=mode, D=D, N=N, q0=q0, group=8)])
                    assert grouped["family"] == GROUPED and one["family"] == POLY
                    assert (grouped["D"], grouped["chunk"], grouped["nch"]) == (one["D"], one["chunk"], one["nch"])
                    cell = one["stride"] * one["SUBS"]
                    assert grouped["stride"] * grouped["SUBS"] == cell        # the same NCO cell ...
                    assert grouped["shift"] + grouped["sub0"] * grouped["stride"] == q0 % cell
                    assert one["shift"] + one["sub0"] * one["stride"] == q0 % cell   # ... and the same place in it
                    assert (grouped["vec"], grouped["sh"]) == (one["vec"], one["sh"])


def test_statuses(planner):
    def status(**kw):
        p = planner([case(**kw)])[0]
        return p["status"], p["family"]

    big_t = (1 << 26) + 1
    # T > 2^26: the generic kernel; not supported for a grouped or a stream-tiled call
    assert status(T=big_t) == (OK, GENERIC)
    assert status(T=big_t, mode=FM, group=4) == (NOT_SUPPORTED, NONE)
    assert status(T=big_t, stream_tiled=1) == (NOT_SUPPORTED, NONE)
    # a tap span that does not fit: generic, or not supported (grouped, stream-tiled)
    assert status(T=20000) == (OK, GENERIC)
    assert status(T=20000, mode=AM, group=4) == (NOT_SUPPORTED, NONE)
    assert status(T=20000, stream_tiled=1) == (NOT_SUPPORTED, NONE)
    # stream-tiled refuses the runtime-D, generic and matrix-core routes
    assert status(D=13) == (OK, RT) and status(D=13, stream_tiled=1) == (NOT_SUPPORTED, NONE)
    assert status(D=13, T=8) == (OK, GENERIC) and status(D=13, T=8, stream_tiled=1) == (NOT_SUPPORTED, NONE)
    assert status(entry=ENTRY_GENERIC, stream_tiled=1) == (NOT_SUPPORTED, NONE)
    assert status(sample=IQ8) == (OK, I8_FIR) and status(sample=IQ8, stream_tiled=1) == (OK, POLY)
    assert status(sample=IQ8, mode=FM) == (OK, I8_CHAIN) and status(sample=IQ8, mode=FM, stream_tiled=1) == (OK, POLY)
    assert status(variant=7, stream_tiled=1) == (NOT_SUPPORTED, NONE)
    # grouped launches exist for D in {2, 4, 8}
    assert status(mode=FM, D=8, group=3) == (OK, GROUPED) and status(mode=FM, D=6, group=3) == (NOT_SUPPORTED, NONE)
    # more workgroups than one launch takes: invalid value; not supported for a grouped call
    assert status(N=(1 << 41) + 1) == (INVALID, NONE) and status(N=(1 << 41) + 1, mode=FM, group=1) == (NOT_SUPPORTED, NONE)
    assert status(N=1 << 30, mode=FM, group=8) == (OK, GROUPED) and status(N=1 << 40, mode=FM, group=8) == (NOT_SUPPORTED, NONE)
    assert status(D=13, N=(1 << 39) + 1) == (INVALID, NONE) and status(D=13, T=8, N=(1 << 39) + 1) == (INVALID, NONE)
    assert status(D=13, T=8, N=MAX_GRID * 256) == (OK, GENERIC) and status(D=13, T=8, N=MAX_GRID * 256 + 1) == (INVALID, NONE)
    assert status(sample=IQ8, N=(1 << 42) + 1) == (INVALID, NONE) and status(sample=IQ8, mode=AM, N=(1 << 42) + 1) == (INVALID, NONE)
    # an unknown CU count: the default tile on the float paths, the query's error on the persistent int8 paths
    assert status(cus=0) == (OK, POLY) and status(sample=IQ8, cus=0) == (NO_CUS, NONE)
    assert status(sample=IQ8, mode=FM, cus=0) == (NO_CUS, NONE) and status(sample=IQ8, mode=IQ, cus=0) == (OK, POLY)
    assert status(sample=IQ8, entry=ENTRY_I8_CHAIN, mode=AM, cus=0) == (NO_CUS, NONE)
    # the int8 FIR's matrix-core route needs an 8-byte-aligned output and T <= 196; the chains' T <= 132
    assert status(sample=IQ8, outm=4) == (OK, POLY) and status(sample=IQ8, outm=8) == (OK, I8_FIR)
    assert status(sample=IQ8, T=196) == (OK, I8_FIR) and status(sample=IQ8, T=197) == (OK, POLY)
    assert status(sample=IQ8, mode=AM, T=132) == (OK, I8_CHAIN) and status(sample=IQ8, mode=AM, T=133) == (OK, POLY)
    assert status(sample=IQ8, entry=ENTRY_I8_FIR, outm=4) == (INVALID, NONE)
    assert status(sample=IQ8, entry=ENTRY_I8_FIR, T=197) == (INVALID, NONE)
    assert status(sample=IQ8, entry=ENTRY_I8_FIR, D=8) == (INVALID, NONE)
    # variants: the table's, the generic kernel, the matrix-core cores, the probes; anything else is invalid
    assert status(variant=0) == (OK, POLY) and status(variant=7) == (OK, GENERIC) and status(variant=13) == (OK, MFMA_BC)
    assert status(variant=13, T=133) == (INVALID, NONE) and status(variant=2) == (INVALID, NONE)
    assert status(variant=100) == (OK, PROBE) and status(variant=41) == (INVALID, NONE)
    assert status(sample=IQ8, variant=0) == (OK, POLY) and status(sample=IQ8, variant=8) == (INVALID, NONE)
    assert status(sample=IQ8, variant=41) == (OK, I8_FIR) and status(sample=IQ8, variant=100) == (INVALID, NONE)
    assert status(sample=IQ8, variant=43, T=133) == (INVALID, NONE) and status(sample=IQ8, variant=40, T=133) == (OK, I8_FIR)
    # variants are for real taps in FIR mode at D = 4: elsewhere the number is ignored (chains: variant 0 = the exact path)
    assert status(variant=2, D=8) == (OK, POLY) and status(variant=2, taps=COMPLEX_TAPS) == (OK, POLY)
    assert status(sample=IQ8, mode=FM, variant=0) == (OK, POLY)


# DESIGN.md section 3.1, "Shapes": (kernel, R, chunk, WG) of each decimation's default row
COMPLEX_ROWS = {1: (K_CONTIG, 8, 16, 256), 2: (K_POLY, 8, 16, 128), 3: (K_CONTIG, 4, 24, 256), 4: (K_POLY, 4, 16, 256),
                5: (K_CONTIG, 4, 20, 128), 6: (K_POLY, 2, 8, 256), 7: (K_CONTIG, 4, 28, 128), 8: (K_POLY, 2, 8, 256),
                10: (K_POLY, 2, 8, 256), 12: (K_POLY, 2, 8, 256), 16: (K_POLY, 2, 8, 128), 20: (K_POLY, 1, 8, 256),
                24: (K_POLY, 1, 8, 256), 32: (K_POLY, 1, 8, 128), 40: (K_POLY, 1, 8, 128), 48: (K_POLY, 1, 8, 128),
                64: (K_POLY, 1, 8, 64)}
REAL_ROWS = {1: (K_CONTIG, 16, 32, 256), 2: (K_CONTIG, 8, 16, 256), 3: (K_CONTIG, 4, 36, 256), 4: (K_POLY, 8, 8, 128),
             5: (K_CONTIG, 4, 40, 128), 6: (K_CONTIG, 2, 36, 256), 7: (K_CONTIG, 4, 28, 128), 8: (K_POLY, 8, 8, 128),
             10: (K_CONTIG, 2, 40, 256), 12: (K_POLY, 4, 8, 128), 16: (K_POLY, 4, 8, 128), 20: (K_POLY, 1, 8, 256),
             24: (K_POLY, 1, 8, 256), 32: (K_POLY, 1, 8, 256), 40: (K_POLY, 1, 8, 256), 48: (K_POLY, 1, 8, 128),
             64: (K_POLY, 1, 8, 128)}


def test_pinned_default_rows(planner, rows):
    def shape(p):
        return (p["kernel"], p["R"], p["chunk"], p["WG"])

    big = 1 << 24      # (past the D = 4 short-call sizes)
    for D, want in COMPLEX_ROWS.items():
        got = planner([case(sample=COMPLEX, D=D, N=big), case(sample=IQ8, D=D, N=big, mode=IQ),
                       case(sample=COMPLEX, D=D, N=big, taps=COMPLEX_TAPS)])
        assert [shape(p) for p in got] == [want] * 3, D
    for D, want in REAL_ROWS.items():
        got = planner([case(sample=REAL, D=D, N=big)])
        assert shape(got[0]) == want, D
    # complex taps on real samples at D = 1: R 8 (R 16 spilled to scratch)
    assert shape(planner([case(sample=REAL, taps=COMPLEX_TAPS, D=1)])[0]) == (K_CONTIG, 8, 16, 256)
    # one default row per (class, taps, D); the D = 4 short-call shapes are sub-tiles of the default tile
    keys = [(r["cls"], r["taps"], r["D"]) for r in rows if r["role"] & DEFAULT]
    assert len(keys) == len(set(keys))
    short = sorted((r["R"], r["SUBS"]) for r in rows if r["role"] & SHORT)
    assert short == [(1, 4), (2, 2)] and all(r["D"] == 4 and r["cls"] == 2 and r["chunk"] == 16 and r["WG"] == 256
                                             for r in rows if r["role"] & SHORT)


def test_staging(sweep):
    """Vector loads need an aligned pointer and tile stride; the shifted loads a pointer whole samples off with every
    tile equally off; the rest loads per sample."""
    seen = set()
    for c, p in sweep:
        f = fields(c)
        if p["status"] != OK or p["family"] not in TILED:
            continue
        A, B = ALIGN_OF[f["sample"]], BYTES_OF[f["sample"]]
        step = p["stride"] * f["D"] * B
        assert p["vec"] == (1 if f["in"] % A == 0 and step % A == 0 else 0), (c, p)
        assert not (p["vec"] and p["sh"])
        if p["sh"]:
            assert p["family"] != RT and f["in"] % B == 0 and (f["in"] % 16) // B % (16 // B) != 0 or f["sample"] == IQ8, (c, p)
            assert p["sh"] == ((f["in"] % 16) // 4 if f["sample"] == REAL else 1) and step % (16 if f["sample"] != IQ8 else 4) == 0
        seen.add((f["sample"], p["vec"], p["sh"]))
    assert {(COMPLEX, 1, 0), (COMPLEX, 0, 1), (COMPLEX, 0, 0), (IQ8, 1, 0), (IQ8, 0, 1), (IQ8, 0, 0), (REAL, 1, 0),
            (REAL, 0, 1), (REAL, 0, 2), (REAL, 0, 3), (REAL, 0, 0)} <= seen


def test_plan_under_the_sanitizers(tmp_path, sweep):
    """The same stand-alone program built with -fsanitize=address,undefined (where the host compiler has the
    runtimes) plans every case identically and reports nothing."""
    probe = tmp_path / "probe.cpp"
    probe.write_text("int main() { return 0; }\n")
    flags = ("-fsanitize=address,undefined", "-fno-sanitize-recover=undefined")
    r = subprocess.run(["g++", *flags, str(probe), "-o", str(tmp_path / "probe")], capture_output=True, text=True)
    if r.returncode != 0:
        pytest.skip("the host compiler has no address / undefined-behaviour sanitizer runtime")
    run, _ = build_plan_program(tmp_path, flags)
    assert run([c for c, _ in sweep]) == [p for _, p in sweep]
