"""CPU: the FIR row sweep's case tables (tests/fir_sweep.py) against the launch plan (gsdr_amd/csrc/fir_plan.hpp,
compiled into test_fir_plan.py's host program): the literal shape table is the header's, every row of it has sweep
cases, and every launch the GPU modules test_gpu_fir_rows.py and test_gpu_chain_rows.py issue plans to the row and
kernel family it names -- with the tap chunks its tap count was chosen for, within the LDS budget, and in the chain
modes with output 0 where its firstSampleIndex was chosen to put it."""
import pytest

import fir_sweep as sw
from test_fir_plan import BUDGET, CONTIG, POLY, RT, build_plan_program, case

FAMILY_OF = {sw.K_POLY: POLY, sw.K_CONTIG: CONTIG}


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    return build_plan_program(tmp_path_factory.mktemp("fir_sweep_plan"))


def plan_all(program, launches, cus=256):
    run, _ = program
    cases = [case(taps=l.taps, sample=l.sample, mode=l.mode, D=l.D, T=l.T, N=l.N, variant=l.variant, inm=l.inm,
                  q0=l.q0, cus=cus) for l in launches]
    return list(zip(launches, run(cases)))


def check(l, p):
    """Launch l's plan p is what l.expect says."""
    assert p["status"] == 0, (l, p)
    assert 0 < p["lds"] <= BUDGET, (l, p)
    if l.expect[0] == "rt":
        _, wg, paired = l.expect
        assert p["family"] == RT and p["wg"] == wg and p["paired"] == (1 if paired else 0), (l, p)
        assert p["nch"] == -(-l.T // sw.RT_CHUNK), (l, p)
        assert p["stride"] == sw.rt_stride(l.sample, l.D, l.mode), (l, p)
        return
    row = sw.ROW[l.expect[1] if l.expect[0] == "row" else l.expect[2]]
    assert p["family"] == FAMILY_OF[row.kernel], (l, p)
    if l.expect[0] == "row":
        assert p["row"] == sw.ROW_INDEX[row.name] and p["variant"] == -1, (l, p)
    else:
        assert p["variant"] == l.expect[1] and p["row"] == -1, (l, p)
    assert (p["kernel"], p["D"], p["R"], p["chunk"], p["WG"]) == (row.kernel, row.D, row.R, row.chunk, row.WG), (l, p)
    assert p["nch"] == -(-l.T // sw.ct(row)), (l, p)
    assert p["stride"] == sw.stride(row, l.mode), (l, p)
    if l.mode != sw.FIR and row.kernel == sw.K_POLY:
        assert p["shift"] == l.q0 % sw.stride(row, l.mode), (l, p)
    else:
        assert p["shift"] == 0, (l, p)


def test_literal_table_is_the_headers(program):
    _, table = program
    got = table()
    assert len(got) == len(sw.ROWS)
    for i, (g, r) in enumerate(zip(got, sw.ROWS)):
        want = dict(row=i, cls=r.cls, taps=r.taps, D=r.D, kernel=r.kernel, R=r.R, chunk=r.chunk, WG=r.WG, SUBS=r.SUBS,
                    role=r.role)
        assert g == want, r.name


def test_every_row_has_cases(program):
    """A row added to the header without sweep cases fails here (and above, until the literal table has it)."""
    _, table = program
    have = sw.rows_with_cases()
    assert have == {r.name for r in sw.ROWS}
    assert len(table()) == len(have)
    # every row is also a parameter of the module of each mode it serves
    assert {r.name for r, _ in sw.FIR_PARAMS} == {r.name for r in sw.ROWS}
    assert {(r.name, k) for r, k in sw.FIR_PARAMS} == {(r.name, k) for r in sw.ROWS for k in sw.tap_kinds(r)}
    assert {r.name for r, _ in sw.CHAIN_PARAMS} == {r.name for r in sw.ROWS if r.cls == 2}


def test_edge_sets():
    assert sw.t_edges(32) == [1, 31, 32, 33, 64, 65] and sw.t_edges(1) == [1, 2, 3]
    assert sw.n_edges(256) == [1, 255, 256, 257, 515] and sw.n_edges(2) == [1, 2, 3, 7]
    assert [sw.ct(sw.ROW[n]) for n in ("C2", "R4", "C3", "R3", "R6", "C6", "C40", "C48", "C64")] == \
        [32, 32, 24, 36, 36, 48, 320, 384, 512]
    assert [sw.rt_ts(D) for D in sw.RT_DS] == [[10, 16, 17, 33], [51, 64, 65, 81], [101, 112, 113, 129]]


def test_fir_launches_plan_to_their_rows(program):
    grid = lds = 0
    for row, taps in sw.FIR_PARAMS:
        ts, ns = sw.fir_grid(row)
        grid += len(ts) * len(ns)
        assert len(ts) == 6 and len(ns) == 5
        for l, p in plan_all(program, sw.fir_launches(row, taps)):
            check(l, p)
            lds = max(lds, p["lds"])
    assert grid == 2160
    print(f"FIR sweep: {grid} (row, taps, T, N) cases, largest tile {lds} bytes of LDS")


def test_chain_launches_plan_to_their_rows(program):
    n = lds = 0
    for row, mode in sw.CHAIN_PARAMS:
        launches = sw.chain_launches(row, mode)
        n += len(launches)
        for l, p in plan_all(program, launches):
            check(l, p)
            lds = max(lds, p["lds"])
        if row.kernel == sw.K_POLY:  # output 0 first in its tile, second, and last
            s = sw.stride(sw.ROW[sw.routed_name(row)], mode)
            assert sorted({l.q0 % s for l in launches}) == sorted({0, 1, (sw.stride(row, mode) - 1) % s})
    assert n == 5130
    print(f"chain sweep: {n} (row, mode, T, N, q0) cases, largest tile {lds} bytes of LDS")


def test_runtime_d_launches_plan_to_the_stated_widths(program):
    widths = set()
    for sample, taps, D in sw.RT_FIR_PARAMS:
        for l, p in plan_all(program, sw.rt_fir_launches(sample, taps, D)):
            check(l, p)
            widths.add((sample, p["wg"], p["paired"]))
    for D, mode in sw.RT_CHAIN_PARAMS:
        for l, p in plan_all(program, sw.rt_chain_launches(D, mode)):
            check(l, p)
    assert widths == {(sw.COMPLEX, 256, 0), (sw.COMPLEX, 128, 1), (sw.COMPLEX, 64, 1), (sw.REAL, 256, 0),
                      (sw.REAL, 256, 1), (sw.REAL, 128, 1)}


def test_d4_complex_routes_by_size(program):
    """plan_d4_row: the sweep's sizes run the 256-output tile whatever the CU count; one output past its range the
    512-output tile; three rounds of 1,024-output tiles and one output the default tile."""
    d4 = [r for r in sw.ROWS if sw.is_d4_complex(r)]
    assert [r.name for r in d4] == ["C4", "C4R2", "C4R1"]
    for cus in sw.D4_CUS:
        small = [l for r in d4 for k in sw.tap_kinds(r) for l in sw.fir_launches(r, k)]
        small += [l for r in d4 for m in sw.CHAIN_MODES for l in sw.chain_launches(r, m)]
        assert max(l.N for l in small) == 2 * 1024 + 3
        routed = [l for l in small if l.expect[0] == "row"]
        assert routed and all(l.expect[1] == "C4R1" for l in routed)
        big = sw.d4_big_launches(cus) + sw.d4_chain_big_launches(cus)
        assert {l.expect[1] for l in big} == {"C4", "C4R2", "C4R1"}
        assert {l.N for l in big} == {sw.D4_WINDOW, 512 * (cus + 1) + 1, 12288 * cus + 1}
        for l, p in plan_all(program, small + big, cus=cus):
            check(l, p)
    # the windows of a large call lie inside it, the middle one across a tile edge
    for n, tile in ((sw.d4_n_r2(256), 512), (sw.d4_n_r4(256), 1024)):
        head, mid, tail = sw.big_windows(n, tile)
        assert head == 0 and tail + sw.D4_WINDOW == n and sw.D4_WINDOW < mid < tail - sw.D4_WINDOW
        assert mid // tile + 1 == (mid + sw.D4_WINDOW - 1) // tile
