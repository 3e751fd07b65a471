"""CPU: the channelizer's launch plan (gsdr_amd/csrc/channelizer_plan.hpp, HIP-free) compiled into a small host
program, and what its numbers must satisfy for channelizer.hip to be safe: the tiled route only for D in {M, M / 2},
its padded LDS image within the 64 KB budget and large enough for every sample a full tile reads, the largest
workgroup that fits, a plan that depends on (M, D, T) alone, tiles that cover [0, N) exactly once and a refusal
where one launch cannot hold the grid."""
import subprocess

import pytest

from channelizer_ref import build_plan_program

BUDGET = 64 * 1024
THREAD_LIMIT = (1 << 32) - 1           # blocks * threads of one launch
TILE, GENERIC = 0, 1
BANKS = [2, 4, 8, 16, 32, 64]


def tap_counts(M):
    return [1, M - 1, M, 4 * M + 3, 8 * M]


# the GPU tests' shapes, the timing shapes, the generic-route shapes and both sides of the LDS budget
SHAPES = [(M, D, T) for M in BANKS for D in (M, max(1, M // 2)) for T in tap_counts(M)]
SHAPES += [(16, 8, 127), (16, 16, 128), (64, 64, 512), (16, 16, 16), (64, 64, 0), (8, 8, 0),
           (4, 3, 33), (16, 5, 127), (64, 48, 300), (8, 1, 64), (8, 8, 20000), (8, 100001, 7), (16, 4, 127),
           (64, 16, 512), (2, 2, 5000), (2, 2, 5400), (2, 2, 5500), (2, 2, 8193), (64, 64, 3900), (64, 64, 4097), (64, 32, 6000),
           (64, 32, 6200), (8, (1 << 32) - 1, 7)]
SIZES = [1, 2, 63, 64, 65, 127, 128, 129, 255, 256, 257, 1024, 1 << 20, (1 << 24) + 5, (1 << 31) + 5, 1 << 32,
         (1 << 34) - 1, 1 << 34, 1 << 40]


@pytest.fixture(scope="module")
def planner(tmp_path_factory):
    return build_plan_program(tmp_path_factory.mktemp("channelizer_plan"))


@pytest.fixture(scope="module")
def table(planner):
    cases = [(M, D, T, n) for M, D, T in SHAPES for n in SIZES]
    return dict(zip(cases, planner(cases)))


def lds_needed(D, T, kt):
    """Bytes of float2 LDS that hold tile samples [0, (kt - 1) D + T) with one pad sample after each row of D when D
    is even (the kernel's image): the index of the last sample, plus one."""
    span = (kt - 1) * D + T
    if span == 0:
        return 0
    pad = 1 if D % 2 == 0 else 0
    return (span - 1 + (span - 1) // D * pad + 1) * 8


def test_plan_depends_on_the_shape_alone(table):
    for M, D, T in SHAPES:
        plans = [table[(M, D, T, n)] for n in SIZES]
        for key in ("route", "wg", "kt", "span", "lds_bytes"):   # (neither pointers nor the format are arguments)
            assert len({p[key] for p in plans}) == 1, (M, D, T, key)


def test_routes(table):
    by = {s: table[s + (1,)] for s in SHAPES}
    for M in BANKS:
        for D in (M, max(1, M // 2)):
            for T in tap_counts(M):
                assert by[(M, D, T)]["route"] == TILE, (M, D, T)
    for shape in [(16, 8, 127), (16, 16, 128), (64, 64, 512), (64, 64, 3900)]:
        assert by[shape]["route"] == TILE, shape
    # D outside {M, M / 2}
    for shape in [(4, 3, 33), (16, 5, 127), (64, 48, 300), (8, 1, 64), (8, 100001, 7), (16, 4, 127), (64, 16, 512),
                  (8, (1 << 32) - 1, 7)]:
        assert by[shape]["route"] == GENERIC, shape
    # 160 KB of samples a window
    assert by[(8, 8, 20000)]["route"] == GENERIC
    # the workgroup shrinks where D = 64 or long taps make the tile too large, and only there
    assert by[(16, 8, 127)]["kt"] == 256 and by[(16, 16, 128)]["kt"] == 256
    assert by[(64, 64, 512)]["kt"] == 64 and by[(64, 32, 512)]["kt"] == 128 and by[(32, 32, 256)]["kt"] == 128
    assert by[(32, 16, 256)]["kt"] == 256


def test_tiled_route_holds_its_tile_within_the_budget_and_is_the_largest_that_fits(table):
    seen = set()
    for M, D, T in SHAPES:
        p = table[(M, D, T, 1)]
        fitting = [wg for wg in (256, 128, 64) if lds_needed(D, T, wg) <= BUDGET]
        if p["route"] != TILE:
            if D in (M, M // 2):
                assert not fitting, (M, D, T)
            continue
        assert D in (M, M // 2) and D >= 1
        kt, wg = p["kt"], p["wg"]
        assert kt == wg and wg in (64, 128, 256)
        seen.add(wg)
        assert p["span"] == (kt - 1) * D + T
        assert lds_needed(D, T, kt) <= p["lds_bytes"] <= BUDGET, (M, D, T, p)
        assert p["lds_bytes"] % 16 == 0 and p["lds_bytes"] < lds_needed(D, T, kt) + 16
        assert p["pad"] == (1 if D % 2 == 0 else 0)
        assert wg == fitting[0], (M, D, T, p)   # the largest workgroup whose tile fits
    assert seen == {64, 128, 256}
    # on both sides of the budget with the smallest workgroup
    assert table[(2, 2, 5000, 1)]["route"] == TILE and table[(2, 2, 8193, 1)]["route"] == GENERIC
    assert table[(64, 64, 3900, 1)]["route"] == TILE and table[(64, 64, 4097, 1)]["route"] == GENERIC


def test_generic_route_shape(table):
    for M, D, T in SHAPES:
        p = table[(M, D, T, 1)]
        if p["route"] == GENERIC:
            assert p["wg"] == 256 and p["kt"] == 256 and p["lds_bytes"] == 0 and p["span"] == 0


def test_tiles_cover_the_output_times_exactly_once_and_the_grid_limit_refuses(table, planner):
    for (M, D, T, n), p in table.items():
        blocks, kt, wg = p["blocks"], p["kt"], p["wg"]
        assert (blocks - 1) * kt < n <= blocks * kt, (M, D, T, n)
        assert bool(p["ok"]) == (blocks * wg <= THREAD_LIMIT), (M, D, T, n, p)
    edges = []
    for shape in [(16, 8, 127), (64, 32, 512), (64, 64, 512), (16, 5, 127)]:
        p = table[shape + (1,)]
        most = THREAD_LIMIT // p["wg"] * p["kt"]      # output times of the largest grid
        edges += [shape + (n,) for n in (most - p["kt"] + 1, most, most + 1, most + p["kt"])]
    for case, p in zip(edges, planner(edges)):
        most = THREAD_LIMIT // p["wg"] * p["kt"]
        assert bool(p["ok"]) == (case[3] <= most), (case, p)
    assert table[(16, 8, 127, 1 << 34)]["ok"] == 0 and table[(16, 8, 127, (1 << 31) + 5)]["ok"] == 1


def test_extents_and_channel_counts(planner):
    """(N - 1) D + T and M N must fit in 63 bits; M is a power of two in [2, 64]."""
    cases = [(16, 8, 127, 1 << 40), (16, 1 << 31, 31, 1 << 33), (16, 8, (1 << 63) - 120, 16),
             (16, 8, (1 << 63) - 121, 16), (64, 1, 1, 1 << 57), (64, 1, 1, (1 << 57) - 1), (16, 8, (1 << 64) - 1, 16)]
    fits = [p["fits"] for p in planner(cases)]
    assert fits == [1, 0, 0, 1, 0, 1, 0]
    valid = [p["valid"] for p in planner([(M, 1, 1, 1) for M in (0, 1, 2, 3, 4, 6, 8, 12, 16, 32, 48, 64, 96, 128, 1 << 31)])]
    assert valid == [0, 0, 1, 0, 1, 0, 1, 0, 1, 1, 0, 1, 0, 0, 0]


def test_plan_under_the_sanitizers(tmp_path, table):
    """The same stand-alone program built with -fsanitize=address,undefined (where the host compiler has the
    runtimes) plans every case identically and reports nothing."""
    probe = tmp_path / "probe.cpp"
    probe.write_text("int main() { return 0; }\n")
    flags = ("-fsanitize=address,undefined", "-fno-sanitize-recover=undefined")
    r = subprocess.run(["g++", *flags, str(probe), "-o", str(tmp_path / "probe")], capture_output=True, text=True)
    if r.returncode != 0:
        pytest.skip("the host compiler has no address / undefined-behaviour sanitizer runtime")
    run = build_plan_program(tmp_path, flags)
    cases = list(table)
    assert run(cases) == [table[c] for c in cases]
