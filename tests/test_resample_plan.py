"""CPU: the resampler's launch plan (gsdr_amd/csrc/resample_plan.hpp, HIP-free) compiled into a small host program,
and what its numbers must satisfy for resample.hip to be safe: a tiled route whose LDS stays within the budget and
whose span covers a tile from every start, tiles that cover [0, N) exactly once, a route that depends on the filter's
shape alone, and a refusal where one launch cannot hold the grid. The checks are invariants, not a second copy of
the formulas; the sizes run from one output to 2^40, around every threshold."""
import subprocess

import pytest

from resample_ref import build_plan_program

BUDGET = 64 * 1024
R = 8                                  # outputs per thread of the tiled kernel
THREAD_LIMIT = (1 << 32) - 1           # blocks * threads of one launch
TILE, GENERIC = 0, 1
SAMPLES = (4, 8)                       # sizeof float, float2

# (L, M, T): the GPU tests' shapes, the issue's generic-route shapes, and shapes on both sides of the LDS budget
SHAPES = [(L, M, T) for L, M in [(2, 1), (4, 1), (3, 2), (2, 3), (5, 6), (24, 125), (125, 24), (147, 160), (160, 147),
                                 (7, 3)] for T in (1, max(1, L - 1), L, 4 * L + 3, 16 * L)]
SHAPES += [(24, 125, 769), (160, 147, 1601), (5, 6, 121), (4, 1, 65), (4096, 4099, 8192), (3, 2, 20000),
           (2, 100001, 7), (3, 2, 16380), (3, 2, 16381), (3, 2, 16384), (3, 2, 16385), (2, 15, 7), (2, 16, 7), (2, 31, 7), (2, 63, 7), (2, 127, 7),
           (2, 255, 7), (2, 1023, 7), ((1 << 31) - 1, 3, 5), (1 << 31, 3, 5), (5, (1 << 31) - 1, 3), (5, 1 << 31, 3),
           ((1 << 32) - 1, (1 << 32) - 1, 1), (1, 4, 127), (1000003, 1000033, 4001)]
SIZES = [1, 2, 63, 64, 255, 256, 257, 511, 512, 513, 1023, 1024, 1025, 4096, 4097, 1 << 20, (1 << 24) + 5, (1 << 31) + 5,
         1 << 32, (1 << 34) - 1, 1 << 34, 1 << 36, 1 << 40]


@pytest.fixture(scope="module")
def planner(tmp_path_factory):
    return build_plan_program(tmp_path_factory.mktemp("resample_plan"))


@pytest.fixture(scope="module")
def table(planner):
    """(L, M, T, sample, n) -> the plan's fields, every case of this module planned by one run of the program."""
    cases = [(L, M, T, sz, n) for L, M, T in SHAPES for sz in SAMPLES for n in SIZES]
    return dict(zip(cases, planner(cases)))


def windows(L, M, T, start, kt):
    """Input samples outputs [0, kt) need when output 0's window starts at zero-stuffed index `start`: from the
    first output's first sample through ceil(T / L) samples of the last output's."""
    first = -(-start // L)
    last = -(-(start + (kt - 1) * M) // L)
    return last - first + -(-T // L)


def test_route_depends_on_the_shape_alone(table):
    for L, M, T in SHAPES:
        for sz in SAMPLES:
            plans = [table[(L, M, T, sz, n)] for n in SIZES]
            for key in ("route", "wg", "kt", "span", "lds_bytes"):   # (the phase is not even an argument)
                assert len({p[key] for p in plans}) == 1, (L, M, T, sz, key)
    by = {(L, M, T, sz): table[(L, M, T, sz, 1)]["route"] for L, M, T in SHAPES for sz in SAMPLES}
    for sz in SAMPLES:
        assert by[(3, 2, 20000, sz)] == GENERIC     # 80 KB of taps
        assert by[(2, 100001, 7, sz)] == GENERIC    # ~50,000 input samples an output
        assert by[(3, 2, 16385, sz)] == GENERIC     # one tap more than 64 KB
        assert by[(1 << 31, 3, 5, sz)] == GENERIC and by[(5, 1 << 31, 3, sz)] == GENERIC   # 32-bit tile indices
        for shape in [(24, 125, 769), (160, 147, 1601), (5, 6, 121), (4, 1, 65), (4096, 4099, 8192), (7, 3, 6)]:
            assert by[shape + (sz,)] == TILE, shape


def test_tiled_route_fits_the_lds_budget_and_its_span_covers_every_tile_start(table):
    """The LDS of a tiled launch holds the span (plus the slack that lets the kernel keep a sample's offset inside
    its 16-byte granule: one granule less one sample) and the taps (plus 3 floats of the same slack), each
    rounded to 16 bytes, within 64 KB; the span is at least what a tile needs from any start s mod L (every start
    for small L, the extremes and a spread for large L), and some start needs exactly that much."""
    seen = 0
    for L, M, T in SHAPES:
        for sz in SAMPLES:
            p = table[(L, M, T, sz, 1)]
            if p["route"] != TILE:
                continue
            seen += 1
            kt, wg, span = p["kt"], p["wg"], p["span"]
            assert kt == R * wg and wg in (64, 128, 256), (L, M, T, sz)
            assert wg % 64 == 0
            g = 16 // sz
            need = -(-(span + g - 1) * sz // 16) * 16 + -(-(T + 3) * 4 // 16) * 16
            assert need <= p["lds_bytes"] <= BUDGET, (L, M, T, sz, p)
            assert L + kt * M < 1 << 32, (L, M, T, sz)     # the kernel's 32-bit r0 + k M
            starts = range(L) if L <= 4096 else [0, 1, 2, L // 3, L // 2, L - 2, L - 1]
            worst = max(windows(L, M, T, s, kt) for s in starts)
            assert worst <= span, (L, M, T, sz, worst, span)
            if L <= 4096:
                assert worst == span, (L, M, T, sz, worst, span)   # no LDS is planned that no tile can use
            # a larger tile, had there been one, would not have fit
            if wg < 256:
                big = windows(L, M, T, 1 % L, 2 * kt)
                assert (big + g - 1) * sz + (T + 3) * 4 > BUDGET - 32 or 2 * kt * M >= 1 << 31, (L, M, T, sz)
    assert seen >= 2 * 50


def test_generic_route_is_taken_only_where_no_tile_fits(table):
    for L, M, T in SHAPES:
        for sz in SAMPLES:
            p = table[(L, M, T, sz, 1)]
            if p["route"] != GENERIC:
                continue
            assert p["wg"] == 256 and p["kt"] == 256, (L, M, T, sz)
            smallest = windows(L, M, T, 1 % L, R * 64)
            too_big = smallest * sz + T * 4 > BUDGET - 64 or T > BUDGET // 4
            too_wide = L >= 1 << 31 or R * 64 * M >= 1 << 31
            assert too_big or too_wide, (L, M, T, sz)


def test_tiles_cover_the_outputs_exactly_once_and_the_grid_limit_refuses(table, planner):
    for (L, M, T, sz, n), p in table.items():
        blocks, kt, wg = p["blocks"], p["kt"], p["wg"]
        # workgroup b owns outputs [b kt, min((b + 1) kt, n)): all of [0, n), the last tile not empty
        assert (blocks - 1) * kt < n <= blocks * kt, (L, M, T, sz, n)
        assert bool(p["ok"]) == (blocks * wg <= THREAD_LIMIT), (L, M, T, sz, n, p)
    # the edge itself, for each tile size the shapes produce
    edges = []
    for shape in [(24, 125, 769), (2, 15, 7), (2, 31, 7), (2, 63, 7), (2, 127, 7), (3, 2, 20000)]:
        for sz in SAMPLES:
            p = table[shape + (sz, 1)]
            most = THREAD_LIMIT // p["wg"] * p["kt"]      # outputs of the largest grid
            edges += [shape + (sz, n) for n in (most - p["kt"] + 1, most, most + 1, most + p["kt"])]
    for case, p in zip(edges, planner(edges)):
        most = THREAD_LIMIT // p["wg"] * p["kt"]
        assert bool(p["ok"]) == (case[4] <= most), (case, p)
    tiles = {table[s + (4, 1)]["kt"] for s in SHAPES if table[s + (4, 1)]["route"] == TILE}
    assert tiles == {512, 1024, 2048}    # every tile size is exercised above
    assert table[(24, 125, 769, 4, 1 << 40)]["ok"] == 0 and table[(24, 125, 769, 4, 1 << 32)]["ok"] == 1


def test_plan_under_the_undefined_behaviour_sanitizer(tmp_path, table):
    """The same program built with -fsanitize=undefined (where the host compiler has the runtime) plans every case
    identically and reports nothing."""
    probe = tmp_path / "probe.cpp"
    probe.write_text("int main() { return 0; }\n")
    r = subprocess.run(["g++", "-fsanitize=undefined", "-fno-sanitize-recover=undefined", str(probe), "-o",
                        str(tmp_path / "probe")], capture_output=True, text=True)
    if r.returncode != 0:
        pytest.skip("the host compiler has no undefined-behaviour sanitizer runtime")
    run = build_plan_program(tmp_path, ("-fsanitize=undefined", "-fno-sanitize-recover=undefined"))
    cases = list(table)
    assert run(cases) == [table[c] for c in cases]
