"""CPU: the IIR launch plan (gsdr_amd/csrc/iir_plan.hpp, HIP-free) compiled into a small host program, and what its
numbers must satisfy for iir.hip to be safe: the scan levels, a workspace whose regions do not overlap and are
aligned for their element types, a route on which every scan level is run by exactly one kernel within that kernel's
limits, and the tile count with its refusal bound. The checks are invariants of the layout and the route, not a
second copy of the formulas; the sizes run from one sample to 2^40, around every level and route threshold."""
import json
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "gsdr_amd", "csrc")

PROGRAM = r"""
#include <cinttypes>
#include <cstdio>

#include "iir_plan.hpp"

static void list(const char* name, const uint64_t* v, int count) {
  std::printf(",\"%s\":[", name);
  for (int i = 0; i < count; ++i) std::printf("%s%" PRIu64, i ? "," : "", v[i]);
  std::printf("]");
}

int main() {
  uint64_t n, acc, sample;
  int P, fused;
  while (std::scanf("%" SCNu64 " %d %" SCNu64 " %" SCNu64 " %d", &n, &P, &acc, &sample, &fused) == 5) {
    gsdr::iir::ScanPlan p{};
    const bool ok = gsdr::iir::scan_plan(n, P, (size_t)acc, (size_t)sample, fused != 0, &p);
    std::printf("{\"ok\":%d", ok ? 1 : 0);
    if (ok) {
      const int nl = p.levels + 1;
      uint64_t elems[gsdr::iir::kMaxLevels + 1], starts[gsdr::iir::kMaxLevels + 1];
      for (int k = 0; k < nl; ++k) {
        elems[k] = p.elems[k];
        starts[k] = p.starts[k];
      }
      std::printf(",\"levels\":%d", p.levels);
      list("E", p.E, nl);
      list("elems", elems, nl);
      list("starts", starts, nl);
      std::printf(",\"tables\":%zu,\"table_bytes\":%zu,\"s0\":%zu,\"xh_copy\":%zu,\"bytes\":%zu", p.tables,
                  p.table_bytes, p.s0, p.xh_copy, p.bytes);
      std::printf(",\"ntiles\":%" PRIu64 ",\"lowest\":%d,\"rest\":%d,\"upper\":%d", p.ntiles, p.lowest, p.rest,
                  p.upper ? 1 : 0);
    }
    std::printf("}\n");
  }
  return 0;
}
"""

CHUNK, GROUP, REST_GROUPS, UPPER_E2, TILE_BYTES, DOUBLE = 32, 64, 16, 256, 16384, 8
SIZES = [1, 31, 32, 33, 2048, 2049, 4096, 4097, 131072, 131073, 1 << 25, (1 << 25) + 1, (1 << 31) + 5, 1 << 40]
STATES = [1, 2, 4, 8, 16, 31]              # compiled state sizes P
SAMPLES = [(8, 4), (16, 8)]                # (sizeof accumulator, sizeof sample): real, complex
FIRST_REFUSED_TILES = (1 << 31) - 1


def ceil_div(a, b):
    return -(-a // b)


def shapes():
    return [(P, acc, sample, fused) for P in STATES for acc, sample in SAMPLES for fused in (False, True)]


@pytest.fixture(scope="module")
def plan(tmp_path_factory):
    """plan(n, P, acc, sample, fused) -> the ScanPlan's fields (a dict), or None when scan_plan refuses the call; every
    case of this module is planned by one run of the program."""
    d = tmp_path_factory.mktemp("iir_plan")
    src = d / "plan.cpp"
    src.write_text(PROGRAM)
    exe = d / "plan"
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-I" + CSRC, str(src), "-o", str(exe)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    cases = []
    for shape in shapes():
        tile = TILE_BYTES // shape[2]
        edge = (FIRST_REFUSED_TILES - 1) * tile  # the largest accepted tile count, full
        cases += [(n,) + shape for n in SIZES + [edge - tile + 1, edge, edge + 1, edge + tile, edge + tile + 1]]
    text = "".join("%d %d %d %d %d\n" % (n, P, acc, sample, fused) for n, P, acc, sample, fused in cases)
    r = subprocess.run([str(exe)], input=text, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = r.stdout.splitlines()
    assert len(lines) == len(cases)
    table = {}
    for case, line in zip(cases, lines):
        p = json.loads(line)
        table[case] = p if p["ok"] else None
    return lambda n, P, acc, sample, fused: table[(n, P, acc, sample, bool(fused))]


def accepted(plan):
    for shape in shapes():
        for n in SIZES:
            p = plan(n, *shape)
            assert p is not None, (n, shape)
            yield n, shape, p


def test_levels(plan):
    """Level 0 has one element a 32-sample chunk, every level above one element a group of 64 below it, and the
    levels stop at the first one that is a single group."""
    for n, shape, p in accepted(plan):
        E, levels = p["E"], p["levels"]
        assert len(E) == levels + 1 and E[0] == ceil_div(n, CHUNK), (n, shape)
        for k in range(levels):
            assert E[k + 1] == ceil_div(E[k], GROUP), (n, shape, k)
        assert 1 <= E[levels] <= GROUP, (n, shape)
        assert levels == 0 or E[levels - 1] > GROUP, (n, shape)
    assert plan(2048, 4, 8, 4, True)["levels"] == 0 and plan(2049, 4, 8, 4, True)["levels"] == 1
    assert plan(131072, 4, 8, 4, True)["levels"] == 1 and plan(131073, 4, 8, 4, True)["levels"] == 2


def test_workspace_regions_are_disjoint_and_aligned(plan):
    """Per level the elements and their start states (E[k] P accumulators each), levels + 1 tables of 64 P x P
    doubles, the entry state (P accumulators) and the copy of the input history (P samples): each inside
    [0, bytes), aligned to its element size, and no two overlapping."""
    for n, (P, acc, sample, fused), p in accepted(plan):
        where = (n, P, acc, sample, fused)
        regions = []
        for k in range(p["levels"] + 1):
            regions.append((f"elems[{k}]", p["elems"][k], p["E"][k] * P * acc, acc))
            regions.append((f"starts[{k}]", p["starts"][k], p["E"][k] * P * acc, acc))
            regions.append((f"table[{k}]", p["tables"] + k * p["table_bytes"], GROUP * P * P * DOUBLE, DOUBLE))
        regions.append(("s0", p["s0"], P * acc, acc))
        regions.append(("xh_copy", p["xh_copy"], P * sample, sample))
        for name, start, size, align in regions:
            assert size > 0 and start % align == 0 and 0 <= start and start + size <= p["bytes"], (where, name)
        regions.sort(key=lambda r: r[1])
        for (name_a, start_a, size_a, _), (name_b, start_b, _, _) in zip(regions, regions[1:]):
            assert start_a + size_a <= start_b, (where, name_a, name_b)


def test_every_level_has_exactly_one_owner(plan):
    """Levels [lowest, levels] (lowest = 1 when the chunk passes scan level 0 themselves) are each run by exactly one
    of: a launch per sweep [lowest, rest), the single-workgroup k_iir_scan_rest [rest, levels], or -- `upper` --
    level 1's up-sweep with k_iir_scan_upper for everything above. k_iir_scan_rest walks its levels with 16 waves,
    one group each a round, and is only given levels of at most 16 groups; k_iir_scan_upper holds one level-2 group a
    wave (256 elements) and reads the tables of levels 1..3 only."""
    for n, (P, acc, sample, fused), p in accepted(plan):
        where = (n, P, acc, sample, fused)
        E, levels, lowest, rest, upper = p["E"], p["levels"], p["lowest"], p["rest"], bool(p["upper"])
        assert lowest == (1 if fused else 0), where
        assert lowest <= rest, where
        if lowest <= levels:
            assert rest <= levels, where
        else:
            # one group of chunks, scanned inside the fused chunk passes: no level is left, and rest = lowest = 1 >
            # levels = 0 is what makes the launcher (iir.hip run(): `if (pl.rest <= pl.levels)`) skip k_iir_scan_rest
            assert fused and levels == 0 and rest == lowest and not upper, where
        per_level = [] if upper else list(range(lowest, rest))
        by_rest = [] if upper else list(range(rest, levels + 1))
        by_upper = list(range(1, levels + 1)) if upper else []
        owned = sorted(per_level + by_rest + by_upper)
        assert owned == list(range(lowest, levels + 1)), (where, per_level, by_rest, by_upper)
        for k in by_rest:
            assert ceil_div(E[k], GROUP) <= REST_GROUPS, (where, k)
        if upper:
            assert fused and 2 <= levels <= 3 and E[2] <= UPPER_E2, where
    for P, acc, sample, _ in shapes():
        assert plan(1 << 25, P, acc, sample, True)["upper"] == 1, (P, acc)
        assert plan((1 << 25) + 1, P, acc, sample, True)["upper"] == 0, (P, acc)
        assert plan(1 << 25, P, acc, sample, False)["upper"] == 0, (P, acc)


def test_tiles_and_refusal(plan):
    """One workgroup a chunk-pass tile of 16 KiB of samples; a grid takes fewer than 2^31 - 1 of them, and the call is
    refused from exactly that many tiles on."""
    for n, (P, acc, sample, fused), p in accepted(plan):
        assert p["ntiles"] == ceil_div(n, TILE_BYTES // sample), (n, sample)
    for shape in shapes():
        tile = TILE_BYTES // shape[2]
        edge = (FIRST_REFUSED_TILES - 1) * tile
        for n in (edge - tile + 1, edge):
            p = plan(n, *shape)
            assert p is not None and p["ntiles"] == FIRST_REFUSED_TILES - 1, (n, shape)
        for n in (edge + 1, edge + tile, edge + tile + 1):
            assert plan(n, *shape) is None, (n, shape)
