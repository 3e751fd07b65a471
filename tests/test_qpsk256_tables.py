"""CPU: what gsdrQpsk256InitConstellation computes on the host (gsdr_amd/csrc/qpsk256_tables.hpp, HIP-free) compiled into
a small host program: the 256-point tables bit for bit against the oracle, the encoding of the circular table's
per-cell candidate lists, and the claim the circular demodulation kernel relies on -- for every received point on the
grid, in the cell the kernel's own float32 arithmetic puts it in, the reference's exhaustive cuCabsf argmin is on that
cell's list (and is the point of a one-point cell)."""
import json
import os
import struct
import subprocess

import numpy as np
import pytest

from oracle import oracle as o

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "gsdr_amd", "csrc")
GRID, LIST_BYTES, SPAN = 96, 4096, 1.3

# One line a case: the table's 512 floats as bits, R and inv_cs as bits, the 96 x 96 cell words, and the list bytes
# build_cells wrote. The lists are built twice over images pre-filled with 0x00 and 0xff: `used` is the first list
# byte the two runs left different, `tail_untouched` that no byte from there on was written, `cells_equal` that every
# cell word was written (both only meaningful when R > 0).
PROGRAM = r"""
#include <cstddef>
#include <cstdio>
#include <cstring>

#include "qpsk256_tables.hpp"

struct Pt {
  float x, y;
};
static_assert(sizeof(Pt) == 8 && offsetof(Pt, x) == 0 && offsetof(Pt, y) == 4, "float2's layout");

static unsigned bits(float v) {
  unsigned u;
  std::memcpy(&u, &v, 4);
  return u;
}

int main() {
  unsigned type, abits;
  static gsdr::CircCells a, b;
  while (std::scanf("%u %x", &type, &abits) == 2) {
    float amplitude;
    std::memcpy(&amplitude, &abits, 4);
    Pt t[256];
    gsdr::build_table(type, amplitude, t);
    std::memset(&a, 0x00, sizeof(a));
    std::memset(&b, 0xff, sizeof(b));
    gsdr::build_cells(t, &a);
    gsdr::build_cells(t, &b);
    int used = 0;
    while (used < gsdr::kCellListBytes && a.lists[used] == b.lists[used]) ++used;
    int untouched = 1, cells_equal = 1;
    for (int i = used; i < gsdr::kCellListBytes; ++i) untouched &= a.lists[i] == 0x00 && b.lists[i] == 0xff;
    for (int i = 0; i < gsdr::kCellGrid * gsdr::kCellGrid; ++i) cells_equal &= a.cell[i] == b.cell[i];
    std::printf("{\"table\": [");
    for (int i = 0; i < 256; ++i) std::printf("%s%u, %u", i ? ", " : "", bits(t[i].x), bits(t[i].y));
    std::printf("], \"R\": %u, \"inv_cs\": %u, \"R_b\": %u, \"used\": %d, \"tail_untouched\": %d, \"cells_equal\": %d, \"cells\": [",
                bits(a.R), bits(a.inv_cs), bits(b.R), used, untouched, cells_equal);
    for (int i = 0; i < gsdr::kCellGrid * gsdr::kCellGrid; ++i) std::printf("%s%u", i ? ", " : "", (unsigned)a.cell[i]);
    std::printf("], \"lists\": [");
    for (int i = 0; i < used; ++i) std::printf("%s%u", i ? ", " : "", (unsigned)a.lists[i]);
    std::printf("]}\n");
  }
  return 0;
}
"""

AMPLITUDES = [1.0, 0.5, 2.5, 0.37, 3.0, -2.5]          # the amplitudes the GPU tests use
STRUCTURE = [1.0, 0.37, -2.5]
DEGENERATE = [0.0, float("inf"), float("nan")]
EXTREME = [1e-20, 1e20]
CASES = [(t, a) for t in (0, 1) for a in AMPLITUDES] + [(1, a) for a in DEGENERATE + EXTREME] + [(0, 0.0), (0, float("nan"))]


def f32_bits(v):
    return struct.unpack("<I", struct.pack("<f", v))[0]


def build_tables_program(directory, extra_flags=()):
    """Compiles qpsk256_tables.hpp into a host program in `directory`; returns run(cases) -> one dict a case
    (type, amplitude), in order."""
    src = os.path.join(str(directory), "qpsk256_tables.cpp")
    exe = os.path.join(str(directory), "qpsk256_tables" +
                       ("_" + "".join(c for c in "".join(extra_flags) if c.isalnum()) if extra_flags else ""))
    with open(src, "w") as f:
        f.write(PROGRAM)
    r = subprocess.run(["g++", "-std=c++17", "-ffp-contract=off", "-O1", "-Wall", "-Wextra", *extra_flags, "-I" + CSRC, src,
                        "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]

    def run(cases):
        text = "".join("%d %x\n" % (t, f32_bits(a)) for t, a in cases)
        out = subprocess.run([exe], input=text, capture_output=True, text=True)
        assert out.returncode == 0 and out.stderr == "", (out.returncode, out.stderr[-3000:])
        lines = out.stdout.splitlines()
        assert len(lines) == len(cases)
        return lines

    return run


@pytest.fixture(scope="module")
def raw(tmp_path_factory):
    return build_tables_program(tmp_path_factory.mktemp("qpsk256_tables"))(CASES)


@pytest.fixture(scope="module")
def built(raw):
    return {(t, f32_bits(a)): json.loads(line) for (t, a), line in zip(CASES, raw)}


def case(built, ctype, amp):
    return built[(ctype, f32_bits(amp))]


def as_f32(bits):
    return np.array([bits], dtype=np.uint32).view(np.float32)[0]


@pytest.mark.parametrize("ctype", [0, 1])
@pytest.mark.parametrize("amp", AMPLITUDES)
def test_table_bits_equal_the_oracle(built, ctype, amp):
    got = np.array(case(built, ctype, amp)["table"], dtype=np.uint32)
    want = o.qpsk256_table(ctype, amp).view(np.uint32)
    assert np.array_equal(got, want)


def check_structure(c, table):
    """The encoding of a built cell structure; returns (cell lengths, cell fields, list bytes)."""
    rmax = np.hypot(table.real.astype(np.float64), table.imag.astype(np.float64)).max()
    R = np.float32(rmax * SPAN)
    inv_cs = np.float32(GRID) / (np.float32(2.0) * R)
    assert type(inv_cs) is np.float32
    assert c["R"] == f32_bits(R) and c["inv_cs"] == f32_bits(inv_cs) and c["R_b"] == c["R"]
    assert c["cells_equal"] == 1 and c["tail_untouched"] == 1
    words = np.array(c["cells"], dtype=np.uint32)
    lists = np.array(c["lists"], dtype=np.uint8)
    used = c["used"]
    assert words.size == GRID * GRID and np.all(words < 1 << 16) and lists.size == used <= LIST_BYTES
    length, field = words >> 12, words & 0xFFF
    assert length.min() >= 1 and length.max() <= 15
    assert np.all(field[length == 1] < 256)
    longer = length > 1
    assert np.all(field[longer] + length[longer] <= used)
    distinct = {}
    for off, n in set(zip(field[longer].tolist(), length[longer].tolist())):
        entries = lists[off:off + n]
        assert np.all(np.diff(entries.astype(np.int32)) > 0), (off, n)      # strictly ascending
        assert distinct.setdefault(entries.tobytes(), off) == off, (off, n)   # identical lists are stored once
    # the lists tile the used bytes: nothing is stored that no cell points to
    assert sum(len(k) for k in distinct) == used
    return length, field, lists


@pytest.mark.parametrize("amp", STRUCTURE)
def test_cell_structure_and_the_documented_counts(built, amp):
    c = case(built, 1, amp)
    length, field, _ = check_structure(c, o.qpsk256_table(1, amp))
    longer = length > 1
    counts = (int((length == 1).sum()), int(longer.sum()),
              len(set(zip(field[longer].tolist(), length[longer].tolist()))), c["used"])
    print("one-point cells, longer lists, distinct lists, list bytes:", counts)
    # the figures the comment of CircCells and DESIGN.md section 3.7 state ("at any amplitude")
    assert counts == (2863, 6353, 1078, 3293)


def membership(c):
    """member[cell, p]: point p is on the cell's list; and the cells' lengths."""
    words = np.array(c["cells"], dtype=np.uint32)
    lists = np.array(c["lists"], dtype=np.uint8)
    length, field = words >> 12, words & 0xFFF
    member = np.zeros((GRID * GRID, 256), dtype=bool)
    one = length == 1
    member[np.nonzero(one)[0], field[one]] = True
    for cell in np.nonzero(~one)[0]:
        member[cell, lists[field[cell]:field[cell] + length[cell]]] = True
    assert np.array_equal(member.sum(axis=1), length)
    return member, length, field


def ulp_neighbours(v):
    """v and the float32 values 1 and 2 ulp on either side."""
    out = [v]
    for toward in (np.float32(np.inf), np.float32(-np.inf)):
        w = v
        for _ in range(2):
            w = np.nextafter(w, toward)
            out.append(w)
    return np.concatenate(out)


def coverage_points(R, inv_cs, seed):
    """float32 points: 200,000 uniform over a square 5 % larger than [-R, R)^2, and points at 0, +-1 and +-2 ulp around
    every cell edge along a few rows and columns (and on the diagonal, where both coordinates sit at an edge)."""
    rng = np.random.default_rng(seed)
    half = np.float32(1.05) * R
    uni = (rng.random((200_000, 2), dtype=np.float32) * np.float32(2.0) - np.float32(1.0)) * half
    cs = np.float64(1.0) / np.float64(inv_cs)
    edges = ulp_neighbours((-np.float64(R) + np.arange(GRID + 1) * cs).astype(np.float32))
    # a few rows / columns: mid-cell coordinates of cells 0, 17, 48, 95 and two arbitrary in-cell offsets
    along = ((np.array([0.5, 17.5, 48.5, 95.5, 30.13, 71.77]) * cs) - np.float64(R)).astype(np.float32)
    a, b = np.meshgrid(edges, along, indexing="ij")
    rows = np.stack([a.ravel(), b.ravel()], axis=1)
    cols = rows[:, ::-1]
    per_edge = edges.reshape(5, GRID + 1)
    da, db = np.meshgrid(np.arange(5), np.arange(5), indexing="ij")
    diag = np.stack([per_edge[da.ravel()].ravel(), per_edge[db.ravel()].ravel()], axis=1)
    pts = np.concatenate([uni, rows, cols, diag]).astype(np.float32)
    assert pts.dtype == np.float32
    return pts, uni.shape[0]


@pytest.mark.parametrize("amp", STRUCTURE)
def test_every_cell_list_holds_the_reference_argmin_of_every_point_in_the_cell(built, amp):
    c = case(built, 1, amp)
    table = o.qpsk256_table(1, amp)
    member, length, field = membership(c)
    R, inv_cs = as_f32(c["R"]), as_f32(c["inv_cs"])
    assert R > 0
    pts, n_uniform = coverage_points(R, inv_cs, seed=0xC256 + STRUCTURE.index(amp))
    # the kernel's cell of a point, in float32: (int)((r.x + R) * inv_cs), on the grid when both are in [0, 96)
    fx = (pts[:, 0] + R) * inv_cs
    fy = (pts[:, 1] + R) * inv_cs
    assert fx.dtype == np.float32 and fy.dtype == np.float32
    on = (fx >= 0) & (fy >= 0) & (fx < np.float32(GRID)) & (fy < np.float32(GRID))
    cell = fy[on].astype(np.int32) * GRID + fx[on].astype(np.int32)
    # both sides of the grid's border are exercised, and every cell is hit
    assert n_uniform >= 200_000 and 0.85 < on[:n_uniform].mean() < 0.95 and (~on[n_uniform:]).any()
    assert np.unique(cell).size == GRID * GRID
    want = o.qpsk256_demod(table, pts[on, 0] + 1j * pts[on, 1], rule="cuabs", nthreads=4)
    listed = member[cell, want]
    assert listed.all(), (int((~listed).sum()), pts[on][~listed][:4], cell[~listed][:4], want[~listed][:4])
    one = length[cell] == 1
    assert one.any() and np.array_equal(field[cell][one], want[one])


@pytest.mark.parametrize("amp", DEGENERATE)
def test_degenerate_tables_disable_the_lookup(built, amp):
    c = case(built, 1, amp)
    assert c["R"] == 0 and c["R_b"] == 0
    assert c["used"] == 0 or c["tail_untouched"] == 1


@pytest.mark.parametrize("amp", EXTREME)
def test_extreme_amplitudes_disable_the_lookup_or_build_all_of_it(built, amp):
    c = case(built, 1, amp)
    print("amplitude", amp, "R bits", c["R"], "list bytes", c["used"])
    if c["R"] == 0:
        assert c["R_b"] == 0
    else:
        check_structure(c, o.qpsk256_table(1, amp))


def test_tables_under_the_sanitizers(tmp_path, raw):
    """The same stand-alone program built with -fsanitize=address,undefined (nothing preloaded) writes the same
    output for every case and reports nothing."""
    flags = ("-fsanitize=address,undefined", "-fno-sanitize-recover=undefined")
    assert build_tables_program(tmp_path, flags)(CASES) == raw
