"""The plan of the workgroup-owned XCD-local SpMM at ANY slice count (``owned_plan(..., slices)``,
csrc/dgmi_owned_common.h) and the rule that gives a product's layout its slice count (``dgmi_sliced_layout_slices``,
include/dgmi_layout.h), on the host (no GPU).

A stand-alone C++ program includes the header the kernel and its launcher include.  For 1 / 2 / 3 / 8 / 16 / 64 slices,
every lane-group width, 1 / 3 / 19 / 256 workgroups and 1 / 2 / 4 row rounds it walks every workgroup, phase, task slot
and lane group: every (row, slice, column tile) is covered exactly once; within a round the slices are the innermost
index of a phase and ascend from 0 (the order in which a row's segment sums are joined); a plan of more than
``kOwnedMaxPhases`` phases is refused and no other; the plan made without a slice count is, field by field, the plan of
``kOwnedSlices`` = 8 slices with the phase count today's callers rely on.  The program runs twice, the second time built
with the address and undefined-behaviour sanitizers.

The rule is asked through the C ABI for the shapes of the flagship step, the edges of its 48-64 MiB window and the
``sliced_owned_slices`` knob."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

PROGRAM = r"""
#include <cstdio>
#include <vector>
#include "dgmi_owned_common.h"

using namespace dgmi;

static long long refused = 0, planned = 0;

static int check(int slices, int64_t n_dst, int64_t grid, int64_t F, int lpr, int want_rounds) {
#define FAIL(msg)                                                                                                       \
  do {                                                                                                                  \
    printf("slices %d n_dst %lld grid %lld F %lld lpr %d rounds %d: %s\n", slices, (long long)n_dst, (long long)grid,   \
           (long long)F, lpr, want_rounds, msg);                                                                        \
    return 1;                                                                                                           \
  } while (0)
  const int64_t B = (n_dst + grid - 1) / grid;
  if (B < want_rounds) return 0;
  const int64_t cap = want_rounds == 1 ? 0 : (B + want_rounds - 1) / want_rounds;
  if (cap > 0 && (B + cap - 1) / cap != want_rounds) return 0;  // no cap gives exactly that many rounds
  const int64_t budget_rows = kOwnedLdsRowBytes / (16 * lpr);
  const int64_t fit = cap > 0 && cap < budget_rows ? cap : budget_rows;
  const int64_t rounds = (B + fit - 1) / fit;
  const int col_tiles = (int)((F + 4 * lpr - 1) / (4 * lpr));
  const OwnedPlan p = owned_plan(n_dst, F, lpr, grid, 0, cap, 1, kOwnedPhaseTasks, slices);
  if (rounds * col_tiles * slices > kOwnedMaxPhases) {
    if (p.ok) FAIL("a plan of more than kOwnedMaxPhases phases was not refused");
    ++refused;
    return 0;
  }
  if (!p.ok) FAIL("a plan that fits was refused");
  ++planned;
  if (p.slices != slices) FAIL("the plan does not carry its slice count");
  if (p.row_rounds != rounds || p.col_rounds != col_tiles || p.phases != col_tiles * rounds * slices) FAIL("phases");
  if (p.lds_bytes != (size_t)p.round_rows * 16 * lpr + 4 * ((size_t)p.tasks + p.phases + 2)) FAIL("LDS bytes");
  if (slices == kOwnedSlices) {  // the plan made without a slice count, field by field
    const OwnedPlan q = owned_plan(n_dst, F, lpr, grid, 0, cap);
    if (q.ok != p.ok || q.lpr != p.lpr || q.G != p.G || q.R != p.R || q.col_rounds != p.col_rounds || q.row_rounds != p.row_rounds ||
        q.phases != p.phases || q.slices != p.slices || q.wg_rows != p.wg_rows || q.active != p.active ||
        q.round_rows != p.round_rows || q.tasks != p.tasks || q.n_dst != p.n_dst || q.lds_bytes != p.lds_bytes)
      FAIL("the default slice count does not reproduce the 8-slice plan");
    if (q.phases != q.col_rounds * q.row_rounds * 8) FAIL("the default plan's phases");
  }
  std::vector<int> covered((size_t)n_dst * slices * col_tiles, 0);
  for (int64_t wg = 0; wg < grid + 1; ++wg) {
    const int T = owned_wg_tasks(p, wg);
    if ((T == 0) != (wg >= p.active)) FAIL("workgroups without rows must have no tasks, the others some");
    if (T == 0) continue;
    for (int P = 0; P < p.phases; ++P) {
      const OwnedPhase ph = owned_phase(p, P);
      // slices innermost and ascending: phase P is slice P % slices of round P / slices
      if (ph.slice != P % slices || ph.col_round != P / slices / p.row_rounds || ph.row_round != P / slices % p.row_rounds)
        FAIL("phase decoding");
      if (ph.slice > 0) {
        const OwnedPhase prev = owned_phase(p, P - 1);
        if (prev.col_round != ph.col_round || prev.row_round != ph.row_round || prev.slice != ph.slice - 1)
          FAIL("the slices of a round are not consecutive phases in ascending order");
      } else if (P > 0 && owned_phase(p, P - 1).slice != slices - 1) {
        FAIL("a round does not end with the last slice");
      }
      for (int t = 0; t < T; ++t)
        for (int g = 0; g < p.G; ++g) {
          const OwnedTask k = owned_task(p, wg, ph.row_round, t, g);
          if (k.rows < 0 || k.rows > p.R) FAIL("rows of a lane group");
          if (k.rows > 0 && (k.row0 < wg * B || k.row0 + k.rows > (wg + 1) * B || k.row0 + k.rows > n_dst)) FAIL("rows outside the workgroup's block");
          if (k.rows > 0 && k.lds_row + k.rows > p.round_rows) FAIL("LDS row outside the round");
          for (int r = 0; r < k.rows; ++r) ++covered[((size_t)(k.row0 + r) * slices + ph.slice) * col_tiles + ph.col_round];
        }
    }
  }
  for (int c : covered)
    if (c != 1) FAIL(c == 0 ? "a (row, slice, column tile) is not covered" : "a (row, slice, column tile) is covered twice");
  return 0;
#undef FAIL
}

int main() {
  const int slice_counts[] = {1, 2, 3, 8, 16, 64};
  const int64_t rows[] = {307, 5003};
  const int64_t grids[] = {1, 3, 19, 256};
  const int widths[] = {8, 16, 32, 64};
  const int64_t Fs[] = {128, 344};
  const int round_counts[] = {1, 2, 4};
  for (int slices : slice_counts)
    for (int64_t n : rows)
      for (int64_t grid : grids)
        for (int lpr : widths)
          for (int64_t F : Fs)
            for (int rounds : round_counts)
              if (check(slices, n, grid, F, lpr, rounds)) return 1;
  // slice counts the layout builders do not make
  if (owned_plan(307, 128, 32, 3, 0, 0, 1, kOwnedPhaseTasks, 0).ok || owned_plan(307, 128, 32, 3, 0, 0, 1, kOwnedPhaseTasks, 65).ok ||
      owned_plan(307, 128, 32, 3, 0, 0, 1, kOwnedPhaseTasks, -8).ok) {
    printf("a slice count outside 1 .. 64 was planned\n");
    return 1;
  }
  // the flagship class: 100 000 sources -> 50 000 rows on 16 slices is the plan of 50 000 -> 100 000 on 8
  const OwnedPlan a = owned_plan(50000, 128, 32, 256, 0, 0, 1, kOwnedPhaseTasks, 16), b = owned_plan(100000, 128, 32, 256, 0, 0);
  if (!a.ok || !b.ok || a.phases != 16 || b.phases != 16 || a.row_rounds != 1 || b.row_rounds != 2 || a.round_rows != 196 ||
      b.round_rows != 196 || a.R != b.R || a.tasks != b.tasks || a.R != 4 || a.tasks != 25) {
    printf("the 16-slice plan of the flagship class: phases %d / %d rounds %d / %d LDS rows %d / %d R %d / %d tasks %d / %d\n", a.phases,
           b.phases, a.row_rounds, b.row_rounds, a.round_rows, b.round_rows, a.R, b.R, a.tasks, b.tasks);
    return 1;
  }
  printf("ok planned %lld refused %lld\n", planned, refused);
  return 0;
}
"""


def _run_program(tmp_path, tag, extra):
    src, exe = tmp_path / ("owned_slices_%s.cpp" % tag), tmp_path / ("owned_slices_%s" % tag)
    src.write_text(PROGRAM)
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    cmd = [hipcc, "-x", "hip", "--cuda-host-only", "-O1", "-g", "-std=c++17", "-I" + os.path.join(ROOT, "include"),
           "-I" + os.path.join(ROOT, "dream_gnn_amd", "csrc")] + extra + [str(src), "-o", str(exe)]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-4000:]
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    return r.stdout.strip()


def test_owned_plan_of_any_slice_count_covers_every_segment_once_in_slice_order(tmp_path):
    out = _run_program(tmp_path, "plain", [])
    assert out.startswith("ok planned "), out
    planned, refused = int(out.split()[2]), int(out.split()[4])
    assert planned > 400 and refused > 100, out  # both sides of the 128-phase bound are walked
    # the same walk with the sanitizers on (host code only): same counts, no report
    assert _run_program(tmp_path, "san", ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"]) == out


KNOBS = dict(sliced_owned=-1, sliced_owned_slices=0, sliced_owned_grid=0, sliced_owned_rows=0, sliced_owned_lds_rows=0,
             sliced_lpr=0, sliced_chunk_rows=0)


@pytest.fixture
def knobs():
    from dream_gnn_amd import _lib

    def set_knobs(**kw):
        for name, value in dict(KNOBS, **kw).items():
            _lib.set_tuning(name, value)

    set_knobs()
    try:
        yield set_knobs
    finally:
        set_knobs()


MIB = 1 << 20


def test_layout_rule_names_one_class(knobs):
    """Config 4 at F = 128: the two 100 000-source GCMC products get 16 slices, the other two and both kNN-64 products 8;
    the window is 48-64 MiB of table, both ends included."""
    from dream_gnn_amd import _lib

    f = _lib.sliced_layout_slices
    nd, ns = 100_000, 50_000
    assert f(ns, nd, 128) == 16           # gcmc_fwd drug->disease, gcmc_bwd disease->drug: rows = diseases, sources = drugs
    assert f(nd, ns, 128) == 8            # gcmc_fwd disease->drug, gcmc_bwd drug->disease
    assert f(nd, nd, 128, True) == 8 and f(ns, ns, 128, True) == 8   # kNN-64 (multiplicities in the ids)
    assert f(nd, nd, 128, False) == 8 and f(ns, ns, 128, False) == 8  # the same shapes with unit values: two row rounds / a 24 MiB table
    assert f(ns, nd, 128, True) == 8      # the class is one of unit values
    # the window, at 512 B per source row
    assert 98_304 * 512 == 48 * MIB and 131_072 * 512 == 64 * MIB
    assert f(ns, 98_304, 128) == 16 and f(ns, 98_303, 128) == 8
    assert f(ns, 131_072, 128) == 16 and f(ns, 131_073, 128) == 8
    # the same graph at other widths: a 98 MiB / 24 MiB table is outside the window
    assert f(ns, nd, 256) == 8 and f(ns, nd, 64) == 8
    # inside the window at F = 256 (56 000 sources, 55 MiB): a slice of 3.4 MiB fits an L2 at full width, one column
    # round, 196 LDS rows of 1 KiB fit too (144 of them do not: two row rounds) -> not the class
    assert f(ns, 56_000, 256) == 8
    # below the row count at which a workgroup has enough tasks per phase, and arguments the product refuses
    assert f(32_767, nd, 128) == 8 and f(32_768, nd, 128) == 16
    assert f(0, nd, 128) == 8 and f(ns, 0, 128) == 8 and f(ns, nd, 0) == 8 and f(ns, nd, 126) == 8 and f(-1, -1, -1) == 8
    # row rounds: 50 000 rows on 256 workgroups are 196 LDS rows (one round of 288); 80 000 rows are 313 (two rounds)
    assert f(73_728, nd, 128) == 16 and f(73_729, nd, 128) == 8


def test_layout_rule_under_the_knobs(knobs):
    from dream_gnn_amd import _lib

    f = _lib.sliced_layout_slices
    ns, nd = 50_000, 100_000
    knobs(sliced_owned=0)
    assert f(ns, nd, 128) == 8            # the form is off: the pair's layout
    knobs(sliced_owned=1)
    assert f(ns, nd, 128) == 16 and f(nd, ns, 128) == 8  # forcing the FORM does not change which layout a class gets
    knobs(sliced_chunk_rows=37)
    assert f(ns, nd, 128) == 8            # forced chunking: the pair's product
    knobs(sliced_owned_lds_rows=98)
    assert f(ns, nd, 128) == 8            # two row rounds: not the class
    knobs(sliced_owned_slices=8)
    assert f(ns, nd, 128) == 8
    knobs(sliced_owned_slices=16)
    assert f(ns, nd, 128) == 16 and f(nd, ns, 128) == 16 and f(nd, nd, 128, True) == 16 and f(300, 330, 128) == 16 and f(300, 330, 4) == 16
    knobs(sliced_owned_slices=16, sliced_owned=0)
    assert f(300, 330, 128) == 8
    knobs(sliced_owned_slices=16, sliced_chunk_rows=100)
    assert f(300, 330, 128) == 8
    knobs(sliced_owned_slices=64)
    assert f(300, 330, 128) == 64 and f(300, 330, 344) == 8   # 344 columns: 3 column rounds x 64 slices > 128 phases
    knobs(sliced_owned_slices=3)
    assert f(300, 330, 344) == 3
    knobs(sliced_owned_slices=1000)
    assert f(300, 330, 128) == 64         # clamped to what the layout builders make
    knobs(sliced_owned_slices=16, sliced_owned_lds_rows=10, sliced_owned_grid=256)
    assert f(5_000, 330, 344, True) == 16  # 20 rows per workgroup in 2 rounds x 3 column rounds x 16 slices = 96 phases
    knobs(sliced_owned_slices=16, sliced_owned_lds_rows=5, sliced_owned_grid=256)
    assert f(5_000, 330, 344, True) == 8   # 4 rounds: 192 phases
    knobs(sliced_owned_slices=16, sliced_owned_lds_rows=10, sliced_owned_grid=19)
    assert f(5_000, 330, 128) == 8        # 264 rows per workgroup in 27 rounds: beyond 128 phases


def test_layout_header_declares_exactly_the_new_entry_point():
    """include/dgmi_layout.h is a header of its own (tests/test_abi.py pins dgmi.h's list): it declares the one entry
    point, the library exports it and the ctypes table mirrors it."""
    import re

    from dream_gnn_amd import _lib

    text = open(os.path.join(ROOT, "include", "dgmi_layout.h")).read()
    assert re.findall(r"DGMI_API\s+[\w\s\*]+?\b(dgmi_\w+)\s*\(", text) == ["dgmi_sliced_layout_slices"]
    assert sorted(_lib.LAYOUT_SIGNATURES) == ["dgmi_sliced_layout_slices"] and hasattr(_lib.lib, "dgmi_sliced_layout_slices")
    assert not set(_lib.LAYOUT_SIGNATURES) & set(_lib.SIGNATURES)
    assert _lib.lib.dgmi_set_tuning(b"sliced_owned_slices", 0) == 0
