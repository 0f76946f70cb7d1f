"""The plan of the workgroup-owned SpMM with EIGHT columns per lane (``owned_plan(..., cols_per_lane = 8)``,
csrc/dgmi_owned_common.h: the bf16 gather of csrc/dgmi_owned.hip) on the host (no GPU): a stand-alone C++ program
includes the header the kernel and its launcher include and walks every workgroup, phase, task slot and lane group.
Every (row, slice, 8 lpr-column tile) must be covered exactly once; a task slot covers the same rows in every phase of a
round; ``lds_bytes`` is ``round_rows * 32 lpr`` plus the control words and stays inside the CU's 160 KiB; at most 128
phases; what ``owned_decode`` hands a lane group is what ``owned_phase`` / ``owned_task`` say; and a plan made with the
defaulted argument is field for field the plan of ``cols_per_lane = 4`` passed explicitly."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

PROGRAM = r"""
#include <cstdio>
#include <vector>
#include "dgmi_owned_common.h"

using namespace dgmi;

static bool same(const OwnedPlan& a, const OwnedPlan& b) {
  return a.ok == b.ok && a.lpr == b.lpr && a.G == b.G && a.R == b.R && a.col_rounds == b.col_rounds &&
         a.row_rounds == b.row_rounds && a.phases == b.phases && a.slices == b.slices && a.wg_rows == b.wg_rows &&
         a.active == b.active && a.round_rows == b.round_rows && a.tasks == b.tasks && a.n_dst == b.n_dst &&
         a.lds_bytes == b.lds_bytes;
}

static int check(int64_t n_dst, int64_t grid, int64_t F, int lpr, int R, int want_rounds, int slices) {
#define FAIL(msg)                                                                                                      \
  do {                                                                                                                 \
    printf("n_dst %lld grid %lld F %lld lpr %d R %d rounds %d slices %d: %s\n", (long long)n_dst, (long long)grid,     \
           (long long)F, lpr, R, want_rounds, slices, msg);                                                            \
    return 1;                                                                                                          \
  } while (0)
  const int64_t B = (n_dst + grid - 1) / grid;
  // the cap that gives `want_rounds` row rounds; skipped where no cap gives exactly that many
  if (B < want_rounds) return 0;
  const int64_t cap = want_rounds == 1 ? 0 : (B + want_rounds - 1) / want_rounds;
  if (cap > 0 && (B + cap - 1) / cap != want_rounds) return 0;

  // the defaulted argument: the plan of four columns per lane, field for field — with and without the slice count
  if (!same(owned_plan(n_dst, F, lpr, grid, R, cap, 1, kOwnedPhaseTasks, slices),
            owned_plan(n_dst, F, lpr, grid, R, cap, 1, kOwnedPhaseTasks, slices, 4)))
    FAIL("the defaulted cols_per_lane is not 4");
  if (!same(owned_plan(n_dst, F, lpr, grid, R, cap), owned_plan(n_dst, F, lpr, grid, R, cap, 1, kOwnedPhaseTasks, kOwnedSlices, 4)))
    FAIL("the plan made without slices and cols_per_lane is not (8 slices, 4 columns)");
  {
    const OwnedPlan p4 = owned_plan(n_dst, F, lpr, grid, R, cap, 1, kOwnedPhaseTasks, slices, 4);
    if (p4.ok && (p4.col_rounds != (int)((F + 4 * lpr - 1) / (4 * lpr)) ||
                  p4.lds_bytes != (size_t)p4.round_rows * 16 * lpr + 4 * ((size_t)p4.tasks + p4.phases + 2)))
      FAIL("four columns per lane: 4 lpr-column rounds and 16 lpr bytes per row");
  }

  const OwnedPlan p = owned_plan(n_dst, F, lpr, grid, R, cap, 1, kOwnedPhaseTasks, slices, 8);
  const int col_tiles = (int)((F + 8 * lpr - 1) / (8 * lpr));
  const int64_t budget_rows = kOwnedLdsRowBytes / (32 * lpr);
  if (!p.ok) {
    const int64_t fit = cap > 0 && cap < budget_rows ? cap : budget_rows;
    if (((B + fit - 1) / fit) * col_tiles * slices <= kOwnedMaxPhases) FAIL("a plan that fits was refused");
    return 0;
  }
  if (p.G != 64 / lpr || p.lpr != lpr || p.wg_rows != B || p.col_rounds != col_tiles || p.slices != slices) FAIL("geometry");
  if (p.R < 1 || p.R >= lpr || (R >= 1 && R < lpr && p.R != R)) FAIL("rows per lane group");
  if (cap <= budget_rows && p.row_rounds != want_rounds && (cap > 0 || B <= budget_rows)) FAIL("row rounds");
  if (p.round_rows < 1 || p.round_rows > budget_rows || (cap > 0 && p.round_rows > cap)) FAIL("LDS rows exceed the cap");
  if ((int64_t)p.round_rows * p.row_rounds < B) FAIL("the rounds do not hold a workgroup's rows");
  if (p.phases != p.col_rounds * p.row_rounds * slices || p.phases > kOwnedMaxPhases || p.phases > 128) FAIL("phases");
  if (p.tasks != (p.round_rows + p.G * p.R - 1) / (p.G * p.R)) FAIL("task slots");
  if (p.lds_bytes != (size_t)p.round_rows * 32 * lpr + 4 * ((size_t)p.tasks + p.phases + 2)) FAIL("LDS bytes");
  if (p.lds_bytes > (size_t)(160 << 10)) FAIL("LDS bytes exceed the CU's");
  if (p.active < 1 || p.active > grid || (p.active - 1) * B >= n_dst || p.active * B < n_dst) FAIL("active workgroups");
  std::vector<int> covered((size_t)n_dst * slices * col_tiles, 0);
  for (int64_t wg = 0; wg < grid + 2; ++wg) {
    const int T = owned_wg_tasks(p, wg);
    if ((T == 0) != (wg >= p.active)) FAIL("workgroups without rows must have no tasks, the others some");
    if (T > p.tasks) FAIL("more task slots than the launcher sized LDS for");
    if (T == 0) continue;
    int64_t wg_rows = 0;
    for (int P = 0; P < p.phases; ++P) {
      const OwnedPhase ph = owned_phase(p, P);
      if (ph.slice != P % slices || ph.col_round < 0 || ph.col_round >= col_tiles || ph.row_round < 0 || ph.row_round >= p.row_rounds)
        FAIL("phase decoding");
      if (P > 0 && ph.slice != 0) {  // inside a round: same column tile, same row round as the phase before
        const OwnedPhase prev = owned_phase(p, P - 1);
        if (prev.col_round != ph.col_round || prev.row_round != ph.row_round || prev.slice != ph.slice - 1)
          FAIL("the slices of a round are not consecutive phases in order");
      }
      int64_t cursor = -1;
      for (int t = 0; t < T; ++t)
        for (int g = 0; g < p.G; ++g) {
          const OwnedTask k = owned_task(p, wg, ph.row_round, t, g);
          const OwnedWork w = owned_decode(p, wg, T, P * T + t, g);  // what the kernel's lane group works from
          if (w.phase != P || w.task != t || w.slice != ph.slice || w.col_round != ph.col_round || w.lds_row != k.lds_row ||
              w.rows != k.rows || w.row_base + w.lds_row != k.row0)
            FAIL("owned_decode");
          if (k.rows < 0 || k.rows > p.R) FAIL("rows of a lane group");
          if (k.lds_row != (t * p.G + g) * p.R) FAIL("LDS row of a task");
          if (k.rows > 0 && k.lds_row + k.rows > p.round_rows) FAIL("LDS row outside the round");
          if (ph.slice > 0) {  // the same rows and LDS rows as in the phase before
            const OwnedTask before = owned_task(p, wg, owned_phase(p, P - 1).row_round, t, g);
            if (before.row0 != k.row0 || before.rows != k.rows || before.lds_row != k.lds_row) FAIL("a task's rows change inside a round");
          }
          if (k.rows == 0) continue;
          if (k.row0 < wg * B || k.row0 + k.rows > (wg + 1) * B || k.row0 + k.rows > n_dst) FAIL("rows outside the workgroup's block");
          if (cursor >= 0 && k.row0 != cursor) FAIL("the rows of a phase are not consecutive");
          cursor = k.row0 + k.rows;
          for (int r = 0; r < k.rows; ++r) {
            ++covered[((size_t)(k.row0 + r) * slices + ph.slice) * col_tiles + ph.col_round];
            if (ph.slice == 0 && ph.col_round == 0) ++wg_rows;
          }
        }
    }
    if (wg_rows != owned_wg_rows(p, wg)) FAIL("a workgroup's rows");
    const OwnedWork past = owned_decode(p, wg, T, p.phases * T, 0);
    if (past.phase != p.phases || past.rows != 0) FAIL("a task past the last one has rows");
    for (int q = 0; q < p.row_rounds; ++q)  // slots past T are empty in every round
      for (int g = 0; g < p.G; ++g)
        if (owned_task(p, wg, q, T, g).rows != 0) FAIL("a task slot past the workgroup's last one has rows");
  }
  for (int c : covered)
    if (c != 1) FAIL(c == 0 ? "a (row, slice, column tile) is not covered" : "a (row, slice, column tile) is covered twice");
  return 0;
#undef FAIL
}

int main() {
  const int64_t rows[] = {1, 7, 307, 50000};
  const int64_t grids[] = {1, 3, 8, 19, 256};
  const int widths[] = {8, 16, 32};
  const int64_t Fs[] = {8, 128, 344};
  const int Rs[] = {0, 1, 5};
  const int rounds[] = {1, 2, 4};
  const int slice_counts[] = {3, 8, 16, 64};
  int cases = 0;
  for (int64_t n : rows)
    for (int64_t grid : grids)
      for (int lpr : widths)
        for (int64_t F : Fs)
          for (int R : Rs)
            for (int q : rounds)
              for (int S : slice_counts) {
                // the large product (rounds forced by the LDS budget, the built-in R): 8 / 16 slices at F = 128 / 344
                if (n > 1000 && (F == 8 || R != 0 || (S != 8 && S != 16))) continue;
                if (check(n, grid, F, lpr, R, q, S)) return 1;
                ++cases;
              }
  // a plan of other column counts is refused, as is one beyond 128 phases: 64 slices x 3 column rounds
  if (owned_plan(307, 128, 16, 8, 0, 0, 1, kOwnedPhaseTasks, 8, 2).ok || owned_plan(307, 128, 16, 8, 0, 0, 1, kOwnedPhaseTasks, 8, 16).ok) {
    printf("a plan of 2 or 16 columns per lane was made\n");
    return 1;
  }
  if (owned_plan(307, 344, 16, 8, 0, 0, 1, kOwnedPhaseTasks, 64, 8).ok || !owned_plan(307, 344, 32, 8, 0, 0, 1, kOwnedPhaseTasks, 64, 8).ok) {
    printf("the 128-phase bound: 64 slices x 3 column rounds must be refused, 64 x 2 taken\n");
    return 1;
  }
  printf("ok %d\n", cases);
  return 0;
}
"""


def test_owned_plan_with_eight_columns_per_lane(tmp_path):
    src, exe = tmp_path / "owned_bf16_plan_host.cpp", tmp_path / "owned_bf16_plan_host"
    src.write_text(PROGRAM)
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    cmd = [hipcc, "-x", "hip", "--cuda-host-only", "-O2", "-std=c++17", "-I" + os.path.join(ROOT, "include"),
           "-I" + os.path.join(ROOT, "dream_gnn_amd", "csrc"), str(src), "-o", str(exe)]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-4000:]
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert r.stdout.strip() == "ok %d" % (3 * 5 * 3 * 3 * 3 * 3 * 4 + 1 * 5 * 3 * 2 * 1 * 3 * 2), r.stdout
