"""The plan of the workgroup-owned XCD-local SpMM (``owned_plan`` / ``owned_phase`` / ``owned_task``,
csrc/dgmi_owned_common.h) on the host (no GPU): a stand-alone C++ program includes the header the kernel and its launcher
include and walks every workgroup, phase, task slot and lane group.  Every (row, slice, column tile) must be covered
exactly once; a task slot's rows and LDS rows are the same in every phase of a round; LDS rows stay inside the cap and
the LDS budget; the task slots per phase are the ones the launcher sizes LDS for; workgroups without rows have no tasks."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

PROGRAM = r"""
#include <cstdio>
#include <vector>
#include "dgmi_owned_common.h"

using namespace dgmi;

static int check(int64_t n_dst, int64_t grid, int64_t F, int lpr, int R, int want_rounds) {
#define FAIL(msg)                                                                                                      \
  do {                                                                                                                 \
    printf("n_dst %lld grid %lld F %lld lpr %d R %d rounds %d: %s\n", (long long)n_dst, (long long)grid, (long long)F, \
           lpr, R, want_rounds, msg);                                                                                  \
    return 1;                                                                                                          \
  } while (0)
  const int64_t B = (n_dst + grid - 1) / grid;
  // the cap that gives `want_rounds` row rounds (0: no cap); skipped where B has fewer rows than rounds
  int64_t cap = 0;
  if (want_rounds > 0) {
    if (B < want_rounds) return 0;
    cap = (B + want_rounds - 1) / want_rounds;
    if ((B + cap - 1) / cap != want_rounds) return 0;  // no cap gives exactly that many rounds
  }
  const OwnedPlan p = owned_plan(n_dst, F, lpr, grid, R, cap);
  const int col_tiles = (int)((F + 4 * lpr - 1) / (4 * lpr));
  const int64_t budget_rows = kOwnedLdsRowBytes / (16 * lpr);
  if (!p.ok) {
    const int64_t fit = cap > 0 && cap < budget_rows ? cap : budget_rows;
    if (((B + fit - 1) / fit) * col_tiles * kOwnedSlices <= kOwnedMaxPhases) FAIL("a plan that fits was refused");
    return 0;
  }
  if (p.G != 64 / lpr || p.lpr != lpr || p.wg_rows != B || p.col_rounds != col_tiles) FAIL("geometry");
  if (p.R < 1 || p.R >= lpr || (R >= 1 && R < lpr && p.R != R)) FAIL("rows per lane group");
  if (want_rounds > 0 && cap <= budget_rows && p.row_rounds != want_rounds) FAIL("row rounds");
  if (p.round_rows < 1 || p.round_rows > budget_rows || (cap > 0 && p.round_rows > cap)) FAIL("LDS rows exceed the cap");
  if ((int64_t)p.round_rows * p.row_rounds < B) FAIL("the rounds do not hold a workgroup's rows");
  if (p.phases != p.col_rounds * p.row_rounds * kOwnedSlices || p.phases > kOwnedMaxPhases) FAIL("phases");
  if (p.tasks != (p.round_rows + p.G * p.R - 1) / (p.G * p.R)) FAIL("task slots");
  if (p.lds_bytes != (size_t)p.round_rows * 16 * lpr + 4 * ((size_t)p.tasks + p.phases + 2)) FAIL("LDS bytes");
  if (p.lds_bytes > (size_t)(160 << 10)) FAIL("LDS bytes exceed the CU's");
  if (R <= 0 && p.R > 1 && p.R < kOwnedMaxRows && p.R < lpr - 1 && p.tasks < kOwnedWorkers) FAIL("built-in R leaves a worker without a task");
  if (p.active < 1 || p.active > grid || (p.active - 1) * B >= n_dst || p.active * B < n_dst) FAIL("active workgroups");
  std::vector<int> covered((size_t)n_dst * kOwnedSlices * col_tiles, 0);
  for (int64_t wg = 0; wg < grid + 2; ++wg) {
    const int T = owned_wg_tasks(p, wg);
    if ((T == 0) != (wg >= p.active)) FAIL("workgroups without rows must have no tasks, the others some");
    if (T > p.tasks) FAIL("more task slots than the launcher sized LDS for");
    if (T == 0) continue;
    int64_t wg_rows = 0;
    for (int P = 0; P < p.phases; ++P) {
      const OwnedPhase ph = owned_phase(p, P);
      if (ph.slice != P % kOwnedSlices || ph.col_round < 0 || ph.col_round >= col_tiles || ph.row_round < 0 ||
          ph.row_round >= p.row_rounds)
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
            ++covered[((size_t)(k.row0 + r) * kOwnedSlices + ph.slice) * col_tiles + ph.col_round];
            if (ph.slice == 0 && ph.col_round == 0) ++wg_rows;
          }
        }
    }
    if (wg_rows != owned_wg_rows(p, wg)) FAIL("a workgroup's rows");
    // slots past T are empty in every round
    for (int q = 0; q < p.row_rounds; ++q)
      for (int g = 0; g < p.G; ++g)
        if (owned_task(p, wg, q, T, g).rows != 0) FAIL("a task slot past the workgroup's last one has rows");
  }
  for (int c : covered)
    if (c != 1) FAIL(c == 0 ? "a (row, slice, column tile) is not covered" : "a (row, slice, column tile) is covered twice");
  return 0;
#undef FAIL
}

int main() {
  const int64_t rows[] = {1, 7, 307, 50000, 100000};
  const int64_t grids[] = {1, 3, 8, 19, 256};
  const int widths[] = {8, 16, 32, 64};
  const int64_t Fs[] = {4, 128, 344};
  const int Rs[] = {0, 1, 2, 5, 7, 63};
  int cases = 0;
  for (int64_t n : rows)
    for (int64_t grid : grids)
      for (int lpr : widths)
        for (int64_t F : Fs)
          for (int R : Rs)
            for (int rounds = 0; rounds <= 4; ++rounds) {
              // the two large products: every width, grid and round count at R = built-in / 1 / 5 and F = 128 / 344
              if (n > 1000 && (F == 4 || R == 2 || R == 7 || R == 63)) continue;
              if (check(n, grid, F, lpr, R, rounds)) return 1;
              ++cases;
            }
  printf("ok %d\n", cases);
  return 0;
}
"""


def test_owned_plan_covers_every_segment_once_inside_the_lds_cap(tmp_path):
    src, exe = tmp_path / "owned_plan_host.cpp", tmp_path / "owned_plan_host"
    src.write_text(PROGRAM)
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    cmd = [hipcc, "-x", "hip", "--cuda-host-only", "-O2", "-std=c++17", "-I" + os.path.join(ROOT, "include"),
           "-I" + os.path.join(ROOT, "dream_gnn_amd", "csrc"), str(src), "-o", str(exe)]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-4000:]
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert r.stdout.strip() == "ok %d" % (3 * 5 * 4 * 3 * 6 * 5 + 2 * 5 * 4 * 2 * 3 * 5), r.stdout
