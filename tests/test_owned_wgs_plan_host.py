"""The plan of the workgroup-owned XCD-local SpMM with one and with two workgroups per CU (``owned_plan(..., wgs_per_cu)``,
csrc/dgmi_owned_common.h) on the host (no GPU): a stand-alone C++ program includes the header the kernel and its launcher
include and walks every workgroup, phase, task slot and lane group.  Every (row, slice, column tile) must be covered exactly
once; LDS stays within ``160 KiB / wgs_per_cu`` and the row budget within ``kOwnedLdsRowBytes / wgs_per_cu``; the plan at
``wgs_per_cu = 1`` equals the 6-argument plan field by field.  The walker is built and run twice: plainly, and with the
address and undefined-behaviour sanitizers."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

PROGRAM = r"""
#include <cstdio>
#include <vector>
#include "dgmi_owned_common.h"

using namespace dgmi;

static bool same(const OwnedPlan& a, const OwnedPlan& b) {
  return a.ok == b.ok && a.lpr == b.lpr && a.G == b.G && a.R == b.R && a.col_rounds == b.col_rounds &&
         a.row_rounds == b.row_rounds && a.phases == b.phases && a.wg_rows == b.wg_rows && a.active == b.active &&
         a.round_rows == b.round_rows && a.tasks == b.tasks && a.n_dst == b.n_dst && a.lds_bytes == b.lds_bytes;
}

static int check(int wgs, int64_t n_dst, int64_t grid, int64_t F, int lpr, int R, int want_rounds) {
#define FAIL(msg)                                                                                                       \
  do {                                                                                                                  \
    printf("wgs %d n_dst %lld grid %lld F %lld lpr %d R %d rounds %d: %s\n", wgs, (long long)n_dst, (long long)grid,    \
           (long long)F, lpr, R, want_rounds, msg);                                                                     \
    return 1;                                                                                                           \
  } while (0)
  const int64_t B = (n_dst + grid - 1) / grid;
  // the cap that gives `want_rounds` row rounds; skipped where no cap gives exactly that many
  if (B < want_rounds) return 0;
  const int64_t cap = want_rounds == 1 ? 0 : (B + want_rounds - 1) / want_rounds;
  if (cap > 0 && (B + cap - 1) / cap != want_rounds) return 0;
  const OwnedPlan p = owned_plan(n_dst, F, lpr, grid, R, cap, wgs);
  if (wgs == 1 && !same(p, owned_plan(n_dst, F, lpr, grid, R, cap))) FAIL("wgs_per_cu = 1 is not the 6-argument plan");
  const int col_tiles = (int)((F + 4 * lpr - 1) / (4 * lpr));
  const int64_t budget_rows = kOwnedLdsRowBytes / wgs / (16 * lpr);
  if (!p.ok) {
    const int64_t fit = cap > 0 && cap < budget_rows ? cap : budget_rows;
    if (((B + fit - 1) / fit) * col_tiles * kOwnedSlices <= kOwnedMaxPhases) FAIL("a plan that fits was refused");
    return 0;
  }
  if (p.G != 64 / lpr || p.lpr != lpr || p.wg_rows != B || p.col_rounds != col_tiles || p.n_dst != n_dst) FAIL("geometry");
  if (p.R < 1 || p.R >= lpr || p.R > (R >= 1 ? R : kOwnedMaxRows) || (R >= 1 && R < lpr && p.R != R)) FAIL("rows per lane group");
  if (B <= budget_rows && p.row_rounds != want_rounds) FAIL("row rounds");
  if (p.round_rows < 1 || p.round_rows > budget_rows || (cap > 0 && p.round_rows > cap)) FAIL("LDS rows exceed the cap");
  if ((int64_t)p.round_rows * p.row_rounds < B) FAIL("the rounds do not hold a workgroup's rows");
  if (p.phases != p.col_rounds * p.row_rounds * kOwnedSlices || p.phases > kOwnedMaxPhases) FAIL("phases");
  if (p.tasks != (p.round_rows + p.G * p.R - 1) / (p.G * p.R)) FAIL("task slots");
  if (p.lds_bytes != (size_t)p.round_rows * 16 * lpr + 4 * ((size_t)p.tasks + p.phases + 2)) FAIL("LDS bytes");
  if (p.lds_bytes > (size_t)(160 << 10) / wgs) FAIL("LDS bytes exceed a workgroup's share of the CU's");
  if (R <= 0 && p.R > 1 && p.R < kOwnedMaxRows && p.R < lpr - 1 && p.tasks < owned_form_waves(wgs) - 1)
    FAIL("built-in R leaves a worker without a task");
  if (p.active < 1 || p.active > grid || (p.active - 1) * B >= n_dst || p.active * B < n_dst) FAIL("active workgroups");
  std::vector<int> covered((size_t)n_dst * kOwnedSlices * col_tiles, 0);
  for (int64_t wg = 0; wg < grid + 2; ++wg) {
    const int T = owned_wg_tasks(p, wg);
    if ((T == 0) != (wg >= p.active)) FAIL("workgroups without rows must have no tasks, the others some");
    if (T > p.tasks) FAIL("more task slots than the launcher sized LDS for");
    if (T == 0) continue;
    for (int P = 0; P < p.phases; ++P) {
      const OwnedPhase ph = owned_phase(p, P);
      if (ph.slice != P % kOwnedSlices || ph.col_round < 0 || ph.col_round >= col_tiles || ph.row_round < 0 ||
          ph.row_round >= p.row_rounds)
        FAIL("phase decoding");
      for (int t = 0; t < T; ++t)
        for (int g = 0; g < p.G; ++g) {
          const OwnedTask k = owned_task(p, wg, ph.row_round, t, g);
          if (k.rows < 0 || k.rows > p.R) FAIL("rows of a lane group");
          if (k.lds_row != (t * p.G + g) * p.R) FAIL("LDS row of a task");
          if (k.rows == 0) continue;
          if (k.lds_row + k.rows > p.round_rows) FAIL("LDS row outside the round");
          if (k.row0 < wg * B || k.row0 + k.rows > (wg + 1) * B || k.row0 + k.rows > n_dst) FAIL("rows outside the workgroup's block");
          for (int r = 0; r < k.rows; ++r) ++covered[((size_t)(k.row0 + r) * kOwnedSlices + ph.slice) * col_tiles + ph.col_round];
        }
    }
  }
  for (int c : covered)
    if (c != 1) FAIL(c == 0 ? "a (row, slice, column tile) is not covered" : "a (row, slice, column tile) is covered twice");
  return 0;
#undef FAIL
}

int main() {
  static_assert(owned_form_waves(1) == kOwnedWaves && owned_form_waves(1) - 1 == kOwnedWorkers, "the one-workgroup form");
  static_assert(owned_form_waves(2) == kOwnedPairWaves && 2 * kOwnedPairWaves <= 32, "two workgroups within a CU's 32 waves");
  const int64_t rows[] = {1, 7, 306, 307, 4099};
  const int64_t grids[] = {1, 2, 3, 8, 19, 512};
  const int widths[] = {8, 16, 32, 64};
  const int64_t Fs[] = {4, 128, 344};
  const int Rs[] = {0, 1, 2, 5};
  const int rounds[] = {1, 2, 4};
  int cases = 0;
  for (int wgs = 1; wgs <= 2; ++wgs)
    for (int64_t n : rows)
      for (int64_t grid : grids)
        for (int lpr : widths)
          for (int64_t F : Fs)
            for (int R : Rs)
              for (int q : rounds) {
                if (check(wgs, n, grid, F, lpr, R, q)) return 1;
                ++cases;
              }
  // a workgroup count or form the plan does not know, and the real budgets: half the rows fit with two workgroups
  if (owned_plan(307, 128, 32, 8, 0, 0, 0).ok || owned_plan(307, 128, 32, 8, 0, 0, 3).ok) {
    printf("wgs_per_cu other than 1 and 2 must be refused\n");
    return 1;
  }
  for (int lpr : widths) {
    const OwnedPlan one = owned_plan(100000, 4 * lpr, lpr, 1, 0, 0, 1), two = owned_plan(100000, 4 * lpr, lpr, 1, 0, 0, 2);
    if (one.ok || two.ok) {  // 100 000 rows of one workgroup: too many phases either way
      printf("lpr %d: a plan of more than kOwnedMaxPhases phases was accepted\n", lpr);
      return 1;
    }
    const int64_t n = kOwnedLdsRowBytes / (16 * lpr);  // exactly the one-workgroup row budget
    const OwnedPlan a = owned_plan(n, 4 * lpr, lpr, 1, 0, 0, 1), b = owned_plan(n, 4 * lpr, lpr, 1, 0, 0, 2);
    if (!a.ok || !b.ok || a.row_rounds != 1 || b.row_rounds != 2 || b.round_rows * 2 != a.round_rows ||
        b.lds_bytes > (size_t)(80 << 10)) {
      printf("lpr %d: the row budget is not halved\n", lpr);
      return 1;
    }
  }
  printf("ok %d\n", cases);
  return 0;
}
"""

CASES = 2 * 5 * 6 * 4 * 3 * 4 * 3


@pytest.mark.parametrize("sanitize", [False, True], ids=["plain", "asan_ubsan"])
def test_owned_plan_with_one_and_two_workgroups_per_cu(tmp_path, sanitize):
    src, exe = tmp_path / "owned_wgs_plan_host.cpp", tmp_path / "owned_wgs_plan_host"
    src.write_text(PROGRAM)
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    flags = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"] if sanitize else ["-O2"]
    cmd = [hipcc, "-x", "hip", "--cuda-host-only", "-std=c++17", "-I" + os.path.join(ROOT, "include"),
           "-I" + os.path.join(ROOT, "dream_gnn_amd", "csrc")] + flags + [str(src), "-o", str(exe)]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-4000:]
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert r.stdout.strip() == "ok %d" % CASES, r.stdout
