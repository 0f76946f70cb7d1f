"""The rows -> (worker block, lane group) mapping of the XCD-local SpMM (``sliced_runs`` / ``sliced_run``,
csrc/dgmi_sliced_common.h), on the host (no GPU): a stand-alone C++ program includes the header the kernels include and
walks every worker block and lane group of a launch.  The groups' row ranges must tile ``[row_begin, row_end)`` exactly
once, in order, whatever the rows per group, the taper and the width; the block count must be the one
``sliced_geometry`` puts in the grid; a block's first group is never idle (the touchers read a block's first row from
it); runs never grow towards the end of the chunk and the taper's last section runs ``ceil(R / 4)`` rows."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

PROGRAM = r"""
#include <cstdio>
#include "dgmi_sliced_common.h"

namespace dgmi {
static Tuning g_tuning;
Tuning& tuning() { return g_tuning; }
}  // namespace dgmi

using namespace dgmi;

static int check(int64_t n_rows, int R, int64_t taper, int lpr, int64_t row_begin) {
  Tuning& t = tuning();
  t.sliced_rows = R;
  t.sliced_taper_rows = taper;
  const int n_slices = 8;
  const SlicedGeometry g = sliced_geometry(row_begin, row_begin + n_rows, 128, 1000, 128, n_slices, lpr, 4);
  const int G = 64 / lpr, groups = 4 * G;
  const int r_eff = R < lpr ? R : lpr - 1;
#define FAIL(msg)                                                                                                   \
  do {                                                                                                              \
    printf("n_rows %lld R %d taper %lld lpr %d: %s\n", (long long)n_rows, R, (long long)taper, lpr, msg);           \
    return 1;                                                                                                       \
  } while (0)
  if (g.R != r_eff || g.runs.groups != groups) FAIL("rows per group / groups per block");
  if (g.workers != g.runs.blocks[2]) FAIL("sliced_geometry's worker blocks are not the mapping's");
  if ((int64_t)g.grid.x != (g.workers + g.touchers) * n_slices) FAIL("grid.x");
  if (g.touchers != (g.workers + g.touch_group - 1) / g.touch_group) FAIL("touchers");
  int64_t cursor = 0;
  int prev_run = g.R, last_run = 0;
  for (int64_t b = 0; b < g.workers; ++b) {
    int block_run = 0;
    bool idle_seen = false;
    for (int slot = 0; slot < groups; ++slot) {
      const SlicedRun r = sliced_run(g.runs, b, slot);
      if (r.rows == 0) {
        if (slot == 0) FAIL("the first group of a block is idle");
        if (r.first != n_rows) FAIL("an idle group does not point past the chunk");
        idle_seen = true;
        continue;
      }
      if (idle_seen) FAIL("a working group after an idle one");
      if (r.first != cursor) FAIL(r.first < cursor ? "overlap" : "gap");
      if (r.rows < 1 || r.rows > g.R || r.rows >= lpr) FAIL("rows of a group");
      if (r.rows > block_run) block_run = r.rows;
      cursor += r.rows;
    }
    if (block_run > prev_run) FAIL("runs grow towards the end");
    if (!idle_seen) prev_run = block_run;  // (a ragged block ends a section and may be shorter than the next one's runs)
    last_run = block_run;
  }
  if (cursor != n_rows) FAIL("rows left over");
  for (int64_t b = g.workers; b < g.workers + 3; ++b)
    if (sliced_run(g.runs, b, 0).rows != 0 || sliced_run(g.runs, b, 0).first != n_rows) FAIL("a block past the last one");
  const int64_t per_block = (int64_t)groups * g.R;
  if (taper < 0 && g.workers != (n_rows + per_block - 1) / per_block) FAIL("block count without a taper");
  if (taper > 0 && (taper < n_rows ? taper : n_rows) / 2 >= 1 && last_run > (g.R + 3) / 4) FAIL("the last block is not a short one");
  return 0;
#undef FAIL
}

int main() {
  const int64_t rows[] = {1, 7, 63, 64, 65, 307, 3000, 33001};
  const int Rs[] = {1, 3, 8, 15};
  const int widths[] = {8, 16, 32, 64};
  int cases = 0;
  for (int64_t n : rows)
    for (int R : Rs)
      for (int lpr : widths) {
        const int64_t tapers[] = {-1, 0, 5, n, 64, n / 3};
        for (int64_t taper : tapers)
          for (int64_t row_begin : {(int64_t)0, (int64_t)37}) {
            if (check(n, R, taper, lpr, row_begin)) return 1;
            ++cases;
          }
      }
  printf("ok %d\n", cases);
  return 0;
}
"""


def test_lane_group_rows_tile_the_chunk_and_match_the_grid(tmp_path):
    src, exe = tmp_path / "taper_host.cpp", tmp_path / "taper_host"
    src.write_text(PROGRAM)
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    cmd = [hipcc, "-x", "hip", "--cuda-host-only", "-O1", "-std=c++17", "-I" + os.path.join(ROOT, "include"),
           "-I" + os.path.join(ROOT, "dream_gnn_amd", "csrc"), str(src), "-o", str(exe)]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-4000:]
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert r.stdout.strip() == "ok %d" % (8 * 4 * 4 * 6 * 2), r.stdout
