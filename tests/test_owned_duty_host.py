"""The touching duty of the workgroup-owned SpMM's form without a toucher, on the host (no GPU).

A stand-alone C++ program includes csrc/dgmi_owned_common.h — the header the kernel takes the duty's index arithmetic
from (``owned_duty_chunk``, ``owned_duty_span``, ``owned_touch_rows``, ``owned_touch_boundary``, ``owned_touch_id``) — and, for
plans of every lane-group width, 8 and 16 slices, one and two row and column rounds, short last workgroups and
workgroups without rows, over a random slice-major layout with runs of empty rows, walks every workgroup the way the
kernel does: the wave that reserves task slot k = 0, 1, ... asks ``owned_duty_chunk`` whether the slot carries a duty
and touches the chunks of ``owned_duty_span``.

Checked, for duty chunks of 1, 4, 8, 16 slots and a whole phase and leads of 0, 8, 16 and a phase:
 - every chunk of the launch is touched by exactly one duty, none past the last, and a slot past the last task (the
   reservations the waves make at the end) carries none;
 - a duty touches only chunks at or ahead of its own;
 - every touched boundary word lies inside the slice-major ``segptr`` (``slices * n_dst + 1`` words) and every touched id
   word inside ``indices`` (``nnz`` words);
 - every 128-byte line that lies wholly inside a chunk's boundaries or ids is touched, and both ends of the boundaries;
 - at the toucher's own chunking (``kOwnedTouchChunk``) the words touched are, chunk for chunk, exactly those of the
   toucher wave of the 15-worker form, whose lane formula is restated here.

Built and run twice: plainly, and with the address and undefined-behaviour sanitizers.  The last test pins the
tasks-per-phase target ``owned_plan`` gives sixteen workers."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

PROGRAM = r"""
#include <cstdio>
#include <cstdint>
#include <set>
#include <vector>
#include "dgmi_owned_common.h"

using namespace dgmi;

static uint64_t rng_state = 88172645463325252ull;
static uint32_t rnd() {
  rng_state ^= rng_state << 13;
  rng_state ^= rng_state >> 7;
  rng_state ^= rng_state << 17;
  return (uint32_t)(rng_state >> 20);
}

#define FAIL(...)                 \
  do {                            \
    printf(__VA_ARGS__);          \
    printf("\n");                 \
    return 1;                     \
  } while (0)

typedef std::set<int64_t> Words;

// the words the toucher wave of the 15-worker form reads for chunk `touched` (its lane formula, dgmi_owned_kernel.h)
static void toucher_words(const OwnedPlan& pl, int64_t wg, int T, int touched, const std::vector<int32_t>& segptr, Words& seg,
                          Words& ids) {
  const int chunks_per_phase = (T + kOwnedTouchChunk - 1) / kOwnedTouchChunk;
  const int P = touched / chunks_per_phase, t0 = (touched - P * chunks_per_phase) * kOwnedTouchChunk;
  const OwnedPhase ph = owned_phase(pl, P);
  const int64_t in_round = owned_round_rows(pl, wg, ph.row_round);
  const int64_t lds_first = (int64_t)t0 * pl.G * pl.R;
  int64_t lds_last = lds_first + (int64_t)kOwnedTouchChunk * pl.G * pl.R;
  if (lds_last > in_round) lds_last = in_round;
  if (lds_first >= lds_last) return;
  const int64_t base = (int64_t)ph.slice * pl.n_dst;
  const int64_t r_first = owned_task(pl, wg, ph.row_round, t0, 0).row0, r_last = r_first + (lds_last - lds_first);
  for (int lane = 0; lane < 64; ++lane) {
    const int64_t rp = lane == 0 ? r_first : (lane == 1 ? r_last : r_first + (int64_t)(lane - 1) * 32);
    if (rp <= r_last) seg.insert(base + rp);
  }
  const int64_t e0 = segptr[base + r_first], e1 = segptr[base + r_last];
  for (int lane = 0; lane < 64; ++lane)
    for (int64_t p = e0 + (int64_t)lane * 32; p < e1; p += 64 * 32) ids.insert(p);
}

// the words a duty reads for chunk c (the kernel's loops over owned_touch_boundary / owned_touch_id); 1: out of range
static int duty_words(const OwnedPlan& pl, int64_t wg, int T, int chunk, int c, const std::vector<int32_t>& segptr, int64_t nnz,
                      Words& seg, Words& ids) {
  const OwnedTouchRows tr = owned_touch_rows(pl, wg, T, chunk, c);
  if (!tr.any) return 0;
  if (tr.slice < 0 || tr.slice >= pl.slices || tr.r_first < 0 || tr.r_first >= tr.r_last || tr.r_last > pl.n_dst)
    FAIL("chunk %d: rows [%lld, %lld) of slice %d", c, (long long)tr.r_first, (long long)tr.r_last, tr.slice);
  const int64_t base = (int64_t)tr.slice * pl.n_dst;
  bool ended = false;
  for (int64_t j = 0; j < 4096; ++j) {
    const int64_t rp = owned_touch_boundary(tr.r_first, tr.r_last, j);
    if (rp < 0) {
      ended = true;
      continue;
    }
    if (ended) FAIL("chunk %d: a boundary word behind a -1", c);
    if (rp < tr.r_first || rp > tr.r_last || base + rp >= (int64_t)segptr.size()) FAIL("chunk %d: boundary word %lld out of range", c, (long long)rp);
    seg.insert(base + rp);
  }
  if (!seg.count(base + tr.r_first) || !seg.count(base + tr.r_last)) FAIL("chunk %d: an end of the boundaries is not touched", c);
  for (int64_t line = (base + tr.r_first + 31) / 32; (line + 1) * 32 - 1 <= base + tr.r_last; ++line) {
    bool hit = false;
    for (int64_t wd = line * 32; wd < (line + 1) * 32; ++wd) hit = hit || seg.count(wd);
    if (!hit) FAIL("chunk %d: a whole line of boundaries is not touched", c);
  }
  const int64_t e0 = segptr[base + tr.r_first], e1 = segptr[base + tr.r_last];
  ended = false;
  Words mine;
  for (int64_t j = 0; j < (e1 - e0) / 32 + 70; ++j) {
    const int64_t p = owned_touch_id(e0, e1, j);
    if (p < 0) {
      ended = true;
      continue;
    }
    if (ended) FAIL("chunk %d: an id word behind a -1", c);
    if (p < e0 || p >= e1 || p >= nnz) FAIL("chunk %d: id word %lld out of [%lld, %lld)", c, (long long)p, (long long)e0, (long long)e1);
    mine.insert(p);
  }
  for (int64_t line = (e0 + 31) / 32; (line + 1) * 32 <= e1; ++line) {
    bool hit = false;
    for (int64_t wd = line * 32; wd < (line + 1) * 32; ++wd) hit = hit || mine.count(wd);
    if (!hit) FAIL("chunk %d: a whole line of ids is not touched", c);
  }
  ids.insert(mine.begin(), mine.end());
  return 0;
}

static int check(const OwnedPlan& pl, int64_t grid, const std::vector<int32_t>& segptr, int64_t nnz, int chunk, int lead, long* duties) {
  for (int64_t wg = 0; wg < grid; ++wg) {
    const int T = owned_wg_tasks(pl, wg);
    if (T == 0) {
      if (wg < pl.active) FAIL("an active workgroup without tasks");
      continue;
    }
    const int total = pl.phases * T, chunks = pl.phases * owned_touch_chunks(T, chunk), lead_chunks = owned_duty_lead_chunks(lead, chunk);
    std::vector<int> touched(chunks, 0);
    Words seg, ids;
    for (int k = 0; k < total + 40; ++k) {  // (+40: the slots the waves reserve past the last task)
      const int c = owned_duty_chunk(k, T, chunk, pl.phases);
      if (k >= total) {
        if (c != -1) FAIL("a slot past the last task carries a duty");
        continue;
      }
      const int t = k % T;
      if ((c >= 0) != (t % chunk == 0)) FAIL("slot %d: duty %d", k, c);
      if (c < 0) continue;
      if (c != (k / T) * owned_touch_chunks(T, chunk) + t / chunk) FAIL("slot %d is not the first slot of chunk %d", k, c);
      ++*duties;
      const OwnedDutySpan span = owned_duty_span(c, chunks, lead_chunks);
      if (span.first < 0 || span.first > span.end || span.end > chunks) FAIL("chunk %d: span [%d, %d) of %d", c, span.first, span.end, chunks);
      for (int cc = span.first; cc < span.end; ++cc) {
        if (cc < c) FAIL("chunk %d touches chunk %d behind it", c, cc);
        ++touched[cc];
        if (duty_words(pl, wg, T, chunk, cc, segptr, nnz, seg, ids)) return 1;
      }
    }
    for (int c = 0; c < chunks; ++c)
      if (touched[c] != 1) FAIL("wg %lld chunk %d of %d (chunk %d lead %d) is touched %d times", (long long)wg, c, chunks, chunk, lead, touched[c]);
    if (chunk == kOwnedTouchChunk) {
      Words tseg, tids;
      for (int c = 0; c < chunks; ++c) toucher_words(pl, wg, T, c, segptr, tseg, tids);
      if (tseg != seg || tids != ids) FAIL("wg %lld: the duties' words are not the toucher's (%zu / %zu boundaries, %zu / %zu ids)", (long long)wg, seg.size(), tseg.size(), ids.size(), tids.size());
    }
  }
  return 0;
}

int main() {
  struct Shape {
    int64_t n_dst, F, grid, cap;
    int lpr, R, slices;
  };
  const Shape shapes[] = {
      {3001, 128, 7, 0, 32, 0, 8},    {3001, 128, 7, 215, 32, 0, 8},  {3001, 128, 7, 0, 16, 0, 16}, {3001, 128, 19, 80, 16, 3, 8},
      {2000, 128, 5, 0, 8, 1, 8},     {2000, 256, 3, 0, 64, 0, 8},    {301, 128, 3, 0, 32, 0, 16},  {301, 100, 19, 0, 32, 2, 8},
      {40, 128, 64, 0, 32, 0, 8},     {5000, 128, 2, 0, 32, 1, 8},    {9000, 128, 4, 0, 32, 1, 3},
  };
  long plans = 0, duties = 0;
  for (const Shape& s : shapes) {
    const OwnedPlan pl = owned_plan(s.n_dst, s.F, s.lpr, s.grid, s.R, s.cap, 1, kOwnedPhaseTasks, s.slices, 4, kOwnedDutyWorkers);
    if (!pl.ok) FAIL("no plan for n_dst %lld", (long long)s.n_dst);
    // a slice-major layout: runs of empty rows, degrees 0 .. 40, a few long rows
    std::vector<int32_t> segptr((size_t)s.slices * s.n_dst + 1);
    int64_t nnz = 0;
    for (size_t i = 0; i + 1 < segptr.size(); ++i) {
      segptr[i] = (int32_t)nnz;
      const uint32_t r = rnd();
      nnz += (i / 37) % 5 == 0 ? 0 : (r % 97 == 0 ? 300 + r % 500 : r % 41);
    }
    segptr.back() = (int32_t)nnz;
    for (int chunk : {1, kOwnedTouchChunk, 8, 16, pl.tasks, pl.tasks + 3})  // (pl.tasks: the built-in, a duty per phase)
      for (int lead : {0, kOwnedTouchLead, 16, pl.tasks}) {
        if (check(pl, s.grid, segptr, nnz, chunk, lead, &duties)) {
          printf("n_dst %lld F %lld grid %lld lpr %d slices %d chunk %d lead %d\n", (long long)s.n_dst, (long long)s.F, (long long)s.grid, s.lpr, s.slices, chunk, lead);
          return 1;
        }
        ++plans;
      }
  }
  printf("walks %ld duties %ld\n", plans, duties);
  return 0;
}
"""

PLAN_PROGRAM = r"""
#include <cstdio>
#include "dgmi_owned_common.h"
using namespace dgmi;
int main() {
  // one workgroup, 32-lane groups (G = 2), R = round(rows / (G tasks)) with tasks = round(target workers / 15)
  const OwnedPlan p15 = owned_plan(120, 128, 32, 1, 0, 0), p16 = owned_plan(120, 128, 32, 1, 0, 0, 1, kOwnedPhaseTasks, 8, 4, kOwnedDutyWorkers);
  const OwnedPlan m15 = owned_plan(160, 128, 32, 1, 0, 0, 1, kOwnedPhaseTasksMult), m16 = owned_plan(160, 128, 32, 1, 0, 0, 1, kOwnedPhaseTasksMult, 8, 4, kOwnedDutyWorkers);
  const OwnedPlan same = owned_plan(120, 128, 32, 1, 0, 0, 1, kOwnedPhaseTasks, 8, 4, kOwnedWorkers);
  const OwnedPlan pair = owned_plan(120, 128, 32, 1, 0, 0, 2), pair11 = owned_plan(120, 128, 32, 1, 0, 0, 2, kOwnedPhaseTasks, 8, 4, kOwnedPairWaves - 1);
  const OwnedPlan bad = owned_plan(120, 128, 32, 1, 0, 0, 1, kOwnedPhaseTasks, 8, 4, kOwnedWaves + 1);
  printf("%d %d %d %d %d %d %d %d %d %d %d\n", kOwnedDutyWorkers, kOwnedPhaseTasks, kOwnedPhaseTasksMult, p15.R, p16.R, m15.R, m16.R, same.R,
         pair.R, pair11.R, (int)bad.ok);
  return 0;
}
"""


def _build_and_run(tmp_path, name, program, sanitize):
    src, exe = tmp_path / (name + ".cpp"), tmp_path / name
    src.write_text(program)
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    flags = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"] if sanitize else ["-O2"]
    cmd = [hipcc, "-x", "hip", "--cuda-host-only", "-std=c++17", "-I" + os.path.join(ROOT, "include"),
           "-I" + os.path.join(ROOT, "dream_gnn_amd", "csrc")] + flags + [str(src), "-o", str(exe)]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-4000:]
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    return r.stdout.strip()


@pytest.mark.parametrize("sanitize", [False, True], ids=["plain", "asan_ubsan"])
def test_duty_walk(tmp_path, sanitize):
    out = _build_and_run(tmp_path, "owned_duty_host", PROGRAM, sanitize)
    words = out.split()
    assert words[0] == "walks" and int(words[1]) == 11 * 6 * 4 and int(words[3]) > 10000, out


def test_plan_scales_its_task_target_with_the_workers(tmp_path):
    """``owned_plan``'s built-in R aims at ``round(target * workers / 15)`` tasks per phase: 24 -> 26 and 32 -> 34 for the
    duty form's sixteen workers.  120 rows of 2 lane groups: R = round(120 / 48) = 3 with a toucher, round(120 / 52) = 2
    without; 160 rows at the kNN-64 target: round(160 / 64) = 3 and round(160 / 68) = 2.  ``workers`` = 0 and the form's
    own count are the same plan, and a count above the workgroup's waves is no plan."""
    out = _build_and_run(tmp_path, "owned_duty_plan", PLAN_PROGRAM, False)
    duty_workers, target, target_mult, r15, r16, m15, m16, same, pair, pair11, bad_ok = (int(x) for x in out.split())
    assert (duty_workers, target, target_mult) == (16, 24, 32)
    assert (r15, r16, m15, m16) == (3, 2, 3, 2) and same == r15 and pair == pair11 and bad_ok == 0
