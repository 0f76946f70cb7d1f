"""The hand-over of the gather window from task to task in the workgroup-owned SpMM, on the host (no GPU).

(1) A stand-alone C++ program includes csrc/dgmi_owned_common.h — the header the kernel takes the hand-over's index
arithmetic from (``owned_carry``, ``owned_carry_slot_edge``, ``owned_carry_read_group``, ``owned_carry_start_batch``) —
and walks the schedule the kernel follows for every pair of run lengths (L_A, L_B) in {0 .. 2 W + 1} u {15, 16, 17, 31,
32, 33} and every lane-group width: run A from a cold start, the hand-over, run B to its end.  Every issued edge is a
valid edge of the right run; every edge of B is issued exactly once, by the carry or by the cold prologue, and consumed
in order; no id is read from a run without edges; B's batch 0 is read no sooner than a window of gathers after its
request unless ``owned_carry_read_group`` says the run is too short (-1).  Built and run twice: plainly, and with the
address and undefined-behaviour sanitizers.

(2) The graphs contain the kinds of consecutive pair the GPU test relies on.  The window's graph, under EVERY setting:
non-empty -> non-empty with L_A a multiple of W and not, non-empty -> empty, empty -> non-empty, a pair across two
slices, the last task of the launch, a last source id of ``n_src - 1`` right before a hand-over.  The graph MADE for a
setting (``made_design``), under that setting: every kind — also both runs shorter than W, a run ending in empty rows
before one starting with them, task slots without rows, slice 7 -> slice 0 of the next row round, the step into the next
column round (both runs with edges), an ``n_src - 1`` re-gathered by the clamp behind a hand-over — unless the geometry
rules it out, and then for exactly the reason ``possible_kinds`` gives: R = 1 has no empty row beside one with edges, one
row round has no next one, a round that fills its task slots has none without rows."""
import os
import subprocess

import pytest

import _owned_carry_cases as C

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

PROGRAM = r"""
#include <cstdio>
#include <vector>
#include "dgmi_owned_common.h"

using namespace dgmi;

#define FAIL(msg)                                                          \
  do {                                                                     \
    printf("lpr %d L_A %d L_B %d: %s\n", lpr, La, Lb, msg);                \
    return 1;                                                              \
  } while (0)

// One run of L edges whose window is `warm` (slots 0 .. W - 1 hold its edges 0 .. W - 1, clamped) or cold; `Ln`: the
// run it hands its window to.  Counts issues and consumptions of its own edges in `issued` / `consumed` (a warm run's
// first W were counted by the run before) and those of the next run in `next_issued`.
static int walk(int lpr, int La, int Lb, int L, int Ln, bool warm, std::vector<int>& issued, std::vector<int>& consumed,
                std::vector<int>& next_issued, bool* carried_out) {
  const int W = kOwnedWindow;
  *carried_out = false;
  if (L == 0) return 0;  // the kernel sums nothing and issues nothing; the next run starts cold
  const int groups = owned_window_groups(L);
  long gathers = 0;
  std::vector<int> slot(W, -1);  // the edge of this run each slot holds
  if (warm) {
    for (int u = 0; u < W; ++u) slot[u] = owned_carry_slot_edge(u, L);
  } else {
    for (int lane = 0; lane < lpr; ++lane) {
      const int e = owned_window_id_edge(0, lane, L);
      if (e < 0 || e >= L) FAIL("a lane of the cold batch 0 loads no valid edge");
    }
    for (int u = 0; u < W; ++u) {
      slot[u] = owned_window_id_edge(0, u, L);
      if (u < L) ++issued[u];
      ++gathers;
    }
  }
  if (owned_carry_start_batch() != owned_window_issue_batch(0)) FAIL("the id register does not start with group 0's batch");
  // the next run's batches 0 and 1 are requested at the top of this run
  const long requested_at = gathers;
  const bool carry = owned_carry(L, Ln);
  if (carry && (L <= 0 || Ln <= 0)) FAIL("a window is carried out of or into a run without edges");
  if (!carry && L > 0 && Ln > 0) FAIL("two runs with edges do not hand over");
  bool read_next = false;
  const int read_group = owned_carry_read_group(L);
  if (read_group >= groups - 1 && read_group >= 0) FAIL("the read group is the run's last group or past it");
  int next_edge = 0;
  for (int g = 0; g < groups; ++g) {
    const bool last = g == groups - 1;
    if (last && carry && !read_next) {
      if (read_group != -1) FAIL("the next batch was not read before the last group");
      read_next = true;  // (waits: the function has said so)
    }
    for (int u = 0; u < W; ++u) {
      const int e = g * W + u;
      if (e < L) {
        if (slot[u] != e) FAIL("a slot does not hold the edge that is consumed next");
        if (e != next_edge) FAIL("edges are not consumed in order");
        ++next_edge;
        ++consumed[e];
      }
      if (!last) {
        const int batch = owned_window_issue_batch(g);
        const int ne = owned_window_id_edge(batch, u, L);
        if (ne < 0 || ne >= L) FAIL("an issue names no valid edge of the run");
        const int stands_for = (g + 1) * W + u;
        if (stands_for < L) {
          if (ne != stands_for) FAIL("an issue gathers another edge's row");
          ++issued[ne];
        } else if (ne != L - 1) {
          FAIL("an issue past the end does not repeat the run's last edge");
        }
        slot[u] = ne;
        ++gathers;
      } else if (carry) {
        if (!read_next) FAIL("a slot is refilled from a batch that was not read");
        const int ne = owned_carry_slot_edge(u, Ln);
        if (ne < 0 || ne >= Ln) FAIL("a carried issue names no valid edge of the next run");
        if (u < Ln) {
          if (ne != u) FAIL("slot u does not take edge u of the next run");
          ++next_issued[ne];
        } else if (ne != Ln - 1) {
          FAIL("a carried issue past the end does not repeat the next run's last edge");
        }
        ++gathers;
      }
    }
    if (g == read_group && carry) {
      if (gathers - requested_at < W) FAIL("the next batch 0 is read less than a window after its request");
      read_next = true;
    }
  }
  if (next_edge != L) FAIL("not every edge was consumed");
  *carried_out = carry;
  return 0;
}

static int pair(int lpr, int La, int Lb) {
  std::vector<int> ia(La, 0), ca(La, 0), ib(Lb, 0), cb(Lb, 0), none;
  bool carried = false, unused = false;
  if (walk(lpr, La, Lb, La, Lb, false, ia, ca, ib, &carried)) return 1;
  if (carried != owned_carry(La, Lb)) FAIL("carried");
  if (walk(lpr, La, Lb, Lb, 0, carried, ib, cb, none, &unused)) return 1;
  if (unused) FAIL("a window is carried past the last run");
  for (int e = 0; e < La; ++e)
    if (ia[e] != 1 || ca[e] != 1) FAIL("an edge of A is not issued and consumed exactly once");
  for (int e = 0; e < Lb; ++e)
    if (ib[e] != 1 || cb[e] != 1) FAIL("an edge of B is not issued and consumed exactly once");
  return 0;
}

int main() {
  const int W = kOwnedWindow;
  std::vector<int> lengths;
  for (int L = 0; L <= 2 * W + 1; ++L) lengths.push_back(L);
  for (int L : {15, 16, 17, 31, 32, 33}) lengths.push_back(L);
  int pairs = 0;
  for (int lpr : {8, 16, 32, 64})
    for (int La : lengths)
      for (int Lb : lengths) {
        if (pair(lpr, La, Lb)) return 1;
        ++pairs;
      }
  printf("pairs %d window %d\n", pairs, W);
  return 0;
}
"""

N_LENGTHS = 2 * C.WINDOW + 2 + 6


@pytest.mark.parametrize("sanitize", [False, True], ids=["plain", "asan_ubsan"])
def test_hand_over_walk(tmp_path, sanitize):
    src, exe = tmp_path / "owned_carry_host.cpp", tmp_path / "owned_carry_host"
    src.write_text(PROGRAM)
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    flags = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"] if sanitize else ["-O2"]
    cmd = [hipcc, "-x", "hip", "--cuda-host-only", "-std=c++17", "-I" + os.path.join(ROOT, "include"),
           "-I" + os.path.join(ROOT, "dream_gnn_amd", "csrc")] + flags + [str(src), "-o", str(exe)]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-4000:]
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert r.stdout.strip() == "pairs %d window %d" % (4 * N_LENGTHS ** 2, C.WINDOW), r.stdout


EVERYWHERE = ("in phase: non-empty -> non-empty", "in phase: L_A a multiple of W", "in phase: L_A no multiple of W",
              "in phase: non-empty -> empty", "in phase: empty -> non-empty", "across: next slice",
              "last task of the launch", "last id n_src - 1 before a hand-over")


@pytest.mark.parametrize("grid", C.GRIDS)
@pytest.mark.parametrize("rounds", C.ROUNDS)
@pytest.mark.parametrize("R", C.ROWS)
@pytest.mark.parametrize("lpr", C.WIDTHS)
def test_designs_have_the_pairs_under_every_setting(lpr, R, rounds, grid):
    """The window's graph holds the plain kinds under every setting; the graph made for the setting holds EVERY kind its
    geometry allows, and nothing is missing but what ``possible_kinds`` rules out with its reason."""
    seen = set().union(*(C.kinds(lpr, R, C.lds_cap(rounds, grid), grid, F) for F in C.FS))
    for kind in EVERYWHERE:
        assert kind in seen, kind
    d = C.made_design(lpr, R, rounds, grid)
    made = set().union(*(C.kinds(lpr, R, C.lds_cap(rounds, grid), grid, F, d) for F in C.FS))
    possible = C.possible_kinds(lpr, R, rounds, grid)
    assert made == possible, (sorted(possible - made), sorted(made - possible))
    # what a geometry can rule out, and nothing else
    ruled_out = set(C.ALL_KINDS) - possible
    assert ruled_out <= {"in phase: trailing empty rows -> leading empty rows", "in phase: a task slot without rows",
                         "across: slice 7 -> slice 0 of the next row round"}
    assert ("in phase: trailing empty rows -> leading empty rows" in ruled_out) == (min(R, lpr - 1) == 1)
    assert ("across: slice 7 -> slice 0 of the next row round" in ruled_out) == (C.D.plan(lpr, R, C.lds_cap(rounds, grid), C.D.N_DST, grid)[1] == 1)
    assert "across: next column round" in made  # F = 344: two column rounds or more at every width


@pytest.mark.parametrize("F", C.FS)
def test_made_designs_stay_exact(F):
    import numpy as np

    d = C.made_design(8, 5, 2, 2)
    X = np.random.default_rng(F).integers(-8, 9, (d.n_src, F)).astype(np.float32)
    for mult in (None, d.mult):
        assert C.D.reference(d, X, mult).dtype == np.float32  # (asserts the bound on the partial sums)
    assert int(d.indices.max()) == d.n_src - 1


def test_settings_cross_what_they_claim():
    s = C.settings()
    assert len(s) == len(C.GRIDS) * len(C.WIDTHS) * len(C.ROWS) * len(C.ROUNDS) * len(C.WORKERS) * 2
    assert {k["sliced_owned_workers"] for k in s} == {0, 1, 2} and {k["sliced_owned_grid"] for k in s} == {1, 2}
    # F = 344 at 8-lane groups: 11 column rounds
    assert -(-344 // (4 * 8)) == 11
