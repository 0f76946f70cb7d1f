"""The rolling gather window of the workgroup-owned SpMM on the host (no GPU).

(1) A stand-alone C++ program includes csrc/dgmi_owned_common.h — the header the kernel takes the window's index
arithmetic from — and walks the schedule the kernel follows, for every lane-group width and every run length
0 .. 3 LPR + 9: every edge is issued exactly once and before it is consumed, no id
is read from a batch that has not been requested (and a batch requested inside the run is read no sooner than a full
window of gathers later), every lane's id load and every edge issued past the end names a valid edge of the same run.
Built and run twice: plainly, and with the address and undefined-behaviour sanitizers.  It also prints ``owned_plan`` for
the settings of the GPU test, which (2) compares with the restatement in _owned_window_cases.py.

(3) The designed graph of _owned_window_cases.py covers what it claims under every setting test_gpu_spmm_owned_window.py
runs, and its integer operands keep every partial sum exact in fp32."""
import os
import subprocess

import numpy as np
import pytest

import _owned_window_cases as D

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

PROGRAM = r"""
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "dgmi_owned_common.h"

using namespace dgmi;

static int walk(int lpr, int L) {
  const int W = kOwnedWindow;
#define FAIL(msg)                                                      \
  do {                                                                 \
    printf("W %d lpr %d L %d: %s\n", W, lpr, L, msg);                  \
    return 1;                                                          \
  } while (0)
  const int groups = owned_window_groups(L);
  if (groups != (L + W - 1) / W) FAIL("groups");
  if (L == 0) return 0;  // the kernel skips a run without edges
  std::vector<int> issued(L, 0), consumed(L, 0);
  std::vector<long> requested_at(groups + kOwnedWindowFirstBatches + 1, -1);  // gathers issued when a batch was requested
  std::vector<char> first(groups + kOwnedWindowFirstBatches + 1, 0);
  long gathers = 0;
  // what every lane of the group loads for a batch, and what an issue reads out of it
  auto load_batch = [&](int batch) {
    for (int lane = 0; lane < lpr; ++lane) {
      const int e = owned_window_id_edge(batch, lane, L);
      if (e < 0 || e >= L) return false;
      if (e != owned_window_id_edge(batch, lane % W, L)) return false;
    }
    return true;
  };
  auto issue = [&](int batch, int u, int edge) {  // `edge`: the edge this issue stands for (may lie past the end)
    if (requested_at[batch] < 0) return "an id is read from a batch that was not requested";
    if (!first[batch] && gathers - requested_at[batch] < W) return "a batch is read less than a window after its request";
    const int e = owned_window_id_edge(batch, u, L);
    if (e < 0 || e >= L) return "an issue names no valid edge of the run";
    if (edge < L) {
      if (e != edge) return "an issue gathers another edge's row";
      ++issued[edge];
    } else if (e != L - 1) {
      return "an issue past the end does not repeat the run's last edge";
    }
    ++gathers;
    return (const char*)nullptr;
  };
  // before the run: batches 0 and 1; the prologue issues edges 0 .. W - 1 out of batch 0
  for (int b = 0; b < kOwnedWindowFirstBatches; ++b) {
    if (!load_batch(b)) FAIL("a lane of a first batch loads no valid edge");
    requested_at[b] = 0;
    first[b] = 1;
  }
  for (int u = 0; u < W; ++u)
    if (const char* err = issue(0, u, u)) FAIL(err);
  int reg = 1;  // the batch in the id register
  for (int g = 0; g + 1 < groups; ++g) {
    const int batch = owned_window_issue_batch(g);
    if (batch != reg) FAIL("the id register does not hold the batch the group's issues read");
    if (requested_at[batch] < 0) FAIL("the group reads a batch that was not requested");
    if (!first[batch] && gathers - requested_at[batch] < W) FAIL("the register is read less than a window after its request");
    const int next = owned_window_request_batch(g);
    if (next >= (int)requested_at.size() || requested_at[next] >= 0) FAIL("a batch is requested twice or out of range");
    if (next != owned_window_issue_batch(g + 1)) FAIL("the request is not the next group's batch");
    if (!load_batch(next)) FAIL("a lane of a requested batch loads no valid edge");
    // (the ids of this group's issues have left the register before the request overwrites it)
    const long at = gathers;
    for (int u = 0; u < W; ++u) {
      const int e = g * W + u;
      if (e >= L) FAIL("a group that issues is not full");
      if (issued[e] != 1 || consumed[e] != 0) FAIL("an edge is consumed before it was issued, or twice");
      ++consumed[e];
      if (const char* err = issue(batch, u, (g + 1) * W + u)) FAIL(err);
    }
    requested_at[next] = at;
    reg = next;
  }
  for (int u = 0; u < W; ++u) {  // the last group only consumes
    const int e = (groups - 1) * W + u;
    if (e >= L) break;
    if (issued[e] != 1 || consumed[e] != 0) FAIL("an edge of the last group was not issued, or consumed twice");
    ++consumed[e];
  }
  for (int e = 0; e < L; ++e)
    if (issued[e] != 1 || consumed[e] != 1) FAIL("an edge is not issued and consumed exactly once");
  return 0;
#undef FAIL
}

int main(int argc, char** argv) {
  static_assert(kOwnedWindow >= 1 && kOwnedWindow <= 8, "at most eight 4-bit multiplicity fields in a register");
  int walks = 0;
  for (int lpr : {8, 16, 32, 64}) {
    if (lpr % kOwnedWindow != 0) {
      printf("the window does not divide width %d\n", lpr);
      return 1;
    }
    for (int L = 0; L <= 3 * lpr + 9; ++L) {
      if (walk(lpr, L)) return 1;
      ++walks;
    }
  }
  printf("walks %d window %d lds_row_bytes %lld\n", walks, kOwnedWindow, (long long)kOwnedLdsRowBytes);
  // owned_plan for the settings given as (lpr R cap) triples: n_dst and grid first
  const long n_dst = atol(argv[1]), grid = atol(argv[2]);
  for (int i = 3; i + 2 < argc; i += 3) {
    const OwnedPlan p = owned_plan(n_dst, 128, atoi(argv[i]), grid, atoi(argv[i + 1]), atol(argv[i + 2]));
    printf("plan %d %lld %d %d %d %d %d\n", (int)p.ok, (long long)p.wg_rows, p.row_rounds, p.round_rows, p.R, p.G, p.tasks);
  }
  return 0;
}
"""

WALKS = sum(3 * w + 10 for w in D.WIDTHS)
TRIPLES = [(w, r, D.lds_cap(k)) for w in D.WIDTHS for r in D.ROWS for k in D.ROUNDS]


@pytest.mark.parametrize("sanitize", [False, True], ids=["plain", "asan_ubsan"])
def test_window_walk_and_plan(tmp_path, sanitize):
    src, exe = tmp_path / "owned_window_host.cpp", tmp_path / "owned_window_host"
    src.write_text(PROGRAM)
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    flags = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"] if sanitize else ["-O2"]
    cmd = [hipcc, "-x", "hip", "--cuda-host-only", "-std=c++17", "-I" + os.path.join(ROOT, "include"),
           "-I" + os.path.join(ROOT, "dream_gnn_amd", "csrc")] + flags + [str(src), "-o", str(exe)]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-4000:]
    args = [str(D.N_DST), str(D.GRID)] + [str(x) for t in TRIPLES for x in t]
    r = subprocess.run([str(exe)] + args, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    lines = r.stdout.strip().splitlines()
    assert lines[0] == "walks %d window %d lds_row_bytes %d" % (WALKS, D.WINDOW, D.LDS_ROW_BYTES), lines[0]
    assert len(lines) == 1 + len(TRIPLES)
    for (lpr, R, cap), line in zip(TRIPLES, lines[1:]):
        B, rounds, round_rows, R_eff, G = D.plan(lpr, R, cap)
        tasks = -(-round_rows // (G * R_eff))
        assert line == "plan 1 %d %d %d %d %d %d" % (B, rounds, round_rows, R_eff, G, tasks), (lpr, R, cap, line)


def _run_lengths(d, run):
    return d.seglen[run.slice, run.row0:run.row0 + run.rows]


@pytest.mark.parametrize("rounds", D.ROUNDS)
@pytest.mark.parametrize("R", D.ROWS)
@pytest.mark.parametrize("lpr", D.WIDTHS)
def test_design_covers_what_it_claims(lpr, R, rounds):
    d = D.design()
    assert 100 <= d.n_dst <= 300 and set(np.unique(d.seglen).tolist()) <= set(D.LENGTHS)
    assert D.plan(lpr, R, D.lds_cap(rounds))[1] == rounds
    runs = D.runs(lpr, R, D.lds_cap(rounds))
    covered = np.zeros((D.N_SLICES, d.n_dst), np.int64)
    where = {"first": set(), "middle": set(), "last": set()}
    multiple = short = trailing = last_id = last_id_ragged = False
    tasks = {}
    for run in runs:
        lens = _run_lengths(d, run)
        covered[run.slice, run.row0:run.row0 + run.rows] += 1
        total = int(lens.sum())
        if run.rows:
            key = (run.wg, run.task, run.slice)
            tasks[key] = tasks.get(key, 0) + total
        if run.rows == R:
            where["first"].add((run.slice, int(lens[0])))
            where["last"].add((run.slice, int(lens[-1])))
            where["middle"].update((run.slice, int(n)) for n in lens[1:-1])
        multiple |= total > 0 and total % D.WINDOW == 0 and total % lpr == 0
        short |= 0 < total < D.WINDOW
        trailing |= total > 0 and run.rows > 1 and lens[-1] == 0
        if total > 0:
            last = d.indices[d.segptr[run.slice * d.n_dst + run.row0 + run.rows] - 1]
            last_id |= last == d.n_src - 1
            last_id_ragged |= last == d.n_src - 1 and total % D.WINDOW != 0
    assert np.all(covered == 1), "the restated plan does not cover every (row, slice) once"
    every = {(s, n) for s in range(D.N_SLICES) for n in D.LENGTHS}
    assert where["first"] >= every and where["last"] >= every, "a length is missing as first / last row of a run in a slice"
    if R >= 3:
        assert where["middle"] >= every, "a length is missing as a middle row of a run in a slice"
    assert multiple, "no run is a multiple of the window and of the lane-group width"
    assert short, "no run is shorter than the window"
    assert trailing or R == 1, "no run ends in empty rows"
    assert any(total == 0 for total in tasks.values()), "no wholly empty task"
    assert last_id and last_id_ragged, "no run ends at source n_src - 1 (one of them not a multiple of the window)"


@pytest.mark.parametrize("F", [4, 128, 344])
def test_integer_operands_stay_exact(F):
    d = D.design()
    X = np.random.default_rng(F).integers(-8, 9, (d.n_src, F)).astype(np.float32)
    for mult in (None, d.mult):
        y = D.reference(d, X, mult)  # asserts the bound on the partial sums
        assert y.dtype == np.float32 and np.abs(y).max() < 2 ** 24
    assert d.mult.min() == 1 and d.mult.max() == 8 and int(d.indices.max()) == d.n_src - 1
