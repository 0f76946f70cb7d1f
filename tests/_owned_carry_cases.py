"""The hand-over of the gather window from task to task in the workgroup-owned SpMM (csrc/dgmi_owned_kernel.h; its index
arithmetic: ``owned_carry_*`` in csrc/dgmi_owned_common.h) on the graph designed for the window itself
(_owned_window_cases.py), with the order in which one wave runs the tasks of a workgroup restated on the host.  Plain
module, shared by test_owned_carry_host.py — which proves that every kind of consecutive pair of runs occurs under the
settings the GPU test uses — and test_gpu_spmm_owned_carry.py.

With ``sliced_owned_workers = 1`` one wave of a workgroup runs its tasks k, k + 1, k + 2, ... (phase-major: column
round, row round, slice; then the task slots of the phase), so lane group g hands its window from its run in task k to
its run in task k + 1 for every k; with 2 workers the pairs interleave, with 0 all 15 workers take tasks."""
from collections import namedtuple

import numpy as np

import _owned_window_cases as D
from oracle import oracle as O

WINDOW = D.WINDOW
WIDTHS, ROWS, ROUNDS = D.WIDTHS, D.ROWS, D.ROUNDS
GRIDS, WORKERS, FS = (1, 2), (1, 2, 0), (4, 128, 344)

Step = namedtuple("Step", "wg k phase col_round row_round slice task group row0 rows L last_id")


def lds_cap(rounds, grid):
    """``sliced_owned_lds_rows`` that cuts a workgroup's rows into ``rounds`` row rounds or more (0: no cap)."""
    B = -(-D.N_DST // grid)
    return 0 if rounds == 1 else -(-B // rounds)


def settings():
    """The knob settings the GPU test crosses with values, F and the layout of ``Y``."""
    return [dict(sliced_lpr=w, sliced_owned_rows=r, sliced_owned_grid=g, sliced_owned_lds_rows=lds_cap(k, g),
                 sliced_owned_workers=n, sliced_no_off32=o)
            for g in GRIDS for w in WIDTHS for r in ROWS for k in ROUNDS for n in WORKERS for o in (0, 1)]


def task_order(lpr, R_req, cap, grid, F, d=None):
    """Every (task, lane group) of every workgroup in the order ``k`` a single worker wave runs them, with the run's
    length and last source id: ``owned_plan`` / ``owned_phase`` / ``owned_task`` restated."""
    d = D.design() if d is None else d
    B, rounds, round_rows, R, G = D.plan(lpr, R_req, cap, D.N_DST, grid)
    col_rounds = -(-F // (4 * lpr))
    out = {}
    for wg in range(grid):
        own = max(0, min(B, D.N_DST - wg * B))
        T = -(-min(own, round_rows) // (G * R))
        steps = []
        for phase in range(col_rounds * rounds * D.N_SLICES):
            cq, s = divmod(phase, D.N_SLICES)
            cr, q = divmod(cq, rounds)
            in_round = max(0, min(round_rows, own - q * round_rows))
            for t in range(T):
                for g in range(G):
                    lds_row = (t * G + g) * R
                    rows = max(0, min(R, in_round - lds_row))
                    row0 = wg * B + q * round_rows + lds_row
                    L = int(d.seglen[s, row0:row0 + rows].sum()) if rows else 0
                    last = int(d.indices[d.segptr[s * D.N_DST + row0 + rows] - 1]) if L else -1
                    steps.append(Step(wg, phase * T + t, phase, cr, q, s, t, g, row0, rows, L, last))
        out[wg] = (T, G, steps)
    return out


def pairs(lpr, R_req, cap, grid, F, d=None):
    """The consecutive pairs (A, B) of runs of one lane group, tasks k and k + 1 of one workgroup."""
    out = []
    for wg, (T, G, steps) in task_order(lpr, R_req, cap, grid, F, d).items():
        by = {(st.k, st.group): st for st in steps}
        last_k = max(st.k for st in steps) if steps else -1
        for st in steps:
            out.append((st, by.get((st.k + 1, st.group)), st.k == last_k))
    return out


def kinds(lpr, R_req, cap, grid, F, d=None):
    """Which kinds of pair occur under a setting (the names test_owned_carry_host.py asks for)."""
    d = D.design() if d is None else d
    W = WINDOW
    seen = set()
    for a, b, is_last in pairs(lpr, R_req, cap, grid, F, d):
        if b is None:
            if is_last:
                seen.add("last task of the launch")
            continue
        same_phase = a.phase == b.phase
        if same_phase:
            if a.L > 0 and b.L > 0:
                seen.add("in phase: non-empty -> non-empty")
                seen.add("in phase: L_A %s multiple of W" % ("a" if a.L % W == 0 else "no"))
                if a.L < W and b.L < W:
                    seen.add("in phase: both shorter than W")
            if a.L > 0 and b.L == 0:
                seen.add("in phase: non-empty -> empty")
            if a.L == 0 and b.L > 0:
                seen.add("in phase: empty -> non-empty")
            if a.L > 0 and b.L > 0 and a.rows > 1 and b.rows > 1 and d.seglen[a.slice, a.row0 + a.rows - 1] == 0 \
                    and d.seglen[b.slice, b.row0] == 0:
                seen.add("in phase: trailing empty rows -> leading empty rows")
            if a.rows == 0 or b.rows == 0:
                seen.add("in phase: a task slot without rows")
        else:
            if b.slice == a.slice + 1 and a.L > 0 and b.L > 0:
                seen.add("across: next slice")
            if a.slice == D.N_SLICES - 1 and b.slice == 0 and b.row_round == a.row_round + 1:  # (with or without edges)
                seen.add("across: slice 7 -> slice 0 of the next row round")
            if b.col_round == a.col_round + 1 and a.L > 0 and b.L > 0:
                seen.add("across: next column round")
        if a.L > 0 and b.L > 0 and a.last_id == d.n_src - 1:
            seen.add("last id n_src - 1 before a hand-over")
        if a.L > 0 and 0 < b.L < W and b.last_id == d.n_src - 1:
            seen.add("last id n_src - 1 behind a hand-over, re-gathered by the clamp")
    return seen


# A second design, made FOR the geometry it runs under: 280 rows again, and every run (the rows one lane group sums in
# one task) of every workgroup and row round gets, slice by slice, the shape that makes its hand-over to the same lane
# group's run in the next task slot a wanted kind — so every kind occurs under every setting whose geometry allows it.
#   slice 0: 3 edges in the run's first row                    -> both runs shorter than W
#   slice 1: 5 edges in the first row of an even task slot, in the last row of an odd one
#                                                              -> a run ending in empty rows before one starting with them (R >= 2)
#   slice 2 / 3: 6 edges in the first row of even / odd task slots only -> non-empty -> empty and empty -> non-empty
#   slice 4 / 5 / 6: 8 / 9 / 33 edges in the first row         -> L_A a multiple of W, not one, a run of many groups
#   slice 7: 2 edges in the first row, the last one from source n_src - 1
#                                                              -> that row re-gathered by the clamp behind a hand-over
# Every run has edges in slices 0 and 7, so the steps into the next row round and the next column round hand over too.
_made = {}


def geometry(lpr, R_req, rounds, grid):
    """(workgroup, row round, task slot, lane group, first row, rows) of every run with rows, and the plan."""
    B, n_rounds, round_rows, R, G = D.plan(lpr, R_req, lds_cap(rounds, grid), D.N_DST, grid)
    out = []
    for wg in range(grid):
        own = max(0, min(B, D.N_DST - wg * B))
        T = -(-min(own, round_rows) // (G * R))
        for q in range(n_rounds):
            in_round = max(0, min(round_rows, own - q * round_rows))
            for t in range(T):
                for g in range(G):
                    lds_row = (t * G + g) * R
                    rows = max(0, min(R, in_round - lds_row))
                    if rows:
                        out.append((wg, q, t, g, wg * B + q * round_rows + lds_row, rows))
    return out, (B, n_rounds, round_rows, R, G)


def made_design(lpr, R_req, rounds, grid):
    key = (lpr, R_req, rounds, grid)
    if key in _made:
        return _made[key]
    rng = np.random.default_rng(7 + 1000 * lpr + 100 * R_req + 10 * rounds + grid)
    width = D.N_SRC // D.N_SLICES
    seglen = np.zeros((D.N_SLICES, D.N_DST), np.int64)
    runs, _ = geometry(lpr, R_req, rounds, grid)
    for wg, q, t, g, row0, rows in runs:
        first, last = row0, row0 + rows - 1
        seglen[0, first] = 3
        seglen[1, first if t % 2 == 0 else last] = 5
        seglen[2 + t % 2, first] = 6
        seglen[4, first], seglen[5, first], seglen[6, first], seglen[7, first] = 8, 9, 33, 2
    dst, src = [], []
    for s in range(D.N_SLICES):
        for row in range(D.N_DST):
            n = int(seglen[s, row])
            ids = rng.integers(s * width, (s + 1) * width, n)
            if n and s == D.N_SLICES - 1:
                ids[-1] = D.N_SRC - 1
            dst.append(np.full(n, row))
            src.append(ids)
    dst, src = np.concatenate(dst).astype(np.int32), np.concatenate(src).astype(np.int32)
    segptr, indices, _ = O.csr_sliced_from_coo(dst, src, D.N_DST, D.N_SRC, D.N_SLICES)  # (stable: a segment's last edge stays last)
    assert np.array_equal(np.diff(segptr.astype(np.int64)).reshape(D.N_SLICES, D.N_DST), seglen)
    d = D.Design(D.N_DST, D.N_SRC, dst, src, rng.integers(1, 9, dst.size).astype(np.int32), seglen, segptr, indices)
    for a in d:
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    _made[key] = d
    return d


ALL_KINDS = ("in phase: non-empty -> non-empty", "in phase: L_A a multiple of W", "in phase: L_A no multiple of W",
             "in phase: both shorter than W", "in phase: non-empty -> empty", "in phase: empty -> non-empty",
             "in phase: trailing empty rows -> leading empty rows", "in phase: a task slot without rows",
             "across: next slice", "across: slice 7 -> slice 0 of the next row round", "across: next column round",
             "last task of the launch", "last id n_src - 1 before a hand-over",
             "last id n_src - 1 behind a hand-over, re-gathered by the clamp")


def possible_kinds(lpr, R_req, rounds, grid):
    """The kinds of pair the geometry of a setting allows (over F = 4 / 128 / 344), each with the reason it may be
    missing: a pure function of the plan, not of any graph."""
    runs, (B, n_rounds, round_rows, R, G) = geometry(lpr, R_req, rounds, grid)
    out = {"in phase: non-empty -> non-empty", "in phase: L_A a multiple of W", "in phase: L_A no multiple of W",
           "in phase: both shorter than W", "in phase: non-empty -> empty", "in phase: empty -> non-empty",
           "across: next slice", "last task of the launch", "last id n_src - 1 before a hand-over",
           "last id n_src - 1 behind a hand-over, re-gathered by the clamp"}
    if R >= 2:  # a run of one row has no empty row beside one with edges
        out.add("in phase: trailing empty rows -> leading empty rows")
    if n_rounds >= 2:  # one row round: slice 7 is followed by the next column round, or by nothing
        out.add("across: slice 7 -> slice 0 of the next row round")
    if max(-(-F // (4 * lpr)) for F in FS) >= 2:
        out.add("across: next column round")
    # a task slot without rows: some lane group of a workgroup's last slot of some row round lies past the round's rows
    with_rows = {(wg, q, t, g) for wg, q, t, g, _, _ in runs}
    slots = {(wg, q, t) for wg, q, t, _, _, _ in runs}
    if any((wg, q, t, g) not in with_rows for wg, q, t in slots for g in range(G)) or \
            any((wg, q) not in {(w2, q2) for w2, q2, _ in slots} for wg in range(grid) for q in range(n_rounds)):
        out.add("in phase: a task slot without rows")
    return out
