"""A graph designed for the rolling gather window of the workgroup-owned SpMM (csrc/dgmi_owned_kernel.h; the window's index
arithmetic: csrc/dgmi_owned_common.h), and the plan of the forced form restated on the host.  Plain module (like
_spmm_cases.py), shared by test_owned_window_host.py — which checks that the design covers what it claims, for every
setting the GPU test runs — and test_gpu_spmm_owned_window.py.

280 destination rows, 160 sources in 8 slices of 20 columns, 2 workgroups of 140 rows (``sliced_owned_grid = 2``), so
that a lane group's RUN — the R consecutive rows one lane group sums for one slice, back to back through one window —
starts at a multiple of 5 and of 2 whether the workgroup's rows take one row round or two.

* rows 0 .. 139 (workgroup 0), dense: segment (row, slice) has ``LENGTHS[(row + row // 14 + 3 slice) % 14]`` edges, so
  every length occurs in every slice as the first, a middle and the last row of a 5-row run, and as either row of a 2-row run;
* rows 140 .. 179 and 260 .. 279 (workgroup 1), sparse: 5-row patterns of ``SPARSE`` — runs shorter than the window, runs
  that are an exact multiple of the window and of 8 / 16 / 32 / 64 edges, runs that end in empty rows, a run whose only edge is its last row's;
* rows 180 .. 259: empty in every slice — whole tasks without an edge at every lane-group width;
* the last edge of every non-empty segment of slice 7 in rows 260 .. 279 reads source ``n_src - 1``: an edge issued past
  the end of such a run gathers the table's last row again.

Operands are small integers (``X`` in [-8, 8], multiplicities 1 .. 8): a row has at most 8 * 65 edges, so every partial
sum stays below 8 * 8 * 520 = 33 280 < 2**24 and is exact in fp32 in any order (``reference`` asserts it)."""
from collections import namedtuple

import numpy as np

from oracle import oracle as O

LENGTHS = (0, 1, 7, 8, 9, 15, 16, 17, 31, 32, 33, 63, 64, 65)
N_DST, N_SRC, N_SLICES, GRID = 280, 160, 8, 2
DENSE_ROWS = 140
EMPTY_ROWS = (180, 260)  # [first, last)
SPARSE = ((8, 0, 0, 0, 0), (1, 0, 1, 0, 0), (16, 16, 0, 0, 0), (31, 33, 0, 0, 0), (7, 0, 0, 0, 0), (0, 0, 0, 0, 1),
          (64, 0, 0, 0, 0), (32, 0, 0, 0, 0), (0, 0, 0, 0, 0), (0, 16, 0, 0, 0), (0, 0, 8, 0, 0), (1, 1, 1, 1, 1))
LDS_ROW_BYTES = 144 << 10  # kOwnedLdsRowBytes
WINDOW = 4                 # kOwnedWindow
WIDTHS, ROWS, ROUNDS = (8, 16, 32, 64), (1, 2, 5), (1, 2)

Design = namedtuple("Design", "n_dst n_src dst src mult seglen segptr indices")
Run = namedtuple("Run", "wg task group slice row0 rows")

_design = None


def design():
    global _design
    if _design is not None:
        return _design
    rng = np.random.default_rng(2024)
    width = N_SRC // N_SLICES
    seglen = np.zeros((N_SLICES, N_DST), np.int64)
    for s in range(N_SLICES):
        for row in range(DENSE_ROWS):
            seglen[s, row] = LENGTHS[(row + row // 14 + 3 * s) % 14]
        sparse_rows = list(range(DENSE_ROWS, EMPTY_ROWS[0])) + list(range(EMPTY_ROWS[1], N_DST))
        for k in range(0, len(sparse_rows), 5):
            pattern = SPARSE[(k // 5 + s) % len(SPARSE)]
            for j, row in enumerate(sparse_rows[k:k + 5]):
                seglen[s, row] = pattern[j]
    dst, src = [], []
    for s in range(N_SLICES):
        for row in range(N_DST):
            n = int(seglen[s, row])
            ids = rng.integers(s * width, (s + 1) * width, n)
            if n and s == N_SLICES - 1 and row >= EMPTY_ROWS[1]:
                ids[-1] = N_SRC - 1
            dst.append(np.full(n, row))
            src.append(ids)
    dst, src = np.concatenate(dst).astype(np.int32), np.concatenate(src).astype(np.int32)
    # The layout builder sorts by (slice, row), stably: shuffle whole segments only, so a segment's last edge stays its last.
    seg_key = (src // width).astype(np.int64) * N_DST + dst
    order = np.argsort(rng.permutation(N_SLICES * N_DST)[seg_key], kind="stable")
    dst, src = dst[order], src[order]
    segptr, indices, _ = O.csr_sliced_from_coo(dst, src, N_DST, N_SRC, N_SLICES)
    assert np.array_equal(np.diff(segptr.astype(np.int64)).reshape(N_SLICES, N_DST), seglen)
    _design = Design(N_DST, N_SRC, dst, src, rng.integers(1, 9, dst.size).astype(np.int32), seglen, segptr, indices)
    for a in _design:
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return _design


def lds_cap(rounds):
    """``sliced_owned_lds_rows`` that gives a workgroup's 140 rows ``rounds`` row rounds (0: no cap)."""
    B = -(-N_DST // GRID)
    return 0 if rounds == 1 else -(-B // rounds)


def settings():
    """The knob settings the GPU test crosses with values, F and the layout of ``Y``."""
    return [dict(sliced_lpr=w, sliced_owned_rows=r, sliced_owned_grid=GRID, sliced_owned_lds_rows=lds_cap(k), sliced_no_off32=o)
            for w in WIDTHS for r in ROWS for k in ROUNDS for o in (0, 1)]


def plan(lpr, R_req, cap, n_dst=N_DST, grid=GRID):
    """``owned_plan`` (csrc/dgmi_owned_common.h) for a forced R, restated: (B, row rounds, rows per round, R, G)."""
    B = -(-n_dst // grid)
    fit = LDS_ROW_BYTES // (16 * lpr)
    if 0 < cap < fit:
        fit = cap
    rounds = -(-B // fit)
    return B, rounds, -(-B // rounds), max(1, min(R_req, lpr - 1)), 64 // lpr


def runs(lpr, R_req, cap):
    """Every run of the forced form under a setting: one per (workgroup, row round, task slot, lane group, slice), the
    empty task slots of a short round included (``rows`` = 0)."""
    B, rounds, round_rows, R, G = plan(lpr, R_req, cap)
    tasks = -(-round_rows // (G * R))
    out = []
    for wg in range(GRID):
        own = max(0, min(B, N_DST - wg * B))
        for q in range(rounds):
            in_round = max(0, min(round_rows, own - q * round_rows))
            for t in range(tasks):
                for g in range(G):
                    lds_row = (t * G + g) * R
                    rows = max(0, min(R, in_round - lds_row))
                    for s in range(N_SLICES):
                        out.append(Run(wg, q * tasks + t, g, s, wg * B + q * round_rows + lds_row, rows))
    return out


def reference(d, X, mult=None):
    """``A X`` in int64 over the COO list, as float32; asserts that every partial sum is exact in fp32."""
    w = np.ones(d.dst.size, np.int64) if mult is None else np.asarray(mult, np.int64)
    terms = X[d.src].astype(np.int64) * w[:, None]
    y = np.zeros((d.n_dst, X.shape[1]), np.int64)
    np.add.at(y, d.dst, terms)
    bound = np.zeros_like(y)
    np.add.at(bound, d.dst, np.abs(terms))
    assert np.array_equal(X, np.rint(X)) and bound.max() < 2 ** 24, "the design leaves fp32's exact range"
    return y.astype(np.float32)
