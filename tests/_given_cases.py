"""The documented rank of a GIVEN pair restated on the host, and the planner of the count scan (ops.pair_mlp_rank_list,
csrc/dgmi_pairs_given.hip).  Plain module (like _rank_cases.py), shared by test_given_cases_host.py and
test_gpu_given.py.

For a listed pair (q, c) of an (n_query, n_cand) logit table ``L``: ``total`` counts the candidates ``c' != c`` with
``(q, c')`` not known, ``above`` those of them that rank before ``(q, c)``: logit descending, ties by candidate id
ascending, NaN after every number, -0 equal to +0.  The listed pair never counts itself and is ranked whether or not
it is known.  A listed id outside the table gives logit NaN and ``above = total = -1``."""
import numpy as np


def expected_ranks(L, known, pair_q, pair_c):
    """``(logit, above, total)`` of the listed pairs: float32, int64, int64 arrays in the caller's order.  ``L``:
    (n_query, n_cand) float32 table; ``known``: bool mask of the same shape, or None."""
    L = np.ascontiguousarray(L, dtype=np.float32)
    n_query, n_cand = L.shape
    pair_q, pair_c = np.asarray(pair_q, dtype=np.int64), np.asarray(pair_c, dtype=np.int64)
    n = pair_q.size
    logit = np.full(n, np.nan, dtype=np.float32)
    above, total = np.full(n, -1, dtype=np.int64), np.full(n, -1, dtype=np.int64)
    ids = np.arange(n_cand)
    for e in range(n):
        q, c = int(pair_q[e]), int(pair_c[e])
        if not (0 <= q < n_query and 0 <= c < n_cand):
            continue
        row, t = L[q], L[q, c]
        valid = ids != c
        if known is not None:
            valid &= ~np.asarray(known[q], dtype=bool)
        with np.errstate(invalid="ignore"):
            if np.isnan(t):
                before = ~np.isnan(row) | (ids < c)          # every number, and the NaN candidates with a smaller id
            else:
                before = (row > t) | ((row == t) & (ids < c))  # == holds for -0 and +0; NaN compares false
        logit[e], above[e], total[e] = t, int((valid & before).sum()), int(valid.sum())
    return logit, above, total


def given_plan(n_query, n_cand, n_pairs):
    """``(n_groups, n_seg, seg, workspace_bytes)`` of a rank_list call (csrc/dgmi_pair_stream.h segment_plan): the
    listed pairs go in groups of 32, the candidate axis is cut into ``n_seg`` segments of ``seg`` candidates (the last
    one shorter) so that there are about 16 tasks per workgroup, and a pair's result is the sum over its segments.  A
    workgroup streams a segment in chunks of 128 candidates; of a chunk of n its four waves take ``2 * ceil(n / 8)``
    each (the last ones fewer).  The workspace is the known-pair bitmap."""
    n_groups = (n_pairs + 31) // 32
    s = min((16 * 256 + n_groups - 1) // n_groups, 256, (n_cand + 31) // 32)
    s = max(s, 1)
    seg = (n_cand + s - 1) // s
    n_seg = (n_cand + seg - 1) // seg
    total = (n_cand * ((n_query + 31) // 32) * 4 + 255) // 256 * 256
    return n_groups, n_seg, seg, total
