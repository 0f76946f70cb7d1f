"""Designed rows for the bf16-screened cosine kNN (csrc/dgmi_knn_screen.hip), and the screen's arithmetic restated on the
host.  Plain module (like _rank_cases.py), shared by test_knn_cases_host.py, test_gpu_spmm.py and tools/knn_soak.py.

The screen multiplies bf16 copies of unit rows (round to nearest even: unit roundoff 2**-8 per element) and keeps every
candidate within ``2 * eps`` of a lower bound of the query's k-th best approximate score; the answer is exact only if
``|approx - exact| <= eps`` for EVERY pair.  On random rows the roundings cancel to ~1e-4, so random data cannot tell a
sound eps from one several times too small.  These rows make every rounding pull the same way:

  q   columns [0, h)   p (1 + 2**-8)(1 - eta): just below a bf16 midpoint, rounds DOWN to p
      columns [h, 2h)  p (1 + 2**-8)(1 + eta): just above it, rounds UP to p (1 + 2**-7)
  A   columns [0, h)   p (1 + 53/128 + 2**-8)(1 - eta): rounds down         -> approx(q, A) is too SMALL by ~0.0047
  B_j columns [h, 2h)  p (1 + 53/128 + 2**-8)(1 + eta): rounds up           -> approx(q, B_j) is too LARGE by ~0.0047
      of which ``nlow`` sit one bf16 step lower, p (1 + 52/128 + 2**-8)(1 + eta), so that exact(q, A) > exact(q, B_j)

and every row carries a filler, in columns where q is zero (q's own: where every other row is zero), that makes its fp32
norm 1.  A is q's true nearest neighbour; a screen whose eps is below the attained error never lets A reach the exact
rescoring once k decoys B_j have set the threshold.

eta = 2**-18 survives the rounding of the designed values to fp32 (half an ulp is 2**-24 relative) and is far below what
the scores resolve."""
import math
from collections import namedtuple

import numpy as np
import torch

ETA = 2.0 ** -18
U_BF16 = 2.0 ** -8                       # unit roundoff of bf16 under round to nearest: 8 significant bits
EPS_TRUE = 2.0 ** -7 + 2.0 ** -16        # (1 + u)**2 - 1: |approx - exact| <= EPS_TRUE |q| |c|, products summed exactly
EPS_OLD = 0.0042                         # the margin the screen shipped with (2**-8 + 2**-18 + slack): too small

Design = namedtuple("Design", "D k p h nlow q A B")   # q, A: (D,) float32; B: (k, D) float32


def shape_of(D):
    """(p, h) for width D: p = 2**-e and h columns per half, h <= (D - 4) / 2 (four columns stay free for fillers), with
    the largest h p**2 <= 0.4961 (q's designed part has squared norm 2 h p**2 (1 + 2**-8)**2 < 1): the highest score."""
    best = None
    for e in range(1, 12):
        p = 2.0 ** -e
        h = min((D - 4) // 2, int(0.4961 / (p * p)))
        if h >= 1 and (best is None or h * p * p >= best[1] * best[0] ** 2):  # (a tie: the wider design)
            best = (p, h)
    assert best is not None, "D too small for the design"
    return best


# Decoy elements one bf16 step lower: each takes p**2 (1 + 2**-8) / 128 off the decoy's exact score and as much off its
# approximate one.  With none, exact(B) is 1e-5 ABOVE exact(A) (the two eta terms).  p <= 2**-4 (D >= 256): 10, an exact
# gap of 3.0e-4 (D = 1024: 6.6e-5).  p = 2**-3 (D <= 128), where one step is worth 1.2e-4: 2, an exact gap of 2.3e-4 — with
# 10 the decoys' approximate scores would fall far enough for A to pass the old margin.
def default_nlow(D):
    return 10 if shape_of(D)[0] < 2.0 ** -3 else 2


def _with_filler(main64, cols, weights):
    """float32 row: the designed part (rounded to fp32 first) plus a filler spread over `cols` in proportion to
    `weights` (a unit vector) that brings the norm OF THE FP32 ROW to 1."""
    row = main64.astype(np.float32)
    rest = 1.0 - float(np.sum(row.astype(np.float64) ** 2))
    assert rest > 0.0, "no room for a filler"
    assert np.all(row[list(cols)] == 0)
    row[list(cols)] = (math.sqrt(rest) * np.asarray(weights, dtype=np.float64)).astype(np.float32)
    return row


def build(D, k, nlow=None):
    """q, A and k decoys for width D.  The decoys differ only in their fillers — distinct columns where D leaves room,
    otherwise distinct directions in the last two columns — so they are k distinct rows with the SAME exact and the same
    approximate similarity to q (q is zero in every filler column but its own)."""
    p, h = shape_of(D)
    nlow = default_nlow(D) if nlow is None else nlow
    assert 0 <= nlow <= h and k >= 1
    lo, hi = 1.0 - ETA, 1.0 + ETA
    q = np.zeros(D)
    q[:h] = p * (1 + U_BF16) * lo
    q[h:2 * h] = p * (1 + U_BF16) * hi
    a = np.zeros(D)
    a[:h] = p * (1 + 53 / 128 + U_BF16) * lo
    b = np.zeros(D)
    b[h:2 * h] = p * (1 + 53 / 128 + U_BF16) * hi
    b[h:h + nlow] = p * (1 + 52 / 128 + U_BF16) * hi
    free = D - 2 * h - 2                 # columns after q's and A's fillers
    assert free >= 2
    rows_b = []
    for j in range(k):
        if free >= k:
            rows_b.append(_with_filler(b, [2 * h + 2 + j], [1.0]))
        else:
            th = 0.5 * math.pi * (j + 1) / (k + 1)
            rows_b.append(_with_filler(b, [D - 2, D - 1], [math.cos(th), math.sin(th)]))
    t = torch.from_numpy
    return Design(D, k, p, h, nlow, t(_with_filler(q, [2 * h], [1.0])), t(_with_filler(a, [2 * h + 1], [1.0])),
                  t(np.stack(rows_b)))


def bf16_round(x):
    """fp32 -> bf16 (round to nearest even, what knn_to_bf16_kernel does) -> float64."""
    return x.to(torch.float32).to(torch.bfloat16).to(torch.float64)


def exact_scores(q, C):
    """<q, c> of fp32 rows in float64."""
    return C.to(torch.float64) @ q.to(torch.float64)


def approx_scores(q, C):
    """What the screen computes, up to fp32 accumulation order: bf16 x bf16 products summed in float64."""
    return bf16_round(C) @ bf16_round(q)


def embed(base, design, q_at, a_at, b_at=0):
    """A copy of the unit rows `base` (N, D) with the design written over rows q_at, a_at and b_at .. b_at + k - 1."""
    x = base.clone()
    k = design.B.shape[0]
    assert len({q_at, a_at} | set(range(b_at, b_at + k))) == k + 2
    x[q_at], x[a_at], x[b_at:b_at + k] = design.q, design.A, design.B
    return x
