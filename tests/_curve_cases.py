"""Designed samples for the curve-area kernels (ops.curve_areas) and the definition of include/dgmi_curve.h restated on
the host in integers.  Plain module (like _rank_cases.py), shared by test_curve_cases_host.py and test_gpu_curve.py.

The reference works on the ranking key of a score (-0 and +0 one value, every NaN one group below all numbers): counts
and U2 are numpy int64, exact; the float64 sum behind aupr is taken over the groups in descending order with
``math.fsum`` (correctly rounded), so the reference's own error is the rounding of its terms.  Every design is a
function of ``n`` alone (seeded), and says where its tie groups and segments lie in the sorted sequence."""
import math
from collections import namedtuple

import numpy as np

Stats = namedtuple("Stats", "count auroc aupr info")  # (S, 6) int64 rows (P, N, TPt, FPt, G, U2); (S,) float64 x 2; int

SORT_TILE = 8192  # records per workgroup of the radix sort


def bound(n):
    """Allowed |aupr - reference|: two float64 sums of at most n non-negative terms that total at most 1, plus a few
    divisions."""
    return 4 * max(int(n), 1) * 2.0 ** -53


def order_key(score):
    """uint32 ranking key of fp32 scores: larger score -> larger key, NaN -> 0, -0 == +0."""
    s = np.ascontiguousarray(score, dtype=np.float32)
    u = s.view(np.uint32).copy()
    u[u == 0x80000000] = 0
    key = np.where(u & 0x80000000, ~u, u | np.uint32(0x80000000)).astype(np.uint32)
    key[np.isnan(s)] = 0
    return key


def _one_segment(key, pos, reach):
    """(P, N, TPt, FPt, G, U2), auroc, aupr of one segment's samples."""
    if key.size == 0:
        return (0, 0, 0, 0, 0, 0), math.nan, math.nan
    uniq, inv = np.unique(key, return_inverse=True)
    G = uniq.size
    inv = (G - 1) - inv.reshape(-1)  # group 0 = the largest key
    p = np.bincount(inv, weights=pos, minlength=G).astype(np.int64)
    m = np.bincount(inv, minlength=G).astype(np.int64) - p
    TP, FP = np.cumsum(p), np.cumsum(m)
    TP0 = TP - p
    P, N = int(TP[-1]), int(FP[-1])
    U2 = int(np.sum(m * (2 * TP0 + p)))
    auroc = np.float64(U2) / np.float64(2 * P * N) if P * N else math.nan
    if P:
        pi = TP / (TP + FP).astype(np.float64)
        pi0 = np.r_[1.0, pi[:-1]]
        aupr = math.fsum(p * (pi + pi0)) / (2.0 * P)
    else:
        aupr = math.nan
    return (P, N, int(np.sum(pos & reach)), int(np.sum(~pos & reach)), G, U2), float(auroc), aupr


def reference(score, label, segment=None, n_segments=0, threshold=0.0):
    """The definition, per segment: Stats with S = max(n_segments, 1) rows."""
    score = np.asarray(score, dtype=np.float32).reshape(-1)
    label = np.asarray(label, dtype=np.float32).reshape(-1)
    key, pos = order_key(score), label != 0
    with np.errstate(invalid="ignore"):
        reach = score >= np.float32(threshold)  # fp32 compare; False for a NaN on either side
    info = int(np.isnan(score).any()) | int(((label != 0) & (label != 1)).any()) << 1
    S = max(int(n_segments), 1)
    count, auroc, aupr = np.zeros((S, 6), np.int64), np.full(S, np.nan), np.full(S, np.nan)
    if segment is None:
        members = [np.arange(score.size)]
    else:
        seg = np.asarray(segment).astype(np.int64).reshape(-1)
        ok = (seg >= 0) & (seg < S)
        info |= int((~ok).any()) << 2
        order = np.argsort(np.where(ok, seg, S), kind="stable")
        cuts = np.searchsorted(np.where(ok, seg, S)[order], np.arange(S + 1))
        members = [order[cuts[s]:cuts[s + 1]] for s in range(S)]
    for s, idx in enumerate(members):
        if idx.size:
            count[s], auroc[s], aupr[s] = _one_segment(key[idx], pos[idx], reach[idx])
    return Stats(count, auroc, aupr, info)


def group_lengths(score):
    """Lengths of the tie groups in descending score order (what a design claims about itself)."""
    key = np.sort(order_key(score))[::-1]
    ends = np.flatnonzero(np.r_[key[1:] != key[:-1], True])
    return np.diff(np.r_[-1, ends])


# ---------------------------------------------------------------------------------------------
# score / label designs: f(n) -> (score fp32, label fp32), samples in random order
# ---------------------------------------------------------------------------------------------
def _rng(n, salt):
    return np.random.default_rng(1000003 * salt + n)


def _labels(rng, n, frac=0.4):
    return (rng.random(n) < frac).astype(np.float32)


def _shuffled(rng, score, label):
    order = rng.permutation(score.size)
    return np.ascontiguousarray(score[order], np.float32), np.ascontiguousarray(label[order], np.float32)


def _levels_desc(n):
    """n distinct fp32 values, descending (exact quarter steps around 0)."""
    return ((n // 2 - np.arange(n)) * 0.25).astype(np.float32)


def distinct(n):
    rng = _rng(n, 1)
    return _shuffled(rng, _levels_desc(n), _labels(rng, n))


def all_tied(n):
    rng = _rng(n, 2)
    label = _labels(rng, n)
    if n >= 2:
        label[:2] = (1, 0)  # both classes
    return np.full(n, 0.375, np.float32), label


def separated(n):
    """Every positive above every negative (n >= 2: both classes)."""
    rng = _rng(n, 3)
    label = _labels(rng, n)
    if n >= 2:
        label[:2] = (1, 0)
    label = np.sort(label)[::-1]  # positives first = the larger scores
    return _shuffled(rng, _levels_desc(n), label)


def reversed_(n):
    score, label = separated(n)
    return score, 1 - label


def few_levels(levels):
    def design(n):
        rng = _rng(n, 10 + levels)
        return (rng.integers(0, levels, n) - levels // 2).astype(np.float32) * 0.5, _labels(rng, n)
    design.__name__ = "levels_%d" % levels
    return design


def tie_across_sort_tile(n):
    """Distinct scores but for ONE tie group of 8197 samples at sorted positions 8190 .. 16386 (n >= 16387)."""
    rng = _rng(n, 4)
    score = _levels_desc(n)
    score[8190:8190 + 8197] = score[8190]
    return _shuffled(rng, score, _labels(rng, n))


def ties_across_every_64(n):
    """Tie groups [0, 32), [32, 96), [96, 160), ...: every multiple of 64 lies strictly inside a group."""
    rng = _rng(n, 5)
    group = (np.arange(n) + 32) // 64
    return _shuffled(rng, (-group).astype(np.float32), _labels(rng, n))


def signed_zeros(n):
    rng = _rng(n, 6)
    return rng.choice(np.array([-0.0, 0.0, -1.0, 1.0], np.float32), n), _labels(rng, n)


def infinities(n):
    rng = _rng(n, 7)
    return rng.choice(np.array([-np.inf, np.inf, -2.0, 0.5, 3.0], np.float32), n), _labels(rng, n)


def denormals(n):
    rng = _rng(n, 8)
    k = rng.integers(-5, 6, n)
    score = (np.abs(k).astype(np.uint32) | np.where(k < 0, np.uint32(0x80000000), np.uint32(0))).astype(np.uint32)
    return score.view(np.float32), _labels(rng, n)  # +-k 2**-149, k = 0..5: eleven values, all below the smallest normal


def only_positives(n):
    score, _ = few_levels(7)(n)
    return score, np.ones(n, np.float32)


def only_negatives(n):
    score, _ = few_levels(7)(n)
    return score, np.zeros(n, np.float32)


SIZES = [1, 2, 63, 64, 65, 8191, 8192, 8193, 24593, 100003]
DESIGNS = [distinct, all_tied, separated, reversed_, few_levels(2), few_levels(7), tie_across_sort_tile, ties_across_every_64,
           signed_zeros, infinities, denormals, only_positives, only_negatives]


def applies(design, n):
    return n >= 16387 if design is tie_across_sort_tile else True


# ---------------------------------------------------------------------------------------------
# segment designs: f(n) -> (segment int32 in sample order, n_segments, sizes by id); the sorted sequence holds the
# segments in id order, so the sizes say where the boundaries lie
# ---------------------------------------------------------------------------------------------
def _assign(rng, sizes):
    n = int(np.sum(sizes))
    seg = np.repeat(np.arange(len(sizes)), sizes).astype(np.int32)
    return seg[rng.permutation(n)], len(sizes), np.asarray(sizes, np.int64)


def boundary_segments(n):
    """Boundaries exactly on and one off the sorted positions 64, 8192 and 16384 (those below n), with empty first,
    middle and last segments, one-sample segments and one segment over three sort tiles when n allows."""
    rng = _rng(n, 20)
    cuts = [c for c in (63, 64, 65, 8191, 8192, 8193, 16383, 16384, 16385) if c < n]
    sizes = np.diff(np.r_[0, cuts, n]).tolist()
    sizes = [0] + sizes[:2] + [0] + sizes[2:] + [0]  # ids 0, 3 and the last are empty
    return _assign(rng, sizes)


def single_sample_segments(n):
    """Every sample its own segment (each has one class only: both areas NaN or auroc NaN)."""
    return _assign(_rng(n, 21), [1] * n)


def random_segments(n):
    rng = _rng(n, 22)
    S = 37
    seg = rng.integers(0, S, n).astype(np.int32)
    return seg, S, np.bincount(seg, minlength=S).astype(np.int64)


def out_of_range_segments(n):
    """random_segments with every seventh id outside [0, S): -1, S, a large one."""
    seg, S, _ = random_segments(n)
    seg = seg.copy()
    bad = np.arange(0, n, 7)
    seg[bad] = np.array([-1, S, 2 ** 31 - 1], np.int32)[np.arange(bad.size) % 3]
    ok = (seg >= 0) & (seg < S)
    return seg, S, np.bincount(seg[ok], minlength=S).astype(np.int64)


SEGMENT_DESIGNS = [boundary_segments, single_sample_segments, random_segments, out_of_range_segments]
SEGMENT_SIZES = [1, 65, 8193, 24593, 100003]


def segment_applies(design, n):
    return n <= 8193 if design is single_sample_segments else True


def one_class_segment(label, segment, which):
    """`label` with every sample of segment `which` made positive."""
    label = label.copy()
    label[segment == which] = 1
    return label
