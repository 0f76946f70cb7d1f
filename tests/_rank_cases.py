"""Designed decoders for the two ranking kernels (ops.pair_mlp_topk, ops.pair_mlp_row_topk) and the documented order
restated on the host.  Plain module (like _cases.py), shared by test_rank_cases_host.py and test_gpu_rank_exact.py.

A designed decoder makes ``logit(i, j)`` an exactly representable function of two vectors ``a`` (per drug) and ``c``
(per disease), so the expected answer is integer arithmetic plus a ``lexsort`` and the kernels are held to equality:
the same ids, in the same order, with the same logit bits.  Condition on every design: ``a[i] + c[j]`` and
``a[i] + c[j] + b3`` are exact in fp32 (integers below 2**24; the ``*_table`` functions assert it), and for ``uniform``
``|a[i] + c[j]| < 2**16``: its 64 equal hidden units are summed with weight 2**-6, and a partial sum ``m * r / 64``,
m <= 64, must stay within fp32's 24 bits in any summation order.

Signed zero is left out by name: the kernels map -0.0 to the key of +0.0 and return +0.0, a design cannot produce both
signs reliably, so zero logits compare by value and no case rests on the sign."""
from collections import namedtuple

import numpy as np
import torch

H1, H2 = 128, 64

Pairs = namedtuple("Pairs", "drug dis logit")        # (n,) int64, (n,) int64, (n,) float32; n = min(k, #novel pairs)
Rows = namedtuple("Rows", "cand logit count")        # (n_q, k) int64 (-1 pad), (n_q, k) float32 (NaN pad), (n_q,) int32


# ---------------------------------------------------------------------------------------------
# designs: (P, Q, W2, b2, w3, b3) as float32 CPU tensors
# ---------------------------------------------------------------------------------------------
def _pack(P, Q, W2, b2, w3, b3):
    return tuple(torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32)) for x in (P, Q, W2, b2, w3, [b3]))


def additive(a, c, k0=0, k1=127, h0=0, h1=63, b3=0.0):
    """``logit(i, j) = a[i] + c[j] + b3``: input column k0 carries the sum, k1 its negation, hidden unit h0 reads k0
    and h1 reads k1, ``w3[h0] = 1``, ``w3[h1] = -1``: ``relu(s) - relu(-s) = s``.  Everything else is zero."""
    a, c = np.asarray(a, dtype=np.float64), np.asarray(c, dtype=np.float64)
    assert k0 != k1 and h0 != h1
    P, Q = np.zeros((a.size, H1)), np.zeros((c.size, H1))
    P[:, k0], P[:, k1], Q[:, k0], Q[:, k1] = a, -a, c, -c
    W2, w3 = np.zeros((H2, H1)), np.zeros(H2)
    W2[h0, k0] = W2[h1, k1] = 1.0
    w3[h0], w3[h1] = 1.0, -1.0
    return _pack(P, Q, W2, np.zeros(H2), w3, b3)


def _exact32(t64):
    """The float64 table as float32, which must hold it exactly (the condition on every design)."""
    t32 = t64.astype(np.float32)
    assert np.array_equal(t32.astype(np.float64), t64, equal_nan=True), "the design leaves fp32's exact range"
    return t32


def additive_table(a, c, b3=0.0):
    return _exact32(np.asarray(a, dtype=np.float64)[:, None] + np.asarray(c, dtype=np.float64)[None, :] + b3)


def uniform(a, c, sign, k0=0, b3=0.0):
    """``logit(i, j) = sign * relu(a[i] + c[j]) + b3``: every hidden unit reads column k0 with weight 1 and
    ``w3 = sign * 2**-6``.  No product 0 * inf anywhere, so an infinite ``a`` / ``c`` gives ``sign * inf`` and a NaN
    gives NaN."""
    a, c = np.asarray(a, dtype=np.float64), np.asarray(c, dtype=np.float64)
    assert sign in (1, -1)
    P, Q = np.zeros((a.size, H1)), np.zeros((c.size, H1))
    P[:, k0], Q[:, k0] = a, c
    W2 = np.zeros((H2, H1))
    W2[:, k0] = 1.0
    return _pack(P, Q, W2, np.zeros(H2), np.full(H2, sign * 2.0 ** -6), b3)


def uniform_table(a, c, sign, b3=0.0):
    s = np.asarray(a, dtype=np.float64)[:, None] + np.asarray(c, dtype=np.float64)[None, :]
    with np.errstate(invalid="ignore"):
        r = np.where(s < 0, 0.0, s)  # keeps NaN, as torch.relu does
    assert not (np.abs(r[np.isfinite(r)]) >= 2.0 ** 16).any()
    return _exact32(sign * r + b3)


def dead(n_drug, n_dis, b3, seed=0):
    """Every hidden unit dead (``W2 = 0``, ``b2 = -1``): every logit is exactly ``b3`` whatever P and Q hold."""
    rng = np.random.default_rng(seed)
    P, Q = rng.integers(-9, 10, (n_drug, H1)), rng.integers(-9, 10, (n_dis, H1))
    return _pack(P, Q, np.zeros((H2, H1)), np.full(H2, -1.0), np.ones(H2), b3)


def dead_table(n_drug, n_dis, b3):
    return np.full((n_drug, n_dis), b3, dtype=np.float32)


def torch_logits(P, Q, W2, b2, w3, b3, dtype, rows=32):
    """The decoder formula in plain torch at ``dtype``, chunked over drugs: (n_drug, n_dis)."""
    P, Q, W2, b2, w3, b3 = (t.to(dtype) for t in (P, Q, W2, b2, w3, b3))
    out = torch.empty(P.shape[0], Q.shape[0], dtype=dtype, device=P.device)
    for lo in range(0, P.shape[0], rows):
        h1 = torch.relu(P[lo:lo + rows, None, :] + Q[None])
        out[lo:lo + rows] = torch.relu(h1 @ W2.t() + b2) @ w3 + b3
    return out


def designed_decoder(W2, b2, w3, b3):
    """An ``MLPDecoder`` whose ``lin1`` is ``[I | I]`` with zero bias (so P = drug_feat, Q = dis_feat for finite
    features) and whose ``lin2`` / ``lin3`` are the design."""
    from dream_gnn_amd import model as M

    dec = M.MLPDecoder(H1).eval()
    with torch.no_grad():
        dec.lin1.weight.copy_(torch.cat([torch.eye(H1), torch.eye(H1)], 1))
        dec.lin1.bias.zero_()
        dec.lin2.weight.copy_(W2)
        dec.lin2.bias.copy_(b2)
        dec.lin3.weight.copy_(w3.view(1, H2))
        dec.lin3.bias.copy_(b3)
    return dec


# ---------------------------------------------------------------------------------------------
# the documented order on the host
# ---------------------------------------------------------------------------------------------
def _prepare(L, known):
    L = np.ascontiguousarray(L, dtype=np.float32)
    valid = np.ones(L.shape, dtype=bool) if known is None else ~np.ascontiguousarray(known, dtype=bool)
    return L, valid


def expected_pairs(L, known, k):
    """The ``min(k, #novel)`` novel pairs of the (n_drug, n_dis) table ``L`` in the documented order: logit
    descending, ties by (drug, disease) ascending, NaN after every number.  ``known``: bool mask or None.

    Only a superset of the answer is sorted: the novel pairs above the k-th largest novel number t, as many pairs equal
    to t (in id order) as are still missing, and every novel NaN.  The cut changes nothing but the time."""
    L, valid = _prepare(L, known)
    kk = min(k, int(valid.sum()))
    if kk == 0:
        return Pairs(np.empty(0, np.int64), np.empty(0, np.int64), np.empty(0, np.float32))
    isnan = np.isnan(L)
    num = np.where(valid & ~isnan, L, -np.inf).ravel()
    t = np.partition(num, num.size - kk)[num.size - kk]
    with np.errstate(invalid="ignore"):
        above, equal = valid & (L > t), valid & (L == t)
    first_equal = equal & (np.cumsum(equal.ravel()).reshape(L.shape) <= kk - int(above.sum()))
    drug, dis = np.nonzero(above | first_equal | (valid & isnan))
    l = L[drug, dis]
    nan = np.isnan(l)
    order = np.lexsort((dis, drug, -np.where(nan, 0.0, l).astype(np.float64), nan))[:kk]
    return Pairs(drug[order].astype(np.int64), dis[order].astype(np.int64), l[order])


def expected_rows(L, known, k):
    """Per row q of the (n_query, n_cand) table ``L``: its ``min(k, #novel)`` novel candidates, logit descending, ties
    by candidate ascending, NaN after every number; ``-1`` / NaN past the count.  ``known``: bool mask or None.
    Per-disease lists take ``L.T`` and ``known.T`` of the (n_drug, n_dis) table.  The same superset per row as in
    :func:`expected_pairs`."""
    L, valid = _prepare(L, known)
    n_q, n_c = L.shape
    count = np.minimum(valid.sum(1), k).astype(np.int32)
    cand = np.full((n_q, k), -1, dtype=np.int64)
    logit = np.full((n_q, k), np.nan, dtype=np.float32)
    if n_c == 0 or n_q == 0:
        return Rows(cand, logit, count)
    isnan = np.isnan(L)
    num = np.where(valid & ~isnan, L, -np.inf)
    kth = n_c - np.clip(count, 1, n_c)                   # index of the row's count-th largest in ascending order
    t = np.partition(num, np.unique(kth), axis=1)[np.arange(n_q), kth][:, None]
    with np.errstate(invalid="ignore"):
        above, equal = valid & (L > t), valid & (L == t)
    first_equal = equal & (np.cumsum(equal, axis=1) <= (count - above.sum(1))[:, None])
    row, col = np.nonzero(above | first_equal | (valid & isnan))
    l = L[row, col]
    nan = np.isnan(l)
    order = np.lexsort((col, -np.where(nan, 0.0, l).astype(np.float64), nan, row))
    row, col, l = row[order], col[order], l[order]
    start = np.searchsorted(row, np.arange(n_q))
    rank = np.arange(row.size) - start[row]
    keep = rank < count[row]
    cand[row[keep], rank[keep]] = col[keep]
    logit[row[keep], rank[keep]] = l[keep]
    return Rows(cand, logit, count)


def cut_pairs(e, k):
    """The answer for a smaller k: a prefix (the order is total)."""
    return Pairs(e.drug[:k], e.dis[:k], e.logit[:k])


def cut_rows(e, k):
    return Rows(e.cand[:, :k], e.logit[:, :k], np.minimum(e.count, k).astype(np.int32))


# ---------------------------------------------------------------------------------------------
# equality
# ---------------------------------------------------------------------------------------------
def assert_same_logits(got, exp, what=""):
    """NaN where NaN is expected, equal values elsewhere, equal bit patterns where the value is not zero."""
    got, exp = np.asarray(got, dtype=np.float32), np.asarray(exp, dtype=np.float32)
    assert got.shape == exp.shape, (what, got.shape, exp.shape)
    nan = np.isnan(exp)
    assert np.array_equal(np.isnan(got), nan), "%s: NaN positions differ" % what
    assert np.array_equal(got[~nan], exp[~nan]), "%s: logit values differ" % what
    nz = ~nan & (exp != 0)
    assert np.array_equal(got[nz].view(np.uint32), exp[nz].view(np.uint32)), "%s: logit bits differ" % what


def _np(t):
    return t.detach().cpu().numpy() if isinstance(t, torch.Tensor) else np.asarray(t)


def assert_pairs_equal(got, exp, what=""):
    drug, dis, logit = (_np(t) for t in got)
    assert drug.shape == exp.drug.shape, "%s: %d pairs returned, %d expected" % (what, drug.size, exp.drug.size)
    if not (np.array_equal(drug, exp.drug) and np.array_equal(dis, exp.dis)):
        at = int(np.argmax((drug != exp.drug) | (dis != exp.dis)))
        raise AssertionError("%s: rank %d is pair (%d, %d), expected (%d, %d)"
                             % (what, at, drug[at], dis[at], exp.drug[at], exp.dis[at]))
    assert_same_logits(logit, exp.logit, what)


def assert_rows_equal(got, exp, what=""):
    cand, logit, count = (_np(t) for t in got)
    assert cand.shape == exp.cand.shape and logit.shape == exp.logit.shape, (what, cand.shape, exp.cand.shape)
    assert np.array_equal(count, exp.count), "%s: counts differ" % what
    if not np.array_equal(cand, exp.cand):
        q, r = (int(v[0]) for v in np.nonzero(cand != exp.cand))
        raise AssertionError("%s: row %d rank %d is candidate %d, expected %d" % (what, q, r, cand[q, r], exp.cand[q, r]))
    assert_same_logits(logit, exp.logit, what)  # NaN padding included


# ---------------------------------------------------------------------------------------------
# the per-row planner restated (csrc/dgmi_pairs_rows.hip make_row_plan): how many merge rounds a call takes
# ---------------------------------------------------------------------------------------------
def row_plan(n_query, n_cand, k):
    """``(n_seg, fan, workspace_bytes)`` of a per-row call: a row's ``n_seg`` segment lists are merged ``fan`` at a
    time, in two rounds (and with a second list buffer in the workspace) when ``n_seg > fan``."""
    def up(x):
        return (x + 255) // 256 * 256

    def parts(n_lists):
        return up(n_lists * k * 8) + up(n_lists * 4)

    n_groups = (n_query + 31) // 32
    s = min((16 * 256 + n_groups - 1) // n_groups, 256, (n_cand + 31) // 32)
    s = max(s, 1)
    seg = (n_cand + s - 1) // s
    n_seg = (n_cand + seg - 1) // seg
    kp = 1
    while kp < k:
        kp <<= 1
    fan = min(4096 // kp, 64)
    total = up(n_cand * ((n_query + 31) // 32) * 4) + parts(n_query * n_seg)
    if n_seg > fan:
        total += parts(n_query * ((n_seg + fan - 1) // fan))
    return n_seg, fan, total
