"""Harness counterpart of the reference's ``model.py`` (row H of the scope table).

The reference's ``Net`` (model.py:4-103), its attention fusion (layers.py:324-338) and MLP
decoder (layers.py:341-379) are *callers* of the hot path and stay untouched upstream.  They
are restated here only so that ``smoke()``, ``bench.py`` and the parity tests can drive the
HIP path through the same forward structure on a box that has neither DGL nor the reference:
same ``state_dict`` keys (a reference checkpoint loads with ``strict=True``), same layer
order, same residual accumulation ``out += layer_out / (i + 1)`` (model.py:69-74).
"""
from __future__ import annotations

import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

from . import ops
from .layers import FGCN, GCMCLayer, get_activation


class Attention(nn.Module):
    """Two-way softmax attention over stacked embeddings — layers.py:324-338."""

    #: Opt-in: the whole chain as ONE HIP kernel forward and a recompute backward (``ops.attention_fuse``, DESIGN.md
    #: 4.16) when the operands are fusable: fp32 HIP tensors, exactly two channels, a width that is a multiple of 4 in
    #: [4, 512], rows with unit inner stride on 16-byte boundaries, and the ``project`` the constructor made.  Anything
    #: else takes the torch chain.  With the flag on, the returned ``beta`` carries NO gradient (the kernels return the
    #: weights after dropout as a constant); ``out`` is differentiable in the inputs and the three parameters.
    fused = False

    def __init__(self, in_size, hidden_size=16, dropout_rate=0.1, fused=False):
        super().__init__()
        if fused:
            self.fused = True
        self.project = nn.Sequential(nn.Linear(in_size, hidden_size), nn.Tanh(),
                                     nn.Linear(hidden_size, 1, bias=False))
        self.dropout = nn.Dropout(dropout_rate)

    def forward(self, z):
        if self.fused and z.dim() == 3 and z.shape[1] == 2 and self._fusable(z[:, 0], z[:, 1]):
            return self._fused(z, None)
        return self._chain(z)

    def _chain(self, z):
        beta = self.dropout(torch.softmax(self.project(z), dim=1))
        return (beta * z).sum(1), beta

    def fuse(self, a, b):
        """``self.forward(torch.stack([a, b], 1))``; with ``fused`` set and fusable operands the two tables go to the
        kernel as they are, so the stack is never made.  Returns ``(out, beta)``, ``beta`` of shape ``(n, 2, 1)``; on
        the fused route ``beta`` (the weights after dropout) carries no gradient.  Operands that are not fusable as
        they are (rows off a 16-byte boundary, say) take the torch chain on their stack, not the kernel on a copy."""
        if self.fused and a.dim() == 2 and a.shape == b.shape and self._fusable(a, b):
            return self._fused(a, b)
        z = torch.stack([a, b], dim=1)
        return self._chain(z) if self.fused else self.forward(z)

    def _fusable(self, a, b):
        p = self.project
        if not (isinstance(p, nn.Sequential) and len(p) == 3 and isinstance(p[0], nn.Linear) and isinstance(p[1], nn.Tanh)
                and isinstance(p[2], nn.Linear) and p[0].bias is not None and p[2].bias is None):
            return False
        F_ = a.shape[1]
        if p[0].weight.shape != (16, F_) or p[2].weight.shape != (1, 16) or F_ % 4 != 0 or not 4 <= F_ <= 512:
            return False
        for t in (a, b):
            if not (t.is_cuda and t.dtype == torch.float32 and t.stride(1) == 1 and t.stride(0) % 4 == 0
                    and t.stride(0) >= F_ and t.data_ptr() % 16 == 0):
                return False
        return all(w.is_cuda and w.dtype == torch.float32 for w in (p[0].weight, p[0].bias, p[2].weight))

    def _fused(self, a, b):
        n = a.shape[0]
        mult = None
        if self.training and 0.0 < self.dropout.p:
            # the draw nn.Dropout would make on beta (n, 2, 1): the same mask and the same generator state afterwards
            mult = F.dropout(torch.ones(n, 2, 1, device=a.device), self.dropout.p, True).view(n, 2)
        out, beta = ops.attention_fuse(a, b, self.project[0].weight, self.project[0].bias, self.project[2].weight, mult)
        return out, beta.view(n, 2, 1)


def _split_k_weight_grad(dy, x, chunk: int):
    """``dy^T x`` (out x in) with K = number of rows: chunks of ``chunk`` rows as one batched GEMM, summed, plus the tail."""
    n = x.shape[0] // chunk * chunk
    dw = torch.bmm(dy[:n].view(-1, chunk, dy.shape[1]).transpose(1, 2), x[:n].view(-1, chunk, x.shape[1])).sum(0)
    if n < x.shape[0]:
        dw = dw + dy[n:].t() @ x[n:]
    return dw


class _EdgeLinear(torch.autograd.Function):
    """``F.linear`` over the decoder's edge list (E rows, a few hundred thousand on the real datasets), with the
    weight gradient ``dY^T X`` (out x in, K = E) evaluated split-K: the library's single GEMM for an (64 x 128 x 467 k)
    product runs one 32 x 64 tile per workgroup down the whole K (0.95 ms at the lrssl shape — the largest kernel of a
    training step); chunks of ``CHUNK`` edges as one batched GEMM plus a sum over the chunks take ~0.1 ms.  Same
    values up to fp32 summation order; forward and input gradient are the library's."""

    CHUNK = 2048
    MIN_ROWS = 32768  # below this the plain GEMM is launch-bound anyway

    @staticmethod
    def forward(ctx, x, weight, bias):
        ctx.save_for_backward(x, weight)
        ctx.has_bias = bias is not None
        return F.linear(x, weight, bias)

    @staticmethod
    def backward(ctx, dy):
        x, weight = ctx.saved_tensors
        dy = dy.contiguous()
        dx = None
        if ctx.needs_input_grad[0]:
            # 1-wide layer: the input gradient is an outer product — a broadcast multiply (25 us), not a K = 1 GEMM (79 us)
            dx = dy * weight if weight.shape[0] == 1 else dy @ weight
        dw = db = None
        if ctx.needs_input_grad[1] and weight.shape[0] == 1:
            # lin3 (64 -> 1): dy^T x is a weighted column sum; as a batched GEMM its 1-wide tiles took 200 us
            dw = (x * dy).sum(0, keepdim=True)
        elif ctx.needs_input_grad[1]:
            dw = _split_k_weight_grad(dy, x, _EdgeLinear.CHUNK)
        if ctx.has_bias and ctx.needs_input_grad[2]:
            db = dy.sum(0)
        return dx, dw, db


class _ReluDropout(torch.autograd.Function):
    """``dropout(relu(x))`` over the decoder's E x 128 / E x 64 activations (layers.py:366-369), forward exactly as torch
    does it (same kernels, same RNG consumption), backward in ONE pass from the output alone: ``y > 0`` exactly where the
    input was positive and the element was kept, so ``dx = dy / (1 - p)`` there and 0 elsewhere
    (``dgmi_epilogue_backward_f32`` act 2) — torch's two backward passes (masked scale, then threshold) read and write
    the E-sized tensors twice: 213 -> 130 us on the 467 k x 128 one."""

    @staticmethod
    def forward(ctx, x, p: float):
        y = F.dropout(F.relu(x), p, True)
        ctx.scale = 1.0 / (1.0 - p)
        ctx.save_for_backward(y)
        return y

    @staticmethod
    def backward(ctx, dy):
        (y,) = ctx.saved_tensors
        return ops.epilogue_backward(dy.contiguous(), y, None, 2, 0.0, ctx.scale), None


def _relu_dropout(drop: nn.Dropout, x):
    if (x.is_cuda and drop.training and 0.0 < drop.p < 1.0 and torch.is_grad_enabled() and x.requires_grad
            and x.dtype == torch.float32 and x.is_contiguous() and x.shape[0] >= _EdgeLinear.MIN_ROWS):
        return _ReluDropout.apply(x, float(drop.p))
    return drop(F.relu(x))


class _EdgeLinearReluDropout(torch.autograd.Function):
    """``dropout(relu(x W^T + b))`` over the edge list (the decoder's ``lin2`` stage, layers.py:368): the relu is the
    GEMM's own epilogue (``torch._addmm_activation``: 204 -> 165 us at 467 k x 128 -> 64), the dropout torch's, the backward
    ONE gating pass from the output, then the library GEMM for the input gradient and the split-K weight gradient of
    :class:`_EdgeLinear`."""

    @staticmethod
    def forward(ctx, x, weight, bias, p: float):
        y = torch._addmm_activation(bias, x, weight.t())  # relu(x W^T + b)
        y = F.dropout(y, p, True)
        ctx.scale = 1.0 / (1.0 - p)
        ctx.save_for_backward(x, weight, y)
        return y

    @staticmethod
    def backward(ctx, dy):
        x, weight, y = ctx.saved_tensors
        dz = ops.epilogue_backward(dy.contiguous(), y, None, 2, 0.0, ctx.scale)
        dx = dz @ weight if ctx.needs_input_grad[0] else None
        dw = db = None
        if ctx.needs_input_grad[1]:
            dw = _split_k_weight_grad(dz, x, _EdgeLinear.CHUNK)
        if ctx.needs_input_grad[2]:
            db = dz.sum(0)
        return dx, dw, db, None


def _fusable(drop: nn.Dropout, x) -> bool:
    return (x.is_cuda and drop.training and 0.0 < drop.p < 1.0 and torch.is_grad_enabled() and x.dtype == torch.float32
            and x.dim() == 2 and x.is_contiguous() and x.shape[0] >= _EdgeLinear.MIN_ROWS)


def _edge_linear_relu_dropout(lin: nn.Linear, drop: nn.Dropout, x):
    if _fusable(drop, x) and lin.bias is not None and lin.weight.shape[0] > 1 and hasattr(torch, "_addmm_activation"):
        return _EdgeLinearReluDropout.apply(x, lin.weight, lin.bias, float(drop.p))
    return _relu_dropout(drop, _edge_linear(lin, x))


def _edge_linear(lin: nn.Linear, x):
    if x.is_cuda and x.dim() == 2 and x.shape[0] >= _EdgeLinear.MIN_ROWS and x.is_contiguous() and torch.is_grad_enabled():
        return _EdgeLinear.apply(x, lin.weight, lin.bias)
    return lin(x)


class MLPDecoder(nn.Module):
    """Per-edge gather-concat then 2F->128->64->1 MLP — layers.py:341-375."""

    def __init__(self, in_units, dropout_rate=0.1, fused_training=False):
        super().__init__()
        if fused_training:
            self.fused_training = True
        self.dropout = nn.Dropout(dropout_rate)
        self.sigmoid = nn.Sigmoid()
        self.lin1 = nn.Linear(2 * in_units, 128)
        self.lin2 = nn.Linear(128, 64)
        self.lin3 = nn.Linear(64, 1)
        self.reset_parameters()

    def reset_parameters(self):
        # layers.py:355-358 re-draws the three Linear inits (keeps the RNG stream aligned)
        for lin in (self.lin1, self.lin2, self.lin3):
            lin.reset_parameters()

    #: lin1(cat(h_src, h_dst)) = h_src W_a^T + h_dst W_b^T + b: project the node tables, then add the
    #: projected rows per edge (``dgmi_gather_add_f32``).  Removes the E x 2F matrix and the
    #: E x 2F x 128 GEMM; same parameters, results equal up to fp32 summation order.  False: the
    #: reference's literal order (gather-concat, then lin1 over edges).
    fuse_lin1 = True

    #: Opt-in: the whole MLP over the pair list as ONE HIP kernel forward and a recompute backward
    #: (``ops.pair_mlp_train``) on the split ``lin1`` tables.  No E x 128 / E x 64 tensor is kept for the backward.  The
    #: dropout masks come from a hash keyed by a device-drawn seed, NOT from torch's RNG stream (one ``randint`` draw per
    #: forward instead of two mask draws), which is why the default stays the torch chain.  fp32 HIP inputs only.
    fused_training = False

    def forward(self, graph, drug_feat, dis_feat):
        pairs = graph.edge_pairs()
        if (self.fused_training and drug_feat.is_cuda and dis_feat.is_cuda and drug_feat.dtype == torch.float32
                and dis_feat.dtype == torch.float32):
            P, Q = self._split_lin1(drug_feat, dis_feat)
            if self.training or torch.is_grad_enabled():
                p = float(self.dropout.p) if self.training else 0.0
                return ops.pair_mlp_train(P, Q, *self._tail(), pairs, p).unsqueeze(-1)
            return ops.pair_mlp_score_list(P, Q, *self._tail(), pairs.src, pairs.dst).unsqueeze(-1)
        if self.fuse_lin1:
            Fd = drug_feat.shape[1]
            w = self.lin1.weight
            a, b = drug_feat @ w[:, :Fd].t(), dis_feat @ w[:, Fd:].t()
            if a.is_cuda and self.dropout.training and 0.0 < self.dropout.p < 1.0 and torch.is_grad_enabled():
                out = ops.gather_add_relu_dropout(pairs, a, b, self.lin1.bias, self.dropout.p)
            else:
                out = self.dropout(F.relu(ops.gather_add(pairs, a, b, self.lin1.bias)))
        else:
            # layers.py:361-365: graph.apply_edges(udf_u_mul_e) -> edata['m'] = cat(h_src, h_dst);
            # one fused HIP gather-concat over the decoder edge list (bit-identical values).
            out = ops.gather_concat(pairs, drug_feat, dis_feat)
            out = _relu_dropout(self.dropout, _edge_linear(self.lin1, out))
        out = _edge_linear_relu_dropout(self.lin2, self.dropout, out)
        return _edge_linear(self.lin3, out)

    def top_pairs(self, drug_feat, dis_feat, k, known=None):
        """The eval-mode decoder over ALL (drug, disease) pairs, reduced to the ``k`` best on the device
        (``ops.pair_mlp_topk``): ``(drug_id, disease_id, logit)`` device tensors, ordered by logit descending, ties by
        ``(drug_id, disease_id)`` ascending, NaN last; pairs in ``known = (drug_ids, disease_ids)`` are left out.
        ``lin1`` is split as in :attr:`fuse_lin1` (two small GEMMs in torch); the rest is one HIP kernel.  Dropout is
        not applied (eval mode).  ``1 <= k <= 1024``."""
        k = int(k)
        if not 1 <= k <= ops.PAIR_TOPK_MAX_K:
            raise ValueError("k must be in 1..%d (the on-chip top-k limit), got %d" % (ops.PAIR_TOPK_MAX_K, k))
        Fd = drug_feat.shape[1]
        w1 = self.lin1.weight
        P = torch.addmm(self.lin1.bias, drug_feat, w1[:, :Fd].t())
        Q = dis_feat @ w1[:, Fd:].t()
        kd, ks = (None, None) if known is None else known
        return ops.pair_mlp_topk(P, Q, self.lin2.weight, self.lin2.bias, self.lin3.weight, self.lin3.bias, kd, ks, k)

    def top_pairs_per_row(self, drug_feat, dis_feat, k, by="disease", known=None, rows=None):
        """The eval-mode decoder over ALL (drug, disease) pairs, reduced to the ``k`` best candidates of every query row
        on the device (``ops.pair_mlp_row_topk``).  ``by="disease"``: the queries are diseases and the candidates drugs
        (which drugs fit disease X); ``by="drug"``: the queries are drugs and the candidates diseases.  Pairs in
        ``known = (drug_ids, disease_ids)`` are left out.  ``rows``: an optional 1-D subset of query ids (unique, in
        range); only those rows are scored.  ``lin1`` is split as in :meth:`top_pairs`, and every logit is bit-identical
        to the one :meth:`top_pairs` computes for the same pair.  ``1 <= k <= 128``.

        Returns ``(query_id, cand_id, logit, count)`` device tensors: int64 ``query_id`` (n_q), int64 ``cand_id`` and
        fp32 ``logit`` (n_q x k, ordered by logit descending, ties by candidate id ascending, NaN last; -1 / NaN past
        the row's count) and int32 ``count`` (n_q)."""
        k = int(k)
        if not 1 <= k <= ops.ROW_TOPK_MAX_K:
            raise ValueError("k must be in 1..%d (the per-row on-chip top-k limit), got %d" % (ops.ROW_TOPK_MAX_K, k))
        if by not in ("disease", "drug"):
            raise ValueError('by must be "disease" or "drug", got %r' % (by,))
        n_query = int(dis_feat.shape[0] if by == "disease" else drug_feat.shape[0])
        sub = query_rows(rows, n_query)
        Fd = drug_feat.shape[1]
        w1 = self.lin1.weight
        P = torch.addmm(self.lin1.bias, drug_feat, w1[:, :Fd].t())
        Q = dis_feat @ w1[:, Fd:].t()
        X, C = (Q, P) if by == "disease" else (P, Q)
        kq = kc = None
        if known is not None:
            kd, ks = known
            kq, kc = (ks, kd) if by == "disease" else (kd, ks)
        if sub is None:
            query_id = torch.arange(n_query, device=X.device)
        else:
            query_id = sub.to(X.device)
            X = X.index_select(0, query_id)
            if kq is not None:
                kq, kc = _remap_known(kq.to(X.device).long(), kc.to(X.device).long(), query_id, n_query, C.shape[0])
        cand, logit, count = ops.pair_mlp_row_topk(X, C, self.lin2.weight, self.lin2.bias, self.lin3.weight,
                                                   self.lin3.bias, kq, kc, k)
        return query_id, cand, logit, count

    def _split_lin1(self, drug_feat, dis_feat):
        """``(P, Q)`` with the torch expressions of :meth:`top_pairs`, so that the kernels see the same bits."""
        Fd = drug_feat.shape[1]
        w1 = self.lin1.weight
        return torch.addmm(self.lin1.bias, drug_feat, w1[:, :Fd].t()), dis_feat @ w1[:, Fd:].t()

    def _tail(self):
        return self.lin2.weight, self.lin2.bias, self.lin3.weight, self.lin3.bias

    def pairs_above(self, drug_feat, dis_feat, min_logit, known=None, max_pairs=1 << 20):
        """EVERY (drug, disease) pair not in ``known = (drug_ids, disease_ids)`` whose eval-mode logit is at or above
        ``min_logit`` (``ops.pair_mlp_above``): ``(drug_id, disease_id, logit)`` device tensors in the order of
        :meth:`top_pairs`, every logit bit-identical to the one :meth:`top_pairs` computes for the pair.  The cut is
        inclusive; ``min_logit = NaN`` lists every novel pair.  Raises ``ops.TooManyPairs`` (with the exact count) when
        more than ``max_pairs`` (1..2**24) pairs qualify."""
        max_pairs = ops._check_max_pairs(max_pairs)
        P, Q = self._split_lin1(drug_feat, dis_feat)
        kd, ks = (None, None) if known is None else known
        return ops.pair_mlp_above(P, Q, *self._tail(), kd, ks, float(min_logit), max_pairs)[:3]

    def count_pairs_above(self, drug_feat, dis_feat, min_logit, known=None):
        """How many pairs :meth:`pairs_above` lists at this cut (``ops.pair_mlp_count_above``): exact, nothing stored."""
        P, Q = self._split_lin1(drug_feat, dis_feat)
        kd, ks = (None, None) if known is None else known
        return ops.pair_mlp_count_above(P, Q, *self._tail(), kd, ks, float(min_logit))

    #: the largest ``k`` of :meth:`top_pairs_deep`
    DEEP_MAX_K = 1 << 20

    def top_pairs_deep(self, drug_feat, dis_feat, k, known=None):
        """:meth:`top_pairs` for ``1 <= k <= 2**20``: the same tuple, order and logit bits.  Up to 1024 it is
        :meth:`top_pairs`; beyond, a cut is estimated from every s-th drug row (``s = ceil(k / 512)``, scored by the
        on-chip top-k without the known list: the sample's entry at rank ``ceil(1.5 k / s) + 32``), one emit pass lists
        every novel pair at or above it into ``4 k + 65536`` slots, and the sorted list is cut at ``k``.  A pass that
        returns fewer than ``k`` pairs is repeated with a lower cut (twice the sample rank, then no cut): at most three.

        The estimate only decides how much is emitted: a pass lists EVERY novel pair at or above its cut and counts
        them exactly, so once the count is at least ``k`` (or there is no cut) and within the buffer, the ``k`` best
        of all pairs are among the listed ones and the sorted prefix is the exact answer.  A count beyond the buffer
        raises ``ops.TooManyPairs`` instead of returning a truncated list."""
        k = int(k)
        if not 1 <= k <= self.DEEP_MAX_K:
            raise ValueError("k must be in 1..%d, got %d" % (self.DEEP_MAX_K, k))
        if k <= ops.PAIR_TOPK_MAX_K:
            return self.top_pairs(drug_feat, dis_feat, k, known)
        P, Q = self._split_lin1(drug_feat, dis_feat)
        tail = self._tail()
        kd, ks = (None, None) if known is None else known
        s = -(-k // 512)
        rank = -(-3 * k // (2 * s)) + 32
        sample = ops.pair_mlp_topk(P[::s], Q, *tail, None, None, ops.PAIR_TOPK_MAX_K)[2]
        capacity = 4 * k + 65536
        nan = float("nan")
        for r in (rank, 2 * rank, None):
            everything = r is None or sample.numel() < r
            cut = nan if everything else float(sample[r - 1])
            drug, dis, logit, n = ops.pair_mlp_above(P, Q, *tail, kd, ks, cut, capacity)
            if n >= k or everything or cut != cut:
                break
        return drug[:k], dis[:k], logit[:k]

    def score_pairs(self, drug_feat, dis_feat, drug_ids, dis_ids):
        """The eval-mode logit of every listed pair ``(drug_ids[e], dis_ids[e])`` (``ops.pair_mlp_score_list``): an fp32
        device tensor in the caller's order, every logit bit-identical to the one :meth:`top_pairs`,
        :meth:`top_pairs_per_row` and :meth:`pairs_above` return for the pair (``lin1`` is split as there; this is not
        the arithmetic of :meth:`forward`).  Duplicates are allowed.  ``ValueError`` for id lists of different length or
        of float / bool type, before anything touches the device; ``RuntimeError`` for an id out of range."""
        drug_ids, dis_ids = pair_ids(drug_ids, dis_ids)
        P, Q = self._split_lin1(drug_feat, dis_feat)
        return ops.pair_mlp_score_list(P, Q, *self._tail(), drug_ids.to(P.device), dis_ids.to(P.device))

    def rank_pairs(self, drug_feat, dis_feat, drug_ids, dis_ids, by="disease", known=None):
        """Where every listed pair stands among the candidates of its row (``ops.pair_mlp_rank_list``): ``(logit, above,
        total)`` device tensors in the caller's order.  ``by="disease"``: the query is the pair's disease and the
        candidates are all drugs (the filtered rank of a held-out drug for its disease); ``by="drug"``: the mirror.
        ``total`` counts the other candidates of the row whose pair is not in ``known = (drug_ids, disease_ids)``,
        ``above`` those of them that rank before the listed pair (logit descending, ties by candidate id ascending, NaN
        last): ``above + 1`` is the rank among ``total + 1``.  The listed pair never counts itself, whether it is in
        ``known`` changes nothing, and duplicates get equal results.  The logits are those of :meth:`score_pairs`, so a
        pair that :meth:`top_pairs_per_row` lists at position ``r`` of its row has ``above == r``.

        Every listed pair scans its whole row: ``n_pairs x n_cand`` scores.  Only the distinct listed query rows are
        given to the kernel, so the known-pair bitmap is ``n_cand x ceil(n_distinct / 32)`` words.  Argument errors as
        in :meth:`score_pairs`, and ``ValueError`` for a bad ``by``."""
        if by not in ("disease", "drug"):
            raise ValueError('by must be "disease" or "drug", got %r' % (by,))
        drug_ids, dis_ids = pair_ids(drug_ids, dis_ids)
        P, Q = self._split_lin1(drug_feat, dis_feat)
        dev = P.device
        X, C = (Q, P) if by == "disease" else (P, Q)
        pq, pc = (dis_ids, drug_ids) if by == "disease" else (drug_ids, dis_ids)
        pq, pc = pq.to(dev), pc.to(dev)
        n_query, n_cand = int(X.shape[0]), int(C.shape[0])
        # the distinct listed rows become the query side; an id out of range stays -1 and is flagged by the kernel
        q_ok = (pq >= 0) & (pq < n_query)
        rows = torch.unique(pq[q_ok])
        pos = torch.full((max(n_query, 1),), -1, dtype=torch.long, device=dev)
        pos[rows] = torch.arange(rows.numel(), device=dev)
        pq_new = torch.where(q_ok, pos[pq.clamp(0, max(n_query - 1, 0))], torch.full_like(pq, -1))
        kq = kc = None
        if known is not None:
            kd, ks = known
            kq, kc = (ks, kd) if by == "disease" else (kd, ks)
            kq, kc = _remap_known(kq.to(dev).long(), kc.to(dev).long(), rows, n_query, n_cand)
        return ops.pair_mlp_rank_list(X.index_select(0, rows), C, *self._tail(), pq_new, pc, kq, kc)


def pair_ids(drug_ids, dis_ids):
    """The two id lists of a pair list as 1-D int64 tensors (on the device they came on); ``ValueError`` for float,
    complex or bool ids, more than one dimension or different lengths."""
    out = []
    for name, ids in (("drug_ids", drug_ids), ("disease_ids", dis_ids)):
        t = ids if isinstance(ids, torch.Tensor) else torch.as_tensor(np.asarray(ids))
        if t.numel() == 0 and t.dim() == 1 and not isinstance(ids, (torch.Tensor, np.ndarray)):
            t = t.long()  # an empty Python list has no dtype of its own
        if t.dim() != 1 or t.is_floating_point() or t.is_complex() or t.dtype == torch.bool:
            raise ValueError("%s must be a 1-D list of integer ids, got %s of shape %s" % (name, t.dtype, tuple(t.shape)))
        out.append(t.detach().long())
    if out[0].numel() != out[1].numel():
        raise ValueError("drug / disease id lists differ in length: %d vs %d" % (out[0].numel(), out[1].numel()))
    return out[0], out[1]


def query_rows(rows, n_query: int):
    """``rows`` as a CPU int64 tensor of unique query ids in ``[0, n_query)``, or None; ``ValueError`` otherwise."""
    if rows is None:
        return None
    r = rows if isinstance(rows, torch.Tensor) else torch.as_tensor(np.asarray(rows))
    if r.dim() != 1 or r.is_floating_point() or r.is_complex() or r.dtype == torch.bool:
        raise ValueError("rows must be a 1-D list of integer query ids, got %s of shape %s" % (r.dtype, tuple(r.shape)))
    r = r.detach().cpu().long()
    if r.numel() and (int(r.min()) < 0 or int(r.max()) >= n_query):
        raise ValueError("rows holds a query id outside [0, %d)" % n_query)
    if torch.unique(r).numel() != r.numel():
        raise ValueError("rows holds a duplicate query id")
    return r


def _remap_known(kq, kc, rows, n_query, n_cand):
    """The known pairs of the query subset ``rows``, with query ids renumbered to positions in ``rows``.  A pair with an
    id outside ``[0, n_query) x [0, n_cand)`` is kept with query -1, so that the kernel still flags it."""
    if n_query == 0:
        return kq, kc
    pos = torch.full((n_query,), -1, dtype=torch.long, device=rows.device)
    pos[rows] = torch.arange(rows.numel(), device=rows.device)
    q_ok = (kq >= 0) & (kq < n_query)
    c_ok = (kc >= 0) & (kc < n_cand)
    q_new = torch.where(q_ok, pos[kq.clamp(0, n_query - 1)], torch.full_like(kq, -1))
    keep = (q_new >= 0) | ~q_ok | ~c_ok
    return q_new[keep], kc[keep]


class Net(nn.Module):
    """``TGCN[GCMCLayer x L] || FGCN -> Attention -> MLPDecoder`` — model.py:4-103.

    ``args`` carries the fields the reference reads (model.py:10-57): ``rating_vals``,
    ``src_in_units``, ``dst_in_units``, ``gcn_agg_units``, ``gcn_out_units``, ``dropout``,
    ``gcn_agg_accum``, ``model_activation``, ``share_param``, ``device``, ``layers``,
    ``fdim_drug``, ``fdim_disease``, ``nhid1``, ``nhid2``, ``attention_dropout``.
    """

    def __init__(self, args):
        super().__init__()
        self.layers = args.layers
        self._act = get_activation(args.model_activation)
        self.rating_vals = args.rating_vals
        self.device = args.device
        self.TGCN = nn.ModuleList()
        self.TGCN.append(GCMCLayer(args.rating_vals, args.src_in_units, args.dst_in_units,
                                   args.gcn_agg_units, args.gcn_out_units, args.dropout,
                                   args.gcn_agg_accum, agg_act=self._act,
                                   share_user_item_param=args.share_param, device=args.device))
        for _ in range(1, args.layers):
            width = args.gcn_out_units * (len(args.rating_vals) if args.gcn_agg_accum == "stack" else 1)
            self.TGCN.append(GCMCLayer(args.rating_vals, args.gcn_out_units, args.gcn_out_units, width,
                                       args.gcn_out_units, args.dropout, args.gcn_agg_accum,
                                       agg_act=self._act, share_user_item_param=args.share_param,
                                       ini=False, device=args.device))
        self.FGCN = FGCN(args.fdim_drug, args.fdim_disease, args.nhid1, args.nhid2, args.dropout)
        self.attention = Attention(args.gcn_out_units, dropout_rate=args.attention_dropout)
        self.decoder = MLPDecoder(in_units=args.gcn_out_units, dropout_rate=args.dropout)

    def forward(self, enc_graph, dec_graph, drug_graph, drug_sim_feat, drug_feat, dis_graph,
                disease_sim_feat, dis_feat, drug_feature_graph=None, disease_feature_graph=None,
                Two_Stage=False):
        drug_feats, dis_feats, drug_out, drug_sim_out, dis_out, dis_sim_out = self._encode(
            enc_graph, drug_graph, drug_sim_feat, drug_feat, dis_graph, disease_sim_feat, dis_feat, drug_feature_graph,
            disease_feature_graph, Two_Stage)
        pred = self.decoder(dec_graph, drug_feats, dis_feats)
        return pred, drug_out, drug_sim_out, dis_out, dis_sim_out

    def embed(self, enc_graph, drug_graph, drug_sim_feat, drug_feat, dis_graph, disease_sim_feat, dis_feat,
              drug_feature_graph=None, disease_feature_graph=None, Two_Stage=False):
        """``forward`` without the decoder: the attention-fused ``(drug_feats, dis_feats)`` the decoder consumes
        (model.py:236-238 of the reference's flow).  Same arguments as ``forward`` minus ``dec_graph``."""
        drug_feats, dis_feats, *_ = self._encode(enc_graph, drug_graph, drug_sim_feat, drug_feat, dis_graph,
                                                 disease_sim_feat, dis_feat, drug_feature_graph, disease_feature_graph,
                                                 Two_Stage)
        return drug_feats, dis_feats

    def _encode(self, enc_graph, drug_graph, drug_sim_feat, drug_feat, dis_graph, disease_sim_feat, dis_feat,
                drug_feature_graph, disease_feature_graph, Two_Stage):
        drug_out = dis_out = None
        for i, layer in enumerate(self.TGCN):
            drug_o, dis_o = layer(enc_graph, drug_feat, dis_feat, Two_Stage)
            if i == 0:
                drug_out, dis_out = drug_o, dis_o
            else:
                drug_out = drug_out + drug_o / float(i + 1)
                dis_out = dis_out + dis_o / float(i + 1)
            drug_feat, dis_feat = drug_o, dis_o  # the raw layer output feeds the next layer (:75-76)

        drug_sim_out, dis_sim_out, *_ = self.FGCN(drug_graph, drug_sim_feat, dis_graph, disease_sim_feat,
                                                  drug_feature_graph, disease_feature_graph)
        drug_feats, _ = self.attention.fuse(drug_out, drug_sim_out)
        dis_feats, _ = self.attention.fuse(dis_out, dis_sim_out)
        return drug_feats, dis_feats, drug_out, drug_sim_out, dis_out, dis_sim_out


def common_loss(emb1, emb2):
    """utils.py:87-95: MSE between the two centred, row-normalised Gram matrices."""
    emb1 = F.normalize(emb1 - emb1.mean(0, keepdim=True), p=2, dim=1)
    emb2 = F.normalize(emb2 - emb2.mean(0, keepdim=True), p=2, dim=1)
    return torch.mean((emb1 @ emb1.t() - emb2 @ emb2.t()) ** 2)
