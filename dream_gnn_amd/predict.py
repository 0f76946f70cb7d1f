"""The model's deliverable: the most likely NEW drug-disease associations of a trained ``Net``.

Counterpart of the reference's ``get_top_novel_predictions`` (train.py:26-151, called per fold at :370-376 with
``--top_k``, default 200).  The reference lists every pair absent from the association matrix in Python, re-runs the
whole model (encoder included) on decoder graphs of 5 000 of them at a time, applies ``sigmoid`` and sorts the scores
with pandas.  Here the encoder runs once (``Net.embed``), the decoder's first layer is split into two small GEMMs, and
one HIP kernel scores every pair and keeps the k best on the device (``MLPDecoder.top_pairs``,
``csrc/dgmi_pairs.hip``).

Ranking uses the fp32 LOGIT, not the fp32 sigmoid: in fp32 the sigmoid rounds to exactly 1.0 above a logit of about
17, and the reference's sort leaves the order among equal scores unspecified.  Here the order is the logit
descending, ties broken by ``(drug_id, disease_id)`` ascending (the reference's drug-major enumeration order), NaN
logits last.  Wherever the reference's own scores are distinct, the two orders agree.

``top_novel_per_disease`` / ``top_novel_per_drug`` answer the per-entity questions (which drugs fit disease X, which
new indications fit drug Y): the k best novel candidates of every query row, from one HIP kernel over the same scorer
(``MLPDecoder.top_pairs_per_row``, ``csrc/dgmi_pairs_rows.hip``).  Within a row the order is the global one restricted
to that row: logit descending, ties by candidate id ascending, NaN last.

``novel_pairs_above`` / ``count_novel_pairs_above`` ask by score instead of by count (every novel pair the model puts at
or above a cut, and how many there are), and ``top_novel_pairs_deep`` ranks beyond the on-chip limit (``k`` up to 2**20):
one streaming HIP kernel over the same scorer emits the qualifying pairs with an exact count, a device sort orders them
(``MLPDecoder.pairs_above`` / ``top_pairs_deep``, ``csrc/dgmi_pairs_above.hip``).  Same order, same logit bits.

``score_pairs`` / ``rank_pairs`` answer the reverse question: here is a pair, how does the model score it and where
does it stand among the candidates of its row.  One HIP kernel scores the listed pairs, a second streams every
candidate of each pair's row through the same scorer and only counts (``MLPDecoder.score_pairs`` / ``rank_pairs``,
``csrc/dgmi_pairs_given.hip``).  Same logit bits, same order, so a rank agrees with the pair's position in
``top_novel_per_disease`` / ``top_novel_per_drug``; ``PairRanks`` turns the ranks into hits@k and MRR.
"""
from __future__ import annotations

from dataclasses import dataclass

import numpy as np
import torch

from . import ops
from .model import pair_ids, query_rows

#: the largest ``k`` the on-chip top-k takes; there is no other path inside :func:`top_novel_pairs` (for a deeper
#: list see :func:`top_novel_pairs_deep`, for a list by score :func:`novel_pairs_above`)
MAX_K = ops.PAIR_TOPK_MAX_K
#: the largest ``k`` of :func:`top_novel_pairs_deep`
DEEP_MAX_K = 1 << 20
#: the largest ``max_pairs`` of :func:`novel_pairs_above`
MAX_PAIRS = ops.PAIR_EMIT_MAX_RECORDS
#: the largest ``k`` per row of the per-disease / per-drug lists
ROW_MAX_K = ops.ROW_TOPK_MAX_K


@dataclass
class NovelPairs:
    """The ranked pairs, CPU tensors in rank order: int64 ``drug_id`` / ``disease_id``, fp32 ``logit`` and
    ``score = sigmoid(logit)``."""

    drug_id: torch.Tensor
    disease_id: torch.Tensor
    logit: torch.Tensor
    score: torch.Tensor

    def __len__(self) -> int:
        return int(self.drug_id.numel())

    def to_frame(self, drug_names=None):
        """A pandas DataFrame with the reference's columns (train.py:129-141): ``drug_id, disease_id, score`` and,
        when ``drug_names`` (indexable by drug id) is given, ``drug_name``."""
        import pandas as pd

        df = pd.DataFrame({"drug_id": self.drug_id.numpy(), "disease_id": self.disease_id.numpy(),
                           "score": self.score.numpy()})
        if drug_names is not None:
            names = list(drug_names)
            df["drug_name"] = [names[i] for i in df["drug_id"]]
        return df


def _known_ids(known, n_drug: int, n_dis: int, device):
    """``known`` as (drug_ids, disease_ids) device tensors, or (None, None) when nothing is known."""
    if known is None:
        return None, None
    if isinstance(known, (tuple, list)):
        if len(known) != 2:
            raise ValueError("known must be an (n_drug, n_dis) matrix or a (drug_ids, disease_ids) pair")
        kd, ks = (torch.as_tensor(np.asarray(x) if not isinstance(x, torch.Tensor) else x).reshape(-1) for x in known)
        if kd.numel() != ks.numel():
            raise ValueError("known drug / disease id lists differ in length: %d vs %d" % (kd.numel(), ks.numel()))
        if kd.is_floating_point() or ks.is_floating_point():
            raise ValueError("known ids must be integers")
    else:
        shape = tuple(known.shape)
        if shape != (n_drug, n_dis):
            raise ValueError("known matrix has shape %s, expected (n_drug, n_dis) = (%d, %d)" % (shape, n_drug, n_dis))
        if isinstance(known, torch.Tensor):
            kd, ks = (known != 0).nonzero(as_tuple=True)  # NaN != 0: a NaN cell counts as known, as in train.py:55
        else:
            kd, ks = (torch.from_numpy(x) for x in np.nonzero(np.asarray(known) != 0))
    if kd.numel() == 0:
        return None, None
    return kd.to(device=device, dtype=torch.int64), ks.to(device=device, dtype=torch.int64)


def top_novel_pairs(net, batch, known, k: int = 200) -> NovelPairs:
    """The ``min(k, #novel)`` pairs not in ``known`` that ``net`` scores highest, eval mode.

    ``batch``: one fold's un-augmented inputs (the dict of ``harness``: ``enc_graph``, ``drug_graph``,
    ``drug_sim_feat``, ``drug_feat``, ``disease_graph``, ``disease_sim_feat``, ``disease_feat`` and the optional
    ``drug_feature_graph`` / ``disease_feature_graph``).  ``known``: the association matrix (n_drug x n_dis, numpy or
    torch, nonzero = known; every known association of the dataset, as train.py:46 uses) or a
    ``(drug_ids, disease_ids)`` pair.  ``1 <= k <= 1024``; larger ``k`` raises ``ValueError``.

    The encoder runs once under ``no_grad``; the net's training flag is restored afterwards.  Ordered by logit
    descending, ties by ``(drug_id, disease_id)`` ascending, NaN last (module docstring: why the logit and not the
    sigmoid)."""
    k = int(k)
    if not 1 <= k <= MAX_K:
        raise ValueError("k must be in 1..%d (the on-chip top-k limit), got %d" % (MAX_K, k))
    n_drug, n_dis = int(batch["drug_feat"].shape[0]), int(batch["disease_feat"].shape[0])
    device = batch["drug_feat"].device
    kd, ks = _known_ids(known, n_drug, n_dis, device)

    was_training = net.training
    net.eval()
    try:
        with torch.no_grad():
            hd, hs = net.embed(batch["enc_graph"], batch["drug_graph"], batch["drug_sim_feat"], batch["drug_feat"],
                               batch["disease_graph"], batch["disease_sim_feat"], batch["disease_feat"],
                               batch.get("drug_feature_graph"), batch.get("disease_feature_graph"))
            drug, dis, logit = net.decoder.top_pairs(hd, hs, k, None if kd is None else (kd, ks))
    finally:
        net.train(was_training)
    logit = logit.cpu()
    return NovelPairs(drug.cpu(), dis.cpu(), logit, torch.sigmoid(logit))


@dataclass
class NovelLists:
    """Per-row rankings, CPU tensors: ``by`` (``"disease"`` or ``"drug"``, the query side), int64 ``query_id`` (n_q),
    int64 ``drug_id`` / ``disease_id`` (n_q x k, -1 past a row's count), fp32 ``logit`` and ``score = sigmoid(logit)``
    (n_q x k, NaN past the count) and int64 ``count`` (n_q).  Row r ranks the candidates of query ``query_id[r]``."""

    by: str
    query_id: torch.Tensor
    drug_id: torch.Tensor
    disease_id: torch.Tensor
    logit: torch.Tensor
    score: torch.Tensor
    count: torch.Tensor

    def __len__(self) -> int:
        return int(self.query_id.numel())

    def to_frame(self, drug_names=None):
        """A pandas DataFrame in long form, one line per returned entry (padding left out), rows in order and each
        row's entries by rank: ``query_id, rank, drug_id, disease_id, score`` (rank 1 is the best) and, when
        ``drug_names`` (indexable by drug id) is given, ``drug_name``."""
        import pandas as pd

        k = int(self.drug_id.shape[1]) if self.drug_id.dim() == 2 else 0
        valid = (torch.arange(k)[None, :] < self.count[:, None]).reshape(-1).numpy()
        rank = np.tile(np.arange(1, k + 1), len(self))
        qid = np.repeat(self.query_id.numpy(), k)
        df = pd.DataFrame({"query_id": qid[valid], "rank": rank[valid],
                           "drug_id": self.drug_id.reshape(-1).numpy()[valid],
                           "disease_id": self.disease_id.reshape(-1).numpy()[valid],
                           "score": self.score.reshape(-1).numpy()[valid]})
        if drug_names is not None:
            names = list(drug_names)
            df["drug_name"] = [names[i] for i in df["drug_id"]]
        return df


def _top_novel_lists(net, batch, known, k, by, rows) -> NovelLists:
    k = int(k)
    if not 1 <= k <= ROW_MAX_K:
        raise ValueError("k must be in 1..%d (the per-row on-chip top-k limit), got %d" % (ROW_MAX_K, k))
    n_drug, n_dis = int(batch["drug_feat"].shape[0]), int(batch["disease_feat"].shape[0])
    device = batch["drug_feat"].device
    kd, ks = _known_ids(known, n_drug, n_dis, device)
    rows = query_rows(rows, n_dis if by == "disease" else n_drug)

    was_training = net.training
    net.eval()
    try:
        with torch.no_grad():
            hd, hs = net.embed(batch["enc_graph"], batch["drug_graph"], batch["drug_sim_feat"], batch["drug_feat"],
                               batch["disease_graph"], batch["disease_sim_feat"], batch["disease_feat"],
                               batch.get("drug_feature_graph"), batch.get("disease_feature_graph"))
            qid, cand, logit, count = net.decoder.top_pairs_per_row(hd, hs, k, by, None if kd is None else (kd, ks), rows)
    finally:
        net.train(was_training)
    qid, cand, logit, count = qid.cpu(), cand.cpu(), logit.cpu(), count.cpu().long()
    qmat = torch.where(cand >= 0, qid[:, None].expand_as(cand), torch.full_like(cand, -1))
    drug, dis = (cand, qmat) if by == "disease" else (qmat, cand)
    return NovelLists(by, qid, drug, dis, logit, torch.sigmoid(logit), count)


def top_novel_per_disease(net, batch, known, k: int = 10, diseases=None) -> NovelLists:
    """For every disease (or the diseases in ``diseases``, unique ids, in that order), the ``min(k, #novel)`` drugs not
    known to treat it that ``net`` scores highest, eval mode: the case-study table.  ``batch`` and ``known`` as in
    :func:`top_novel_pairs`; ``1 <= k <= 128``.  Validates ``k``, ``known`` and ``diseases`` before the model runs; the
    encoder runs once under ``no_grad`` and the training flag is restored.  Each row is ordered by logit descending,
    ties by drug id ascending, NaN last."""
    return _top_novel_lists(net, batch, known, k, "disease", diseases)


def top_novel_per_drug(net, batch, known, k: int = 10, drugs=None) -> NovelLists:
    """For every drug (or the drugs in ``drugs``), the ``min(k, #novel)`` diseases it is not known to treat that
    ``net`` scores highest: its best new indications.  Otherwise as :func:`top_novel_per_disease`; ties by disease id
    ascending."""
    return _top_novel_lists(net, batch, known, k, "drug", drugs)


def _cut_logit(min_score, min_logit) -> float:
    """The one cut, as an fp32 logit: ``min_logit`` itself, or ``log(p / (1 - p))`` of ``min_score = p`` computed in
    float64 and rounded once to float32."""
    if (min_score is None) == (min_logit is None):
        raise ValueError("give exactly one of min_score and min_logit")
    if min_logit is not None:
        return float(np.float32(min_logit))
    p = float(min_score)
    if not 0.0 < p < 1.0:
        raise ValueError("min_score must lie in (0, 1), got %r (use min_logit for a cut on the logit)" % (min_score,))
    return float(np.float32(np.log(np.float64(p) / (np.float64(1.0) - np.float64(p)))))


def _with_embedding(net, batch, fn):
    """``fn(hd, hs)`` on the eval-mode embeddings, under ``no_grad``; the net's training flag is restored."""
    was_training = net.training
    net.eval()
    try:
        with torch.no_grad():
            hd, hs = net.embed(batch["enc_graph"], batch["drug_graph"], batch["drug_sim_feat"], batch["drug_feat"],
                               batch["disease_graph"], batch["disease_sim_feat"], batch["disease_feat"],
                               batch.get("drug_feature_graph"), batch.get("disease_feature_graph"))
            return fn(hd, hs)
    finally:
        net.train(was_training)


def _known_of(batch, known):
    n_drug, n_dis = int(batch["drug_feat"].shape[0]), int(batch["disease_feat"].shape[0])
    kd, ks = _known_ids(known, n_drug, n_dis, batch["drug_feat"].device)
    return None if kd is None else (kd, ks)


def _novel_pairs(drug, dis, logit) -> NovelPairs:
    logit = logit.cpu()
    return NovelPairs(drug.cpu(), dis.cpu(), logit, torch.sigmoid(logit))


def novel_pairs_above(net, batch, known, min_score=None, min_logit=None, max_pairs: int = 1 << 20) -> NovelPairs:
    """EVERY pair not in ``known`` that ``net`` puts at or above a cut, eval mode, in the order of
    :func:`top_novel_pairs`.  ``batch`` and ``known`` as there.  Exactly one of ``min_score`` (a probability in (0, 1))
    and ``min_logit`` is given; ``min_logit = NaN`` lists every novel pair.

    The cut is applied to the LOGIT: ``min_score = p`` is translated once to ``float32(log(p / (1 - p)))`` (computed in
    float64) and a pair qualifies iff its fp32 logit is >= that value, inclusive.  The fp32 sigmoid is not compared, for
    the reason the module docstring gives: it saturates to exactly 1.0 and is not one-to-one, so a cut on it would not
    name a set.  A returned ``score`` can therefore differ from ``min_score`` by an ulp on either side.

    Raises ``ops.TooManyPairs`` (``.count`` exact, ``.max_pairs``) when more than ``max_pairs`` (1..2**24) pairs
    qualify: the list is never truncated silently.  Validates ``known``, the cut and ``max_pairs`` before the model
    runs; the encoder runs once under ``no_grad`` and the training flag is restored."""
    cut = _cut_logit(min_score, min_logit)
    max_pairs = ops._check_max_pairs(max_pairs)
    kn = _known_of(batch, known)
    return _novel_pairs(*_with_embedding(net, batch, lambda hd, hs: net.decoder.pairs_above(hd, hs, cut, kn, max_pairs)))


def count_novel_pairs_above(net, batch, known, min_score=None, min_logit=None) -> int:
    """How many pairs :func:`novel_pairs_above` lists at this cut: exact, without a limit, nothing stored."""
    cut = _cut_logit(min_score, min_logit)
    kn = _known_of(batch, known)
    return int(_with_embedding(net, batch, lambda hd, hs: net.decoder.count_pairs_above(hd, hs, cut, kn)))


def top_novel_pairs_deep(net, batch, known, k: int) -> NovelPairs:
    """:func:`top_novel_pairs` for ``1 <= k <= 2**20``: the ``min(k, #novel)`` best novel pairs in the same order, exact
    (``MLPDecoder.top_pairs_deep``: a sampled cut, one emit pass with an exact count, a device sort).  Raises
    ``ops.TooManyPairs`` if a pass finds more pairs than its ``4 k + 65536`` slots hold.  Validates ``k`` and ``known``
    before the model runs; the encoder runs once under ``no_grad`` and the training flag is restored."""
    k = int(k)
    if not 1 <= k <= DEEP_MAX_K:
        raise ValueError("k must be in 1..%d, got %d" % (DEEP_MAX_K, k))
    kn = _known_of(batch, known)
    return _novel_pairs(*_with_embedding(net, batch, lambda hd, hs: net.decoder.top_pairs_deep(hd, hs, k, kn)))


@dataclass
class PairRanks:
    """Given pairs and where each stands in its row, CPU tensors in the caller's order: int64 ``drug_id`` /
    ``disease_id``, fp32 ``logit`` and ``score = sigmoid(logit)``, int64 ``rank`` (1 is the best: one more than the
    number of other novel candidates of the row that rank before the pair) and int64 ``n_candidates`` (the length of
    the list the pair is ranked in, itself included).  ``by`` names the query side: ``"disease"`` ranks the pair's drug
    among all drugs for its disease, ``"drug"`` the pair's disease among all diseases for its drug."""

    by: str
    drug_id: torch.Tensor
    disease_id: torch.Tensor
    logit: torch.Tensor
    score: torch.Tensor
    rank: torch.Tensor
    n_candidates: torch.Tensor

    def __len__(self) -> int:
        return int(self.drug_id.numel())

    def hits_at(self, k: int) -> float:
        """The fraction of the listed pairs with ``rank <= k`` (NaN for an empty list)."""
        k = int(k)
        if k < 1:
            raise ValueError("k must be at least 1, got %d" % k)
        return float((self.rank <= k).double().mean()) if len(self) else float("nan")

    def mrr(self) -> float:
        """The mean reciprocal rank of the listed pairs (NaN for an empty list)."""
        return float((1.0 / self.rank.double()).mean()) if len(self) else float("nan")

    def to_frame(self, drug_names=None):
        """A pandas DataFrame, one line per listed pair in the caller's order: ``drug_id, disease_id, score, rank,
        n_candidates`` and, when ``drug_names`` (indexable by drug id) is given, ``drug_name``."""
        import pandas as pd

        df = pd.DataFrame({"drug_id": self.drug_id.numpy(), "disease_id": self.disease_id.numpy(),
                           "score": self.score.numpy(), "rank": self.rank.numpy(),
                           "n_candidates": self.n_candidates.numpy()})
        if drug_names is not None:
            names = list(drug_names)
            df["drug_name"] = [names[i] for i in df["drug_id"]]
        return df


def score_pairs(net, batch, drug_ids, disease_ids) -> NovelPairs:
    """How ``net`` scores the listed pairs ``(drug_ids[e], disease_ids[e])``, eval mode: a hand-picked candidate list.
    ``batch`` as in :func:`top_novel_pairs`.  Returned in the CALLER'S order, not sorted; duplicates are allowed.  Every
    logit has the bits the ranking functions of this module return for the pair.  Validates the id lists (equal
    length, integers) before the model runs; an id out of range raises ``RuntimeError``.  The encoder runs once under
    ``no_grad`` and the training flag is restored."""
    drug_ids, disease_ids = pair_ids(drug_ids, disease_ids)
    logit = _with_embedding(net, batch, lambda hd, hs: net.decoder.score_pairs(hd, hs, drug_ids, disease_ids))
    return _novel_pairs(drug_ids, disease_ids, logit)


def rank_pairs(net, batch, drug_ids, disease_ids, known, by: str = "disease") -> PairRanks:
    """The filtered rank of every listed pair among the candidates of its row, eval mode: the evaluation protocol for
    held-out indications.  ``by="disease"``: pair ``(d, s)`` is ranked among all drugs ``d'`` for disease ``s`` with
    ``(d', s)`` not in ``known``; ``by="drug"``: among all diseases for drug ``d``.  ``batch`` and ``known`` as in
    :func:`top_novel_pairs` (``known`` is normally the whole association matrix, held-out positives included).

    The listed pair never counts itself and is ranked whether or not it is in ``known``; the other known pairs of its
    row are left out.  Order within a row as everywhere in this module: logit descending, ties by candidate id
    ascending, NaN last, so a pair at position ``r`` (from 0) of its row in :func:`top_novel_per_disease` has rank
    ``r + 1``.  Duplicate listed pairs get equal results.  Returned in the caller's order.

    Every listed pair scans its whole row (``n_pairs x n_candidates`` scores).  Validates the id lists, ``known`` and
    ``by`` before the model runs; an id out of range raises ``RuntimeError``.  The encoder runs once under ``no_grad``
    and the training flag is restored."""
    if by not in ("disease", "drug"):
        raise ValueError('by must be "disease" or "drug", got %r' % (by,))
    drug_ids, disease_ids = pair_ids(drug_ids, disease_ids)
    kn = _known_of(batch, known)
    logit, above, total = _with_embedding(
        net, batch, lambda hd, hs: net.decoder.rank_pairs(hd, hs, drug_ids, disease_ids, by, kn))
    logit = logit.cpu()
    return PairRanks(by, drug_ids.cpu(), disease_ids.cpu(), logit, torch.sigmoid(logit), above.cpu().long() + 1,
                     total.cpu().long() + 1)
