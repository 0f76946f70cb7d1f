"""The host restatement of a given pair's rank (tests/_given_cases.py) against a literal double loop over designed tables
(ties, +-inf, NaN, signed zeros, fully known rows, the target in the known list, duplicates, ids out of range), the scan
planner against the library's workspace size, and PairRanks.hits_at / mrr on hand-written ranks.  No GPU."""
import math

import numpy as np
import pytest
import torch

import _given_cases as GC


def _before(lc, c2, lt, c):
    """Does candidate c2 (logit lc) rank before the target c (logit lt)?  Spelled out case by case."""
    if math.isnan(lt):
        return (not math.isnan(lc)) or c2 < c
    if math.isnan(lc):
        return False
    if lc > lt:
        return True
    return lc == lt and c2 < c  # -0.0 == 0.0 in Python too


def _loop(L, known, pq, pc):
    n_query, n_cand = L.shape
    out = []
    for q, c in zip(pq, pc):
        if not (0 <= q < n_query and 0 <= c < n_cand):
            out.append((float("nan"), -1, -1))
            continue
        above = total = 0
        for c2 in range(n_cand):
            if c2 == c or (known is not None and known[q, c2]):
                continue
            total += 1
            above += _before(float(L[q, c2]), c2, float(L[q, c]), c)
        out.append((float(L[q, c]), above, total))
    return out


def _same(L, known, pq, pc):
    logit, above, total = GC.expected_ranks(L, known, pq, pc)
    assert logit.dtype == np.float32 and above.dtype == np.int64 and total.dtype == np.int64
    ref = _loop(np.asarray(L, dtype=np.float32), known, pq, pc)
    for e, (l, a, t) in enumerate(ref):
        assert (math.isnan(l) and np.isnan(logit[e])) or l == float(logit[e]), e
        assert (a, t) == (int(above[e]), int(total[e])), (e, pq[e], pc[e], a, t, above[e], total[e])
    return logit, above, total


def _all_pairs(n_query, n_cand):
    q, c = np.divmod(np.arange(n_query * n_cand), n_cand)
    return q.tolist(), c.tolist()


def _special_table(seed=0):
    rng = np.random.default_rng(seed)
    L = rng.integers(-2, 3, (7, 13)).astype(np.float32)  # five levels: most logits tie
    L[0, [2, 9]] = np.inf
    L[1, [0, 5, 12]] = -np.inf
    L[2, [1, 2, 11]] = np.nan
    L[3, :] = np.nan                                      # a whole NaN row: the order is the id order
    L[4, [3, 4]] = [0.0, -0.0]                            # one value
    L[5, [0, 6]] = [np.inf, np.nan]
    return L


def test_every_pair_of_a_table_with_ties_inf_and_nan():
    L = _special_table()
    pq, pc = _all_pairs(*L.shape)
    logit, above, total = _same(L, None, pq, pc)
    assert (total == 12).all()
    # a row's `above` values are a permutation of 0..12: the order is total
    assert all(sorted(above[q * 13:(q + 1) * 13]) == list(range(13)) for q in range(7))
    assert above[3 * 13:4 * 13].tolist() == list(range(13))        # NaN row: by id
    assert above[0 * 13 + 2] == 0 and above[0 * 13 + 9] == 1        # the two +inf: first, tie by id
    assert sorted(above[1 * 13 + np.array([0, 5, 12])]) == [10, 11, 12]  # -inf: last among numbers (no NaN in row 1)
    assert sorted(above[2 * 13 + np.array([1, 2, 11])]) == [10, 11, 12]  # NaN after every number
    assert abs(int(above[4 * 13 + 3]) - int(above[4 * 13 + 4])) == 1 and above[4 * 13 + 3] < above[4 * 13 + 4]  # +-0 tie by id


def test_known_pairs_leave_the_row_and_the_target_stays():
    L = _special_table(1)
    rng = np.random.default_rng(2)
    known = rng.random(L.shape) < 0.3
    known[6, :] = True  # a fully known row: nothing to be ranked among
    pq, pc = _all_pairs(*L.shape)
    logit, above, total = _same(L, known, pq, pc)
    assert (above[6 * 13:] == 0).all() and (total[6 * 13:] == 0).all()
    # whether the target itself is known changes nothing
    for q, c in zip(pq, pc):
        one = known.copy()
        one[q, c] = not one[q, c]
        l2, a2, t2 = GC.expected_ranks(L, one, [q], [c])
        e = q * 13 + c
        assert (a2[0], t2[0]) == (above[e], total[e])
    # total is the row's novel count without the target
    novel = (~known).sum(1)
    for e, (q, c) in enumerate(zip(pq, pc)):
        assert total[e] == novel[q] - (0 if known[q, c] else 1)


def test_duplicates_order_and_ids_out_of_range():
    L = _special_table(3)
    known = np.random.default_rng(4).random(L.shape) < 0.2
    pq = [5, 0, 5, 7, -1, 2, 5, 0, 6]
    pc = [6, 2, 6, 0, 3, 13, 6, -1, 12]
    logit, above, total = _same(L, known, pq, pc)
    assert above[0] == above[2] == above[6] and total[0] == total[2] == total[6] and np.isnan(logit[[0, 2, 6]]).all()
    for e in (3, 4, 5, 7):
        assert np.isnan(logit[e]) and above[e] == -1 and total[e] == -1
    assert above[8] >= 0 and total[8] >= 0
    # empty list, empty tables
    l, a, t = GC.expected_ranks(L, None, [], [])
    assert l.size == a.size == t.size == 0
    l, a, t = GC.expected_ranks(np.zeros((3, 0), np.float32), None, [0, 1], [0, 0])
    assert np.isnan(l).all() and (a == -1).all() and (t == -1).all()
    l, a, t = GC.expected_ranks(np.full((1, 1), 2.5, np.float32), None, [0], [0])
    assert (l[0], a[0], t[0]) == (2.5, 0, 0)


def test_random_tables_against_the_loop():
    rng = np.random.default_rng(5)
    for shape in ((1, 1), (3, 31), (5, 40)):
        L = rng.integers(-3, 4, shape).astype(np.float32)
        L[rng.random(shape) < 0.05] = np.nan
        L[rng.random(shape) < 0.05] = np.inf
        known = rng.random(shape) < 0.3
        pq, pc = _all_pairs(*shape)
        _same(L, known, pq, pc)
        _same(L, None, pq, pc)


def test_scan_planner_matches_the_library():
    from dream_gnn_amd import _lib

    W = _lib.lib.dgmi_pair_rank_workspace_bytes
    for n_query, n_cand, n_pairs in ((1, 1, 1), (3, 31, 93), (2, 4100, 40), (681, 763, 3700), (50_000, 100_000, 10_000),
                                     (313, 100_000, 10_000)):
        n_groups, n_seg, seg, total = GC.given_plan(n_query, n_cand, n_pairs)
        assert W(n_query, n_cand, n_pairs) == total
        assert n_groups == -(-n_pairs // 32) and (n_seg - 1) * seg < n_cand <= n_seg * seg and 1 <= n_seg <= 256
    assert GC.given_plan(2, 4100, 40)[1] >= 2       # few pairs: the candidate axis is split
    assert GC.given_plan(2, 4100, 40)[2] < 128      # ... into segments shorter than a chunk
    assert GC.given_plan(40, 128, 40 * 128)[1] > 1 and GC.given_plan(1, 1, 1)[1] == 1


def _ranks(rank):
    from dream_gnn_amd.predict import PairRanks

    n = len(rank)
    z = torch.zeros(n)
    return PairRanks("disease", torch.arange(n), torch.arange(n), z, torch.sigmoid(z), torch.tensor(rank, dtype=torch.int64),
                     torch.full((n,), 100, dtype=torch.int64))


def test_pair_ranks_hits_and_mrr():
    r = _ranks([1, 2, 10, 11, 100])
    assert len(r) == 5
    assert r.hits_at(1) == pytest.approx(0.2) and r.hits_at(2) == pytest.approx(0.4) and r.hits_at(10) == pytest.approx(0.6)
    assert r.hits_at(99) == pytest.approx(0.8) and r.hits_at(100) == 1.0
    assert r.mrr() == pytest.approx((1 + 1 / 2 + 1 / 10 + 1 / 11 + 1 / 100) / 5)
    assert _ranks([1, 1, 1]).mrr() == 1.0 and _ranks([1, 1, 1]).hits_at(1) == 1.0
    with pytest.raises(ValueError):
        r.hits_at(0)
    empty = _ranks([])
    assert len(empty) == 0 and math.isnan(empty.hits_at(5)) and math.isnan(empty.mrr())
    df = r.to_frame()
    assert list(df.columns) == ["drug_id", "disease_id", "score", "rank", "n_candidates"] and df["rank"].tolist() == [1, 2, 10, 11, 100]
    assert list(r.to_frame(drug_names=list("abcde")).columns)[-1] == "drug_name"
