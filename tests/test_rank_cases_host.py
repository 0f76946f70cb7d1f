"""The reference of tests/test_gpu_rank_exact.py held to its own zero tolerance, without a GPU: every designed decoder
of tests/_rank_cases.py, evaluated with plain torch on the CPU in float32 and in float64, equals its integer table bit
for bit; ``expected_pairs`` / ``expected_rows`` equal a brute-force ``sorted()`` on tuple keys on small tables with
ties, +-inf and NaN; the restated per-row planner equals the library's workspace size."""
import math

import numpy as np
import pytest
import torch

import _rank_cases as R

# carrying columns / hidden units: both 64-column halves and both 32-row halves (where the MFMA operand layout
# splits), and one pair that shares an MFMA step (k and k + 64)
LAYOUTS = [dict(k0=0, k1=127, h0=0, h1=63), dict(k0=63, k1=64, h0=31, h1=32), dict(k0=69, k1=5, h0=40, h1=17)]


def _bits_equal(t, table):
    got = t.numpy()
    nan = np.isnan(table)
    assert np.array_equal(np.isnan(got), nan)
    assert np.array_equal(got[~nan].astype(np.float64), table[~nan].astype(np.float64))


def _check_design(design, table):
    for dtype in (torch.float32, torch.float64):
        _bits_equal(R.torch_logits(*design, dtype), table)


@pytest.mark.parametrize("layout", LAYOUTS)
def test_additive_design_is_exact(layout):
    rng = np.random.default_rng(1)
    a, c = rng.integers(-5000, 5000, 257), rng.integers(-5000, 5000, 131)
    _check_design(R.additive(a, c, b3=-3.0, **layout), R.additive_table(a, c, -3.0))
    a, c = rng.integers(-2, 3, 257), rng.integers(0, 4, 131)                       # few levels
    _check_design(R.additive(a, c, b3=0.25, **layout), R.additive_table(a, c, 0.25))
    a, c = np.arange(97) * 61, np.arange(61)                                       # arrival order and its negation
    _check_design(R.additive(a, c, **layout), R.additive_table(a, c))
    _check_design(R.additive(-a, -c, **layout), R.additive_table(-a, -c))
    big = 2 ** 24 - 200                                                            # the edge of the exact range
    a, c = np.array([big - 7, -big + 7, 0, 12345]), np.array([7, -7, 0, 100, -100])
    _check_design(R.additive(a, c, **layout), R.additive_table(a, c))


@pytest.mark.parametrize("sign", [1, -1])
def test_uniform_design_is_exact_and_keeps_inf_and_nan(sign):
    rng = np.random.default_rng(2)
    a, c = rng.integers(-3, 4, 70).astype(np.float64), rng.integers(-1, 3, 45).astype(np.float64)
    a[[3, 40]] = np.inf
    a[10] = np.nan
    c[20] = np.nan
    c[7] = 60000.0
    for b3 in (0.0, 0.5):
        table = R.uniform_table(a, c, sign, b3)
        assert np.isinf(table[3, 0]) and math.copysign(1.0, table[3, 0]) == sign
        assert np.isnan(table[10]).all() and np.isnan(table[:, 20]).all() and np.isnan(table[3, 20])
        assert np.isnan(table).sum() == 70 + 45 - 1, "an infinity turned into NaN"
        _check_design(R.uniform(a, c, sign, b3=b3), table)
        _check_design(R.uniform(a, c, sign, k0=77, b3=b3), table)


def test_dead_design_is_exact():
    b3 = float(np.float32(0.37))
    _check_design(R.dead(65, 33, b3), R.dead_table(65, 33, b3))


def test_a_design_outside_the_exact_range_is_refused():
    with pytest.raises(AssertionError):
        R.additive_table([2 ** 24], [1])
    with pytest.raises(AssertionError):
        R.uniform_table([2 ** 16], [1], 1)


# ---------------------------------------------------------------------------------------------
# expected_* against a brute-force sort
# ---------------------------------------------------------------------------------------------
def _brute_row(values, valid, k):
    """[(cand, logit)] of one row by Python's sorted() on (isnan, -logit, cand)."""
    items = [(c, float(v)) for c, v in enumerate(values) if valid[c]]
    items.sort(key=lambda t: (1, 0.0, t[0]) if math.isnan(t[1]) else (0, -t[1], t[0]))
    return items[:k]


def _brute_pairs(L, valid, k):
    items = [(i, j, float(L[i, j])) for i in range(L.shape[0]) for j in range(L.shape[1]) if valid[i, j]]
    items.sort(key=lambda t: (1, 0.0, t[0], t[1]) if math.isnan(t[2]) else (0, -t[2], t[0], t[1]))
    return items[:k]


def _random_table(rng, n, m, specials):
    L = rng.integers(-2, 3, (n, m)).astype(np.float32)   # 5 levels: large tie classes
    if specials:
        for v in (np.inf, -np.inf, np.nan):
            L[rng.random((n, m)) < 0.08] = v
        L[L == 0] *= rng.choice([1.0, -1.0])             # signed zeros rank as one value
    return L


def _same(a, b):
    return (math.isnan(a) and math.isnan(b)) or a == b


@pytest.mark.parametrize("seed", range(12))
def test_expected_order_equals_a_brute_force_sort(seed):
    rng = np.random.default_rng(seed)
    n, m = int(rng.integers(1, 40)), int(rng.integers(1, 40))
    L = _random_table(rng, n, m, specials=seed % 3 != 0)
    known = [None, rng.random((n, m)) < 0.3, rng.random((n, m)) < 0.95][seed % 3]
    if known is not None and n > 2:
        known[1, :] = True                               # an empty row
    valid = np.ones((n, m), bool) if known is None else ~known
    for k in (1, 2, 7, 33, 128, 1024):
        e = R.expected_pairs(L, known, k)
        want = _brute_pairs(L, valid, k)
        assert len(want) == e.drug.size == e.dis.size == e.logit.size
        for r, (i, j, v) in enumerate(want):
            assert (int(e.drug[r]), int(e.dis[r])) == (i, j) and _same(float(e.logit[r]), v), (k, r)
        if k > 128:
            continue
        for table, mask, vmask in ((L, known, valid), (L.T.copy(), None if known is None else known.T.copy(), valid.T)):
            e = R.expected_rows(table, mask, k)
            assert e.cand.shape == e.logit.shape == (table.shape[0], k)
            for q in range(table.shape[0]):
                want = _brute_row(table[q], vmask[q], k)
                assert int(e.count[q]) == len(want)
                assert [int(c) for c in e.cand[q, :len(want)]] == [c for c, _ in want], (k, q)
                assert all(_same(float(x), v) for x, (_, v) in zip(e.logit[q], want))
                assert (e.cand[q, len(want):] == -1).all() and np.isnan(e.logit[q, len(want):]).all()


def test_a_smaller_k_is_a_prefix():
    rng = np.random.default_rng(99)
    L = _random_table(rng, 37, 29, specials=True)
    known = rng.random(L.shape) < 0.2
    full_p, full_r = R.expected_pairs(L, known, 1024), R.expected_rows(L, known, 128)
    for k in (1, 3, 28, 29, 30, 128):
        R.assert_pairs_equal(R.cut_pairs(full_p, k), R.expected_pairs(L, known, k))
        R.assert_rows_equal(R.cut_rows(full_r, k), R.expected_rows(L, known, k))


def test_equality_helpers_notice_a_difference():
    e = R.expected_rows(np.array([[1.0, 1.0, np.nan, 0.5]], np.float32), None, 3)
    assert e.cand.tolist() == [[0, 1, 3]] and e.count.tolist() == [3]
    for cand, logit in (([[1, 0, 3]], e.logit), ([[0, 1, 3]], np.array([[1.0, 1.0, 0.5000001]], np.float32)),
                        ([[0, 1, 3]], np.array([[1.0, 1.0, np.nan]], np.float32))):
        with pytest.raises(AssertionError):
            R.assert_rows_equal((np.array(cand), logit, e.count), e)
    p = R.expected_pairs(np.array([[2.0, 2.0], [2.0, -np.inf]], np.float32), None, 4)
    assert list(zip(p.drug.tolist(), p.dis.tolist())) == [(0, 0), (0, 1), (1, 0), (1, 1)]
    with pytest.raises(AssertionError):
        R.assert_pairs_equal((p.drug[[1, 0, 2, 3]], p.dis[[1, 0, 2, 3]], p.logit), p)
    with pytest.raises(AssertionError):
        R.assert_pairs_equal((p.drug[:3], p.dis[:3], p.logit[:3]), p)


# ---------------------------------------------------------------------------------------------
# the restated planner
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_query", [1, 3, 33, 681, 2000, 50_000])
@pytest.mark.parametrize("n_cand", [1, 763, 3000, 8193, 20_011, 100_000])
@pytest.mark.parametrize("k", [1, 64, 65, 100, 128])
def test_restated_row_plan_matches_the_library(n_query, n_cand, k):
    from dream_gnn_amd import _lib

    assert _lib.lib.dgmi_row_topk_workspace_bytes(n_query, n_cand, k) == R.row_plan(n_query, n_cand, k)[2]


def test_which_calls_take_two_merge_rounds():
    for n_query in (1, 3, 33):
        for n_cand in (8193, 20_011, 100_000):
            for k in (65, 128):
                n_seg, fan, _ = R.row_plan(n_query, n_cand, k)
                assert fan == 32 and n_seg > fan, (n_query, n_cand, k, n_seg)
    assert R.row_plan(2000, 3000, 100)[:2] == (66, 32)   # the one two-round call of test_gpu_rank.py
    assert R.row_plan(681, 763, 128)[0] <= 32            # lrssl: one round
