"""Every novel pair at or above a cut, and the top-k beyond 1024, on the MI355X (csrc/dgmi_pairs_above.hip ->
ops.pair_mlp_above / pair_mlp_count_above -> MLPDecoder.pairs_above / top_pairs_deep -> predict.novel_pairs_above /
count_novel_pairs_above / top_novel_pairs_deep).

Expected answers never come from the code under test: the designed decoders of tests/_rank_cases.py give the exact set
and order as host integer arithmetic (a threshold list is ``expected_pairs`` at k = #novel filtered by ``L >= cut``), the
on-chip top-k (ops.pair_mlp_topk) gives the bits of a random decoder's best 1024, an fp64 restatement with the
project's tolerance rule (REL = 1e-6 times the term bound, test_gpu_pairs.py) bounds a random decoder's set, and the
reference's own get_top_novel_predictions at top_k = 1500 is the fixture tests/golden/novel_deep1500.npz.

Designed-decoder comparisons are equalities: the same ids, in the same order, with the same logit bits and counts."""
import ctypes
import functools
import os
import types

import numpy as np
import pytest
import torch

import _rank_cases as R
import test_gpu_pairs as TP
from test_gpu_rank_exact import _known_lists

pytestmark = pytest.mark.gpu

NAN, INF = float("nan"), float("inf")
B3 = float(np.float32(0.37))


# ---------------------------------------------------------------------------------------------
# the expected threshold list on the host
# ---------------------------------------------------------------------------------------------
def _qualifies(L, cut):
    """key(L) >= key(cut): ``L >= cut`` for a number (a NaN logit never does), everything for a NaN cut."""
    if cut != cut:
        return np.ones(L.shape, dtype=bool)
    with np.errstate(invalid="ignore"):
        return np.asarray(L, dtype=np.float32) >= np.float32(cut)


def _expected_above(L, known, cut):
    """The novel pairs of table ``L`` at or above ``cut`` in the documented order: ``expected_pairs`` over the pairs that
    are neither known nor below the cut, all of them (which is ``expected_pairs`` at k = #novel filtered by the cut,
    without sorting what the cut removes: ``test_expected_above_is_the_filtered_full_list`` holds the two together)."""
    novel = np.ones(L.shape, dtype=bool) if known is None else ~np.asarray(known, dtype=bool)
    sel = novel & _qualifies(L, cut)
    return R.expected_pairs(L, ~sel, int(sel.sum()))


def _filtered_full_list(L, known, cut):
    n_novel = L.size if known is None else int((~known).sum())
    full = R.expected_pairs(L, known, n_novel)
    keep = _qualifies(full.logit, cut)
    return R.Pairs(full.drug[keep], full.dis[keep], full.logit[keep])


def _above(dev, design, known, cut, max_pairs=1 << 20):
    from dream_gnn_amd import ops

    P, Q, *params = (t.to(dev) for t in design)
    kd, ks = _known_lists(known, dev)
    return ops.pair_mlp_above(P, Q, *params, kd, ks, cut, max_pairs)


def _count(dev, design, known, cut):
    from dream_gnn_amd import ops

    P, Q, *params = (t.to(dev) for t in design)
    kd, ks = _known_lists(known, dev)
    return ops.pair_mlp_count_above(P, Q, *params, kd, ks, cut)


def _check(dev, design, table, known, cuts, what):
    for cut in cuts:
        exp = _expected_above(table, known, cut)
        drug, dis, logit, n = _above(dev, design, known, cut)
        assert n == exp.drug.size == drug.numel(), "%s cut %r: count %d, expected %d" % (what, cut, n, exp.drug.size)
        assert drug.dtype == torch.int64 and dis.dtype == torch.int64 and logit.dtype == torch.float32
        R.assert_pairs_equal((drug, dis, logit), exp, "%s cut %r" % (what, cut))
        assert _count(dev, design, known, cut) == n, "%s cut %r: count-only query" % (what, cut)


def _cuts_of(table):
    """Below everything, inside the range, on a tied value, one ulp above the maximum, -inf, +inf, NaN, both zeros."""
    num = table[np.isfinite(table)]
    values, counts = np.unique(num, return_counts=True)
    tied = float(values[np.argmax(counts)])
    inside = float(np.float32(values[len(values) // 2]) + np.float32(0.5)) if len(values) > 1 else tied
    top = float(np.nextafter(np.float32(num.max()), np.float32(np.inf)))
    return [float(num.min()) - 10.0, inside, tied, top, -INF, INF, NAN, 0.0, -0.0]


# ---------------------------------------------------------------------------------------------
# (a) exact equality on designed decoders
# ---------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _levels(shape, seed=11, lo=-4, hi=5, with_known=True, b3=0.0):
    """(design, table, known mask or None) of an additive design on few integer levels (zero logits among them); shared
    by several tests, none of which writes to it."""
    rng = np.random.default_rng(seed)
    a, c = rng.integers(lo, hi, shape[0]), rng.integers(lo, hi, shape[1])
    known = (rng.random(shape) < 0.02) if with_known else None
    return R.additive(a, c, b3=b3), R.additive_table(a, c, b3), known


def test_expected_above_is_the_filtered_full_list():
    """Host only: the helper above against the definition, on a table with ties, zeros, NaN and infinities."""
    _, table, known = _levels((67, 70))
    table = table.copy()
    table[3, :] = np.nan
    table[5, 7], table[9, 1] = np.inf, -np.inf
    for cut in _cuts_of(table) + [1.0, -3.0]:
        a, b = _expected_above(table, known, cut), _filtered_full_list(table, known, cut)
        assert np.array_equal(a.drug, b.drug) and np.array_equal(a.dis, b.dis)
        assert np.array_equal(a.logit, b.logit, equal_nan=True)
    assert _expected_above(table, known, NAN).drug.size == int((~known).sum())
    assert _expected_above(table, known, -INF).drug.size == int((~known).sum()) - int((~known[3]).sum())


@pytest.mark.parametrize("shape", [(1, 1), (67, 70), (130, 257)])
def test_designed_decoders_every_cut(dev, shape):
    for with_known in (False, True):
        design, table, known = _levels(shape, with_known=with_known)
        _check(dev, design, table, known, _cuts_of(table), "additive %dx%d" % shape)
    design, table, known = _levels(shape, seed=12, b3=0.25)  # nothing at zero, another bias
    _check(dev, design, table, known, _cuts_of(table), "additive b3 %dx%d" % shape)


def test_signed_zero_cuts_select_the_same_set(dev):
    design, table, known = _levels((67, 70))
    assert (table == 0).any()
    a, b = _above(dev, design, known, 0.0), _above(dev, design, known, -0.0)
    assert a[3] == b[3] == int((~known & (table >= 0)).sum())
    for x, y in zip(a[:3], b[:3]):
        assert torch.equal(x, y)


def test_4096_by_4100_all_workgroups_flush(dev):
    """The 64-drug-chunk path with every workgroup of the persistent grid flushing several times: 472 000 of 16.8 M
    pairs qualify (a cut on a tied value, and the same set from a cut between two levels)."""
    shape = (4096, 4100)
    rng = np.random.default_rng(21)
    a, c = rng.integers(0, 40, shape[0]), rng.integers(0, 40, shape[1])
    design, table = R.additive(a, c), R.additive_table(a, c)
    known = rng.random(shape) < 0.01
    exp = _expected_above(table, known, 70.0)
    assert 400_000 < exp.drug.size < 550_000
    for cut in (70.0, 69.5):
        drug, dis, logit, n = _above(dev, design, known, cut)
        assert n == exp.drug.size
        R.assert_pairs_equal((drug, dis, logit), exp, "4096x4100 cut %r" % cut)
    assert _count(dev, design, known, NAN) == int((~known).sum())  # the count-only query has no limit
    from dream_gnn_amd import ops

    with pytest.raises(ops.TooManyPairs) as e:
        _above(dev, design, known, 60.0, max_pairs=1 << 20)
    assert e.value.count == int((~known & (table >= 60)).sum()) and e.value.max_pairs == 1 << 20


# ---------------------------------------------------------------------------------------------
# (b) ties, NaN and infinities
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(67, 70), (1, 129)])
def test_one_tie_class_is_ordered_by_id(dev, shape):
    b3 = B3
    design, table = R.dead(*shape, b3), R.dead_table(*shape, b3)
    above = float(np.nextafter(np.float32(b3), np.float32(np.inf)))
    _check(dev, design, table, None, [b3, above, float(np.nextafter(np.float32(b3), np.float32(-np.inf))), NAN], "dead")
    drug, dis, logit, n = _above(dev, design, None, b3)
    flat = np.arange(shape[0] * shape[1])
    assert n == flat.size and np.array_equal(drug.cpu().numpy(), flat // shape[1]) and np.array_equal(dis.cpu().numpy(), flat % shape[1])
    assert _above(dev, design, None, above)[3] == 0
    known = _levels(shape)[2]
    _check(dev, design, table, known, [b3, above, NAN], "dead with known pairs")


@pytest.mark.parametrize("sign", [1, -1])
def test_nan_and_infinite_logits(dev, sign):
    rng = np.random.default_rng(5)
    a, c = rng.integers(-3, 9, 70).astype(np.float64), rng.integers(-3, 9, 67).astype(np.float64)
    a[3], a[40] = np.nan, np.inf           # a NaN row, a row of sign * inf
    design, table = R.uniform(a, c, sign, b3=1.0), R.uniform_table(a, c, sign, b3=1.0)
    assert np.isnan(table[3]).all() and np.isinf(table[40]).all()
    known = rng.random(table.shape) < 0.05
    _check(dev, design, table, known, _cuts_of(table) + [1.0, sign * 4.0 + 1.0], "uniform sign %d" % sign)
    n_nan = int((~known[3]).sum())
    for cut in (-INF, -1e30, 0.0, INF):    # the NaN row reaches no numeric cut
        drug = _above(dev, design, known, cut)[0]
        assert not bool((drug == 3).any())
    drug, dis, logit, n = _above(dev, design, known, NAN)  # ... and comes last, in id order, under the NaN cut
    assert n == int((~known).sum())
    assert bool(torch.isnan(logit[n - n_nan:]).all()) and not bool(torch.isnan(logit[:n - n_nan]).any())
    assert bool((drug[n - n_nan:] == 3).all()) and dis[n - n_nan:].tolist() == np.nonzero(~known[3])[0].tolist()
    if sign == 1:
        drug, _, logit, n = _above(dev, design, known, INF)
        assert n == int((~known[40]).sum()) and bool((drug == 40).all()) and bool(torch.isinf(logit).all())


# ---------------------------------------------------------------------------------------------
# (c) dense emission and overflow
# ---------------------------------------------------------------------------------------------
def test_dense_emission_and_overflow(dev):
    """96 x 300 with everything qualifying: every fill check flushes."""
    from dream_gnn_amd import ops

    shape = (96, 300)
    design, table, _ = _levels(shape, seed=31, with_known=False)
    total = 28_800
    for cut in (NAN, float(table.min())):
        _check(dev, design, table, None, [cut], "dense")
        assert _above(dev, design, None, cut, max_pairs=total)[3] == total
    for max_pairs in (1000, total - 1):
        with pytest.raises(ops.TooManyPairs) as e:
            _above(dev, design, None, NAN, max_pairs=max_pairs)
        assert e.value.count == total and e.value.max_pairs == max_pairs
    # the raw op into views of sentinel-filled larger tensors: nothing is written outside the views
    P, Q, *params = (t.to(dev) for t in design)
    for cap, lead in ((1000, 0), (1536, 16), (2048 + 7, 3), (total, 5), (total + 100, 1)):
        big_d = torch.full((lead + cap + 4096,), -7, dtype=torch.int32, device=dev)
        big_s, big_l = big_d.clone(), torch.full((lead + cap + 4096,), 123.0, device=dev)
        count, info = torch.ops.dreamgnn_mi.pair_mlp_emit(P, Q, *params, None, None, NAN, big_d[lead:lead + cap],
                                                          big_s[lead:lead + cap], big_l[lead:lead + cap])
        assert count.dtype == torch.int64 and int(count) == total and info.tolist() == [0, 0]
        stored = min(cap, total)
        for big, fill in ((big_d, -7), (big_s, -7), (big_l, 123.0)):
            assert bool((big[:lead] == fill).all()) and bool((big[lead + stored:] == fill).all()), (cap, lead)
        d, s = big_d[lead:lead + stored].cpu().numpy().astype(np.int64), big_s[lead:lead + stored].cpu().numpy().astype(np.int64)
        assert d.min() >= 0 and d.max() < shape[0] and s.min() >= 0 and s.max() < shape[1]
        assert np.unique(d * shape[1] + s).size == stored            # distinct pairs ...
        R.assert_same_logits(big_l[lead:lead + stored].cpu().numpy(), table[d, s], "raw emit")  # ... with their logits
    # capacity 0: count only, empty record tensors
    e_i, e_f = torch.empty(0, dtype=torch.int32, device=dev), torch.empty(0, device=dev)
    count, _ = torch.ops.dreamgnn_mi.pair_mlp_emit(P, Q, *params, None, None, NAN, e_i, e_i.clone(), e_f)
    assert int(count) == total


def test_count_equals_the_host_count_at_five_cuts(dev):
    design, table, known = _levels((96, 300), seed=32)
    dec = R.designed_decoder(*design[2:]).to(dev)
    kd, ks = _known_lists(known, dev)
    P, Q = design[0].to(dev), design[1].to(dev)
    for cut in (-100.0, -2.0, 0.0, 3.0, 8.0):
        want = int((~known & (table >= cut)).sum())
        with torch.no_grad():
            assert dec.count_pairs_above(P, Q, cut, (kd, ks)) == want
    with torch.no_grad():
        assert dec.count_pairs_above(P, Q, 9.0) == 0 and dec.count_pairs_above(P, Q, NAN) == 96 * 300


def test_the_record_sort_alone(dev):
    """dgmi_pair_records_sort_f32 on records the test makes up: ties, both zeros, NaN, infinities, a prefix n."""
    rng = np.random.default_rng(41)
    n, extra = 20_000, 50
    drug, dis = rng.integers(0, 3000, n + extra).astype(np.int32), rng.integers(0, 2 ** 31 - 1, n + extra).astype(np.int32)
    logit = rng.integers(-5, 6, n + extra).astype(np.float32)
    logit[rng.random(n + extra) < 0.05] = np.nan
    logit[:8] = [np.inf, -np.inf, 0.0, -0.0, np.inf, -0.0, 0.0, -np.inf]
    dis[:8] = [5, 5, 9, 8, 4, 7, 6, 4]
    drug[:8] = 1
    d, s, l = (torch.from_numpy(x).to(dev) for x in (drug, dis, logit))
    torch.ops.dreamgnn_mi.pair_records_sort(d, s, l, n)
    nan = np.isnan(logit[:n])
    order = np.lexsort((dis[:n], drug[:n], -np.where(nan, 0.0, logit[:n]).astype(np.float64), nan))
    assert np.array_equal(d[:n].cpu().numpy(), drug[order]) and np.array_equal(s[:n].cpu().numpy(), dis[order])
    R.assert_same_logits(l[:n].cpu().numpy(), logit[order], "sorted records")
    assert np.array_equal(d[n:].cpu().numpy(), drug[n:]) and np.array_equal(s[n:].cpu().numpy(), dis[n:])  # past n: untouched
    assert np.array_equal(l[n:].cpu().numpy(), logit[n:], equal_nan=True)


def test_empty_problem_through_the_c_abi(dev):
    from dream_gnn_amd import _lib

    count = torch.full((1,), 77, dtype=torch.int64, device=dev)
    info = torch.full((2,), 77, dtype=torch.int32, device=dev)
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    for n_drug, n_dis in ((0, 5), (5, 0)):
        count.fill_(77)
        rc = _lib.lib.dgmi_pair_mlp_emit_f32(None, 128, n_drug, None, 128, n_dis, 128, 64, None, None, None, None, None, None,
                                             0, 0.0, 0, None, None, None, count.data_ptr(), info.data_ptr(), None, 0, stream)
        assert rc == 0 and int(count) == 0 and info.tolist() == [0, 0]
    dec = R.designed_decoder(*R.dead(1, 1, 0.5)[2:]).to(dev)
    with torch.no_grad():
        drug, dis, logit = dec.pairs_above(torch.zeros(0, 128, device=dev), torch.zeros(4, 128, device=dev), NAN)
        assert drug.numel() == dis.numel() == logit.numel() == 0
        assert dec.count_pairs_above(torch.zeros(3, 128, device=dev), torch.zeros(0, 128, device=dev), NAN) == 0


# ---------------------------------------------------------------------------------------------
# (d) known pairs
# ---------------------------------------------------------------------------------------------
def test_known_pairs(dev):
    from dream_gnn_amd import ops

    shape = (67, 70)
    design, table, sparse = _levels(shape)
    row, col = np.zeros(shape, dtype=bool), np.zeros(shape, dtype=bool)
    row[[0, 40, 66], :] = True               # fully known drugs
    col[:, [0, 31, 32, 69]] = True           # fully known diseases
    for name, known in (("duplicates", sparse), ("rows", row), ("columns", col), ("both", row | col | sparse),
                        ("everything", np.ones(shape, dtype=bool))):
        _check(dev, design, table, known, [NAN, 0.0, 3.0], "known " + name)  # _known_lists lists a tenth twice
    P, Q, *params = (t.to(dev) for t in design)
    empty = torch.zeros(0, dtype=torch.int32, device=dev)
    exp = _expected_above(table, None, 2.0)
    R.assert_pairs_equal(ops.pair_mlp_above(P, Q, *params, empty, empty, 2.0)[:3], exp, "empty known list")
    R.assert_pairs_equal(ops.pair_mlp_above(P, Q, *params, None, None, 2.0)[:3], exp, "no known list")
    for kd, ks in (([1, 67], [0, 0]), ([1, 2], [0, -1]), ([2 ** 33, 0], [0, 0]), ([0], [70])):
        kd, ks = torch.tensor(kd, device=dev), torch.tensor(ks, device=dev)
        with pytest.raises(RuntimeError, match="outside"):
            ops.pair_mlp_above(P, Q, *params, kd, ks, 0.0)
        with pytest.raises(RuntimeError, match="outside"):
            ops.pair_mlp_count_above(P, Q, *params, kd, ks, 0.0)


# ---------------------------------------------------------------------------------------------
# (e) the same bits as the on-chip top-k, on a random decoder
# ---------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def randn300(dev):
    """A random decoder at 300 x 200 with 2 % known and its on-chip top-1024; no test writes to it."""
    dec = TP._decoder(dev, 3)
    g = torch.Generator(device=dev).manual_seed(13)
    hd, hs = torch.randn(300, 128, device=dev, generator=g), torch.randn(200, 128, device=dev, generator=g)
    mask = torch.rand(300, 200, device=dev, generator=g) < 0.02
    known = mask.nonzero(as_tuple=True)
    with torch.no_grad():
        top = dec.top_pairs(hd, hs, 1024, known)
        P, Q = TP._PQ(dec, hd, hs)
        L, T = TP._all64(P, Q, dec)
    return dict(dec=dec, hd=hd, hs=hs, mask=mask, known=known, top=top, L=L, T=T)


def test_same_bits_as_the_on_chip_topk(randn300):
    c = randn300
    dec, hd, hs, known, top = c["dec"], c["hd"], c["hs"], c["known"], c["top"]
    with torch.no_grad():
        deep = dec.top_pairs_deep(hd, hs, 5000, known)
        assert deep[0].numel() == 5000
        for x, y in zip(deep, top):
            assert torch.equal(x[:1024], y)
        assert torch.equal(deep[2][:1024].view(torch.int32), top[2].view(torch.int32))
        for k in (1, 200, 1024):
            for x, y in zip(dec.top_pairs_deep(hd, hs, k, known), dec.top_pairs(hd, hs, k, known)):
                assert torch.equal(x, y)
        above = dec.pairs_above(hd, hs, float(top[2][-1]), known)
        assert above[0].numel() >= 1024
        for x, y in zip(above, top):
            assert torch.equal(x[:1024], y)
        assert bool((above[2] >= top[2][-1]).all())
    TP._assert_ordered(*deep)


def test_random_decoder_against_fp64(randn300):
    """The set / tolerance rule of test_gpu_pairs.py at a cut: every pair whose fp64 logit clears the cut by more than
    its tolerance is listed, none that misses it by more than its tolerance is, and the listed logits are within
    tolerance."""
    c = randn300
    dec, L, T, mask = c["dec"], c["L"], c["T"], c["mask"]
    flat, tol, known = L.reshape(-1), T.reshape(-1), mask.reshape(-1)
    for q in (0.999, 0.9, 0.5):
        cut = float(np.float32(torch.quantile(flat[~known], q).item()))
        with torch.no_grad():
            drug, dis, logit = dec.pairs_above(c["hd"], c["hs"], cut, c["known"])
            n = dec.count_pairs_above(c["hd"], c["hs"], cut, c["known"])
        assert n == drug.numel()
        got = drug * 200 + dis
        assert torch.unique(got).numel() == got.numel() and not bool(known[got].any())
        listed = torch.zeros_like(known)
        listed[got] = True
        must = ~known & (flat > cut + tol)
        must_not = known | (flat < cut - tol)
        assert bool(listed[must].all()), "a pair above the cut by more than its tolerance is missing"
        assert not bool(listed[must_not].any()), "a pair below the cut by more than its tolerance is listed"
        assert bool(((logit.double() - flat[got]).abs() <= tol[got]).all())
        assert bool((logit >= cut).all())
        TP._assert_ordered(drug, dis, logit)
        assert int(must.sum()) > 0.5 * (1 - q) * int((~known).sum())  # the cut is where it was meant to be


# ---------------------------------------------------------------------------------------------
# (f) deep k, exact
# ---------------------------------------------------------------------------------------------
def _deep(dev, design, known, k):
    dec = R.designed_decoder(*design[2:]).to(dev)
    kd, ks = _known_lists(known, dev)
    with torch.no_grad():
        return dec.top_pairs_deep(design[0].to(dev), design[1].to(dev), k, None if kd is None else (kd, ks))


def test_deep_k_exact(dev):
    shape = (300, 200)
    rng = np.random.default_rng(51)
    known = rng.random(shape) < 0.02
    n_novel = int((~known).sum())
    a, c = rng.integers(-2000, 2000, 300), rng.integers(-2000, 2000, 200)
    cases = {"few levels": _levels(shape, seed=52, with_known=False)[:2],
             "many levels": (R.additive(a, c, b3=0.5), R.additive_table(a, c, 0.5)),
             "one tie class": (R.dead(*shape, B3), R.dead_table(*shape, B3))}
    for name, (design, table) in cases.items():
        full = R.expected_pairs(table, known, n_novel)
        for k in (1025, 5000, n_novel, n_novel + 10):
            R.assert_pairs_equal(_deep(dev, design, known, k), R.cut_pairs(full, k), "deep %s k=%d" % (name, k))
    design, table = cases["many levels"]
    R.assert_pairs_equal(_deep(dev, design, None, 60_000), R.expected_pairs(table, None, 60_000), "deep, every pair")


@pytest.mark.parametrize("where", ["sampled", "skipped"])
@pytest.mark.parametrize("k", [1025, 5000])
def test_deep_k_when_the_sample_misleads(dev, k, where):
    """The large logits sit only in the drug rows the stride samples (the estimated cut is far too high, the first pass
    returns fewer than k pairs and the cut is lowered) or only in the rows it skips (the cut is far too low, the pass
    lists most of the table): the answer is exact either way."""
    shape = (300, 200)
    s = -(-k // 512)
    rng = np.random.default_rng(61)
    in_sample = np.arange(300) % s == 0
    a = rng.integers(0, 50, 300) + 5000 * (in_sample if where == "sampled" else ~in_sample)
    c = rng.integers(0, 50, 200)
    known = rng.random(shape) < 0.02
    design, table = R.additive(a, c), R.additive_table(a, c)
    exp = R.expected_pairs(table, known, k)
    if where == "sampled":  # the premise: the sampled cut leaves fewer than k pairs
        r = -(-3 * k // (2 * s)) + 32
        cut = np.sort(table[in_sample].ravel())[::-1][r - 1]
        assert int((~known & (table >= cut)).sum()) < k
    R.assert_pairs_equal(_deep(dev, design, known, k), exp, "deep k=%d, large logits in the %s rows" % (k, where))


def test_deep_k_overflow_raises_with_the_exact_count(dev):
    """One tie class of 2 000 x 1 000 pairs under a small k: the cut is that value, every pair reaches it."""
    from dream_gnn_amd import ops

    design = R.dead(2000, 1000, B3)
    with pytest.raises(ops.TooManyPairs) as e:
        _deep(dev, design, None, 1025)
    assert e.value.count == 2_000_000 and e.value.max_pairs == 4 * 1025 + 65536


# ---------------------------------------------------------------------------------------------
# (g) the reference's own get_top_novel_predictions beyond 1024 rows
# ---------------------------------------------------------------------------------------------
def _fixture_net(g, dev):
    from dream_gnn_amd import model as M

    nd, ns, emb = int(g["n_drug"]), int(g["n_dis"]), int(g["emb"])
    args = types.SimpleNamespace(rating_vals=[0, 1], src_in_units=emb, dst_in_units=emb, gcn_agg_units=int(g["agg_units"]),
                                 gcn_out_units=int(g["out_units"]), dropout=0.0, gcn_agg_accum="sum",
                                 model_activation="leaky", share_param=True, device=None, layers=int(g["layers"]),
                                 fdim_drug=nd, fdim_disease=ns, nhid1=int(g["nhid1"]), nhid2=int(g["out_units"]),
                                 attention_dropout=0.0)
    net = M.Net(args)
    sd = {key[3:]: torch.from_numpy(g[key]) for key in g.files if key.startswith("sd_")}
    res = net.load_state_dict(sd, strict=True)
    assert not res.missing_keys and not res.unexpected_keys
    return net.to(dev).train()


def test_matches_the_reference_at_top_k_1500(dev):
    from dream_gnn_amd import predict

    g = np.load(os.path.join(TP.GOLD, "novel_deep1500.npz"))
    k, ns = int(g["k"]), int(g["n_dis"])
    assert k == 1500
    net = _fixture_net(g, dev)
    out = predict.top_novel_pairs_deep(net, TP._fixture_batch(g, dev), g["association"], k=k)
    assert net.training and len(out) == k
    TP._assert_ordered(out.drug_id, out.disease_id, out.logit)
    assert not g["association"][out.drug_id.numpy(), out.disease_id.numpy()].any()
    ref_score = {int(d) * ns + int(s): float(v) for d, s, v in zip(g["ref_drug_id"], g["ref_disease_id"], g["ref_score"])}
    nxt_score = {int(d) * ns + int(s): float(v) for d, s, v in
                 zip(g["ref_next_drug_id"], g["ref_next_disease_id"], g["ref_next_score"])}
    mine = {int(d) * ns + int(s): float(v) for d, s, v in zip(out.drug_id, out.disease_id, out.score.double())}
    assert len(mine) == k and len(ref_score) == k
    shared = set(mine) & set(ref_score)
    worst = max(abs(mine[p] - ref_score[p]) for p in shared)
    kth = float(g["ref_score"][-1])
    only_mine, only_ref = set(mine) - set(ref_score), set(ref_score) - set(mine)
    print("shared %d, worst score difference %.3e, only here %d, only in the reference %d"
          % (len(shared), worst, len(only_mine), len(only_ref)))
    assert worst <= 1e-5
    assert len(only_mine) == len(only_ref) and len(only_mine) + len(only_ref) <= 8
    for p in only_ref:
        assert abs(ref_score[p] - kth) <= 2e-5, p
    for p in only_mine:  # a pair just outside the reference's list: among its next rows, within the band
        assert p in nxt_score and abs(nxt_score[p] - kth) <= 2e-5, p


def test_deep_k_returns_every_pair_of_novel_all(dev):
    from dream_gnn_amd import predict

    g = np.load(os.path.join(TP.GOLD, "novel_all.npz"))
    net = _fixture_net(g, dev)
    batch = TP._fixture_batch(g, dev)
    out = predict.top_novel_pairs_deep(net, batch, g["association"], k=2000)
    assert len(out) == len(g["ref_drug_id"]) == int((g["association"] == 0).sum())
    assert np.array_equal(out.drug_id.numpy(), g["ref_drug_id"]) and np.array_equal(out.disease_id.numpy(), g["ref_disease_id"])
    assert np.abs(out.score.numpy().astype(np.float64) - g["ref_score"]).max() <= 1e-5
    # by score: the rows of the reference at or above 0.5, and their number
    top = predict.top_novel_pairs(net, batch, g["association"], k=200)
    above = predict.novel_pairs_above(net, batch, g["association"], min_score=0.5)
    n = int((top.logit >= 0).sum())
    assert 0 < n < len(top) and len(above) == n
    assert predict.count_novel_pairs_above(net, batch, g["association"], min_score=0.5) == n
    for x, y in ((above.drug_id, top.drug_id), (above.disease_id, top.disease_id), (above.logit, top.logit), (above.score, top.score)):
        assert torch.equal(x, y[:n])
    assert abs(n - int((g["ref_score"] >= 0.5).sum())) <= int((np.abs(g["ref_score"] - 0.5) <= 1e-5).sum())
    everything = predict.novel_pairs_above(net, batch, g["association"], min_logit=NAN)
    assert torch.equal(everything.drug_id, top.drug_id) and torch.equal(everything.logit, top.logit)
    with pytest.raises(predict.ops.TooManyPairs) as e:
        predict.novel_pairs_above(net, batch, g["association"], min_logit=NAN, max_pairs=5)
    assert e.value.count == len(top) and net.training


# ---------------------------------------------------------------------------------------------
# (h) determinism, streams, flags
# ---------------------------------------------------------------------------------------------
def test_deterministic_and_any_stream(dev):
    dec = TP._decoder(dev, 4)
    hd, hs = torch.randn(3000, 128, device=dev), torch.randn(2000, 128, device=dev)
    kd, ks = torch.randint(0, 3000, (60000,), device=dev), torch.randint(0, 2000, (60000,), device=dev)
    with torch.no_grad():
        cut = float(dec.top_pairs(hd, hs, 1024, (kd, ks))[2][-1]) - 0.05
        runs = []
        for fn in (lambda: dec.pairs_above(hd, hs, cut, (kd, ks)), lambda: dec.top_pairs_deep(hd, hs, 20_000, (kd, ks))):
            a, b = fn(), fn()
            s = torch.cuda.Stream()
            s.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(s):
                c = fn()
            torch.cuda.current_stream().wait_stream(s)
            runs.append((a, b, c))
    for a, b, c in runs:
        assert a[0].numel() > 1024
        for x, y, z in zip(a, b, c):
            assert torch.equal(x, y) and torch.equal(x, z)
        assert torch.equal(a[2].view(torch.int32), b[2].view(torch.int32))
        TP._assert_ordered(*(t[:3000] for t in a))


def test_predict_restores_the_training_flag_and_leaves_no_gradient(dev):
    from dream_gnn_amd import predict

    g = np.load(os.path.join(TP.GOLD, "novel_all.npz"))
    batch = TP._fixture_batch(g, dev)
    for training in (True, False):
        net = _fixture_net(g, dev).train(training)
        out = predict.novel_pairs_above(net, batch, g["association"], min_logit=-1.0)
        assert net.training == training and len(out) > 0
        assert predict.count_novel_pairs_above(net, batch, g["association"], min_logit=-1.0) == len(out)
        assert net.training == training
        assert len(predict.top_novel_pairs_deep(net, batch, g["association"], k=1025)) == int((g["association"] == 0).sum())
        assert net.training == training
        assert all(p.grad is None for p in net.parameters())
        assert not out.logit.requires_grad and out.logit.device.type == "cpu" and out.drug_id.dtype == torch.int64
        assert torch.equal(out.score, torch.sigmoid(out.logit))
