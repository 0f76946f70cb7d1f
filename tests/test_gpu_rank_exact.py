"""The exact order of the two ranking kernels (csrc/dgmi_pairs.hip -> ops.pair_mlp_topk, csrc/dgmi_pairs_rows.hip ->
ops.pair_mlp_row_topk) on designed decoders (tests/_rank_cases.py): every logit is an exactly representable function of
two integer vectors, the expected answer is integer arithmetic plus a lexsort on the host, and the kernels must return
exactly those ids, in exactly that order, with exactly those logit bits, counts and padding.  Zero tolerance: every
comparison is equality (zero logits by value: the kernels return +0.0 for either sign, and no case rests on the sign).
The one tolerance in this file is the project's fp64 rule (REL = 1e-6) of test_gpu_rank.py, used unchanged for the
randn decoder of the two-merge-round cases.

What random logits never reach, and these cases do: exact tie classes (also at the k-th boundary), the append buffers
held at their stated maximum for a whole run (every offered pair beats the threshold), the second merge round of the
per-row kernel, k next to powers of two, +-inf logits and NaN next to ties, strided and misaligned operands.

tests/test_rank_cases_host.py holds the designs and the expected order to the same zero tolerance without a GPU."""
import functools

import numpy as np
import pytest
import torch

import _rank_cases as R
import test_gpu_rank as TR

pytestmark = pytest.mark.gpu

GLOBAL_KS = (1, 2, 3, 127, 128, 129, 511, 512, 513, 1000, 1023, 1024)
ROW_KS = (1, 2, 3, 31, 32, 33, 63, 64, 65, 127, 128)
FEW_GLOBAL_KS = (1, 129, 1024)
FEW_ROW_KS = (1, 33, 128)
BOTH = ("disease", "drug")

# carrying columns / hidden units of the additive design: both 64-column halves and both 32-row halves (where the MFMA
# operand layout splits), and one pair that shares an MFMA step (k and k + 64); b3 = 0 keeps zero logits in play
LAYOUTS = (dict(k0=0, k1=127, h0=0, h1=63, b3=0.0), dict(k0=63, k1=64, h0=31, h1=32, b3=0.25),
           dict(k0=69, k1=5, h0=40, h1=17, b3=-3.0))


def _known_lists(known, dev, seed=0):
    """A bool mask as the (drug ids, disease ids) the ops take: shuffled, with a tenth of it listed twice."""
    if known is None:
        return None, None
    kd, ks = np.nonzero(known)
    rng = np.random.default_rng(seed)
    n = kd.size
    idx = rng.permutation(np.concatenate([np.arange(n), rng.integers(0, n, n // 10)])) if n else np.arange(0)
    return torch.from_numpy(kd[idx]).to(dev), torch.from_numpy(ks[idx]).to(dev)


def _check(dev, design, table, known=None, global_ks=GLOBAL_KS, row_ks=ROW_KS, by=BOTH, what=""):
    """Both kernels (the per-row one in the directions ``by``) at every k against the host order of ``table``
    (n_drug x n_dis float32) without the pairs of the bool mask ``known``."""
    from dream_gnn_amd import ops

    P, Q, *params = (t.to(dev) for t in design)
    kd, ks = _known_lists(known, dev)
    if global_ks:
        full = R.expected_pairs(table, known, max(global_ks))
        for k in global_ks:
            got = ops.pair_mlp_topk(P, Q, *params, kd, ks, k)
            R.assert_pairs_equal(got, R.cut_pairs(full, k), "%s global k=%d" % (what, k))
    for direction in by if row_ks else ():
        if direction == "disease":
            X, C, kq, kc, T, M = Q, P, ks, kd, np.ascontiguousarray(table.T), None if known is None else known.T
        else:
            X, C, kq, kc, T, M = P, Q, kd, ks, table, known
        full = R.expected_rows(T, M, max(row_ks))
        for k in row_ks:
            got = ops.pair_mlp_row_topk(X, C, *params, kq, kc, k)
            R.assert_rows_equal(got, R.cut_rows(full, k), "%s per %s k=%d" % (what, direction, k))


# ---------------------------------------------------------------------------------------------
# (a) one tie class: the answer is the first k novel pairs / candidates in id order
# ---------------------------------------------------------------------------------------------
B3 = float(np.float32(0.37))


@pytest.mark.parametrize("n_dis", [1, 31, 32, 33, 127, 128, 129, 681])
def test_one_tie_class(dev, n_dis):
    for n_drug in (1, 2, 63, 64, 65, 763):
        table = R.dead_table(n_drug, n_dis, B3)
        _check(dev, R.dead(n_drug, n_dis, B3), table, None, FEW_GLOBAL_KS, FEW_ROW_KS, what="dead %dx%d" % (n_drug, n_dis))
        if n_drug * n_dis >= 1024:  # the definition, spelled out once more: the first k pairs in id order
            e = R.expected_pairs(table, None, 1024)
            flat = np.arange(1024)
            assert np.array_equal(e.drug, flat // n_dis) and np.array_equal(e.dis, flat % n_dis)


def _mask(kind, n_drug, n_dis):
    i, j = np.arange(n_drug)[:, None], np.arange(n_dis)[None, :]
    m = np.zeros((n_drug, n_dis), dtype=bool)
    if kind == "word_edges":  # the bitmap words run along diseases in one direction and along drugs in the other
        edge_j = np.isin(j, [0, 31, 32, 63, 64, n_dis - 1])
        edge_i = np.isin(i, [0, 31, 32, 63, 64, n_drug - 1])
        m = (edge_j & (i % 3 == 0)) | (edge_i & (j % 3 == 1))
    elif kind == "rows":
        m[[0, 5, n_drug - 1], :] = True
    elif kind == "columns":
        m[:, [0, 32, n_dis - 1]] = True
    elif kind == "checkerboard":
        m = (i + j) % 2 == 0
    elif kind == "everything":
        m[:] = True
    elif kind == "all_but_the_last":
        m[:] = True
        m[n_drug - 1, n_dis - 1] = False
    return np.ascontiguousarray(m)


@pytest.mark.parametrize("kind", ["word_edges", "rows", "columns", "checkerboard", "everything", "all_but_the_last"])
@pytest.mark.parametrize("shape", [(65, 129), (64, 33), (763, 681)])
def test_one_tie_class_with_known_pairs(dev, shape, kind):
    n_drug, n_dis = shape
    known = _mask(kind, n_drug, n_dis)
    _check(dev, R.dead(n_drug, n_dis, B3), R.dead_table(n_drug, n_dis, B3), known, FEW_GLOBAL_KS, FEW_ROW_KS,
           what="dead %dx%d %s" % (n_drug, n_dis, kind))


# ---------------------------------------------------------------------------------------------
# (b) few levels: k cuts through a tie class of thousands of pairs; (d) the k sweep
# ---------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _few_levels(shape, layout, with_known, seed=3):
    """(design, table, known mask or None); shared by several tests, none of which writes to it."""
    n_drug, n_dis = shape
    rng = np.random.default_rng(seed)
    a, c = rng.integers(-2, 3, n_drug), rng.integers(0, 3, n_dis)  # 5 x 3 levels
    lay = dict(LAYOUTS[layout])
    known = (rng.random(shape) < 0.01) if with_known else None
    return R.additive(a, c, **lay), R.additive_table(a, c, lay["b3"]), known


FEW_LEVEL_CASES = [((763, 681), 0), ((763, 681), 1), ((763, 681), 2), ((4001, 4003), 1)]


@pytest.mark.parametrize("with_known", [False, True])
@pytest.mark.parametrize("shape,layout", FEW_LEVEL_CASES)
def test_few_levels(dev, shape, layout, with_known):
    design, table, known = _few_levels(shape, layout, with_known)
    _check(dev, design, table, known, what="levels %dx%d" % shape)


# ---------------------------------------------------------------------------------------------
# (c) arrival order: every offered pair beats the threshold (ascending), none after the first k (descending), and a
# sawtooth; (d) the k sweep
# ---------------------------------------------------------------------------------------------
def _arrival(kind, shape, layout):
    n_drug, n_dis = shape
    i, j = np.arange(n_drug), np.arange(n_dis)
    if kind == "ascending":    # logit = the pair's flat index: the last k pairs / the last k candidates of each row
        a, c = i * n_dis, j
    elif kind == "descending":
        a, c = -i * n_dis, -j
    else:                      # sawtooth: drugs i and i + 64 tie, the ramp restarts with every 64-drug chunk
        a, c = (i % 64) * n_dis, j
    lay = dict(LAYOUTS[layout], b3=0.0)
    assert n_drug * n_dis < 2 ** 24
    return R.additive(a, c, **lay), R.additive_table(a, c)


# 4001 x 4003: below 2**24 pairs, and big enough for 64-drug chunks and the full 256-workgroup grid
@pytest.mark.parametrize("shape,layout,kind", [((763, 681), 1, "ascending"), ((763, 681), 1, "descending"),
                                               ((763, 681), 1, "sawtooth"), ((4001, 4003), 0, "ascending"),
                                               ((4001, 4003), 2, "descending"), ((4001, 4003), 2, "sawtooth")])
def test_arrival_order(dev, shape, layout, kind):
    design, table = _arrival(kind, shape, layout)
    if kind == "ascending":
        e = R.expected_pairs(table, None, 5)
        last = shape[0] * shape[1] - 1
        assert (e.drug * shape[1] + e.dis).tolist() == [last - r for r in range(5)]
    _check(dev, design, table, None, what="%s %dx%d" % ((kind,) + shape))


def test_arrival_order_with_known_pairs(dev):
    shape = (4001, 4003)
    design, table = _arrival("ascending", shape, 1)
    known = np.random.default_rng(4).random(shape) < 0.01
    known[-3:, :] = True  # the three best drugs are known everywhere
    _check(dev, design, table, known, FEW_GLOBAL_KS + (513,), FEW_ROW_KS + (65,), what="ascending with known")


# ---------------------------------------------------------------------------------------------
# (e) per-row merge rounds: few queries against many candidates, n_seg > fan
# ---------------------------------------------------------------------------------------------
def _assert_two_rounds(n_query, n_cand, k):
    """Host arithmetic: the call really takes a second merge round, and the library's workspace holds the second list
    buffer that goes with it (so these cases cannot quietly stop covering it if the planner changes)."""
    from dream_gnn_amd import _lib

    n_seg, fan, total = R.row_plan(n_query, n_cand, k)
    assert n_seg > fan, "one merge round only: (%d, %d, k=%d) has %d segments, fan %d" % (n_query, n_cand, k, n_seg, fan)
    assert _lib.lib.dgmi_row_topk_workspace_bytes(n_query, n_cand, k) == total


def _many_candidates(kind, n_query, n_cand, seed=5):
    """(query vector, candidate vector) of an additive design."""
    rng = np.random.default_rng(seed)
    if kind == "levels":
        return rng.integers(0, 3, n_query), rng.integers(-2, 3, n_cand)
    if kind == "ascending":
        return np.arange(n_query) * n_cand, np.arange(n_cand)
    if kind == "descending":
        return -np.arange(n_query) * n_cand, -np.arange(n_cand)
    return rng.integers(0, 3, n_query), np.arange(n_cand) % 4096  # sawtooth: ties across segments


@pytest.mark.parametrize("k", [65, 128])
@pytest.mark.parametrize("n_cand", [8193, 20_011, 100_000])
@pytest.mark.parametrize("n_query", [1, 33])
def test_two_merge_rounds(dev, n_query, n_cand, k):
    _assert_two_rounds(n_query, n_cand, k)
    for n, kind in enumerate(("levels", "ascending", "descending", "sawtooth")):
        xq, xc = _many_candidates(kind, n_query, n_cand)
        lay = dict(LAYOUTS[n % 3], b3=0.0)
        # queries are diseases (X = Q, C = P), then queries are drugs (X = P, C = Q)
        for by, a, c in (("disease", xc, xq), ("drug", xq, xc)):
            known = None
            if kind == "levels":
                known = np.random.default_rng(6).random((a.size, c.size)) < 0.01
            _check(dev, R.additive(a, c, **lay), R.additive_table(a, c), known, (), (k,), (by,),
                   what="%s %dx%d" % (kind, n_query, n_cand))


@pytest.mark.parametrize("k", [65, 128])
@pytest.mark.parametrize("by", BOTH)
def test_two_merge_rounds_row_subsets_through_the_decoder(dev, by, k):
    n_query, n_cand = 33, 100_000
    xq, xc = _many_candidates("levels", n_query, n_cand, seed=7)
    a, c = (xc, xq) if by == "disease" else (xq, xc)
    P, Q, W2, b2, w3, b3 = R.additive(a, c, **LAYOUTS[1])
    table = R.additive_table(a, c, LAYOUTS[1]["b3"])
    known = np.random.default_rng(8).random(table.shape) < 0.01
    T, M = (np.ascontiguousarray(table.T), known.T) if by == "disease" else (table, known)
    full = R.expected_rows(T, M, k)
    dec = R.designed_decoder(W2, b2, w3, b3).to(dev)
    hd, hs = P.to(dev), Q.to(dev)
    kd, ks = _known_lists(known, dev)
    for rows in (None, [5, 0, 32], [17]):
        _assert_two_rounds(n_query if rows is None else len(rows), n_cand, k)
        with torch.no_grad():
            qid, cand, logit, count = dec.top_pairs_per_row(hd, hs, k, by=by, known=(kd, ks), rows=rows)
        sel = np.arange(n_query) if rows is None else np.asarray(rows)
        assert qid.tolist() == sel.tolist()
        R.assert_rows_equal((cand, logit, count), R.Rows(full.cand[sel], full.logit[sel], full.count[sel]),
                            "rows=%r per %s" % (rows, by))


@pytest.mark.parametrize("n_query,n_cand,k", [(33, 100_000, 128), (1, 100_000, 65), (33, 20_011, 65)])
def test_two_merge_rounds_randn_against_fp64(dev, n_query, n_cand, k):
    """A randn decoder under the fp64 rule of test_gpu_rank.py, unchanged (REL = 1e-6; set equal up to near-ties of
    the k-th)."""
    _assert_two_rounds(n_query, n_cand, k)
    dec = TR._decoder(dev, 21)
    g = torch.Generator(device=dev).manual_seed(22)
    for by in BOTH:
        nd, ns = (n_cand, n_query) if by == "disease" else (n_query, n_cand)
        hd, hs = torch.randn(nd, 128, device=dev, generator=g), torch.randn(ns, 128, device=dev, generator=g)
        mask = torch.rand(nd, ns, device=dev, generator=g) < 0.01
        kd, ks = mask.nonzero(as_tuple=True)
        with torch.no_grad():
            P, Q = TR._PQ(dec, hd, hs)
        X, C, M = (Q, P, mask.t()) if by == "disease" else (P, Q, mask)
        _, cand, logit, count = TR._rows(dec, hd, hs, k, by, (kd, ks))
        assert cand.shape == (n_query, k)
        for q in range(n_query):
            L, T = TR._row64(X, C, dec, q)
            TR._assert_row(cand[q], logit[q], count[q], L, T, M[q], k)


# ---------------------------------------------------------------------------------------------
# (f) specials: +inf on top of a tie class, -inf below one, NaN last and ordered by id, padding after
# ---------------------------------------------------------------------------------------------
SPECIAL_SHAPES = [(33, 31),    # 1023 pairs: k = 1024 returns everything
                  (40, 30),    # 999 numbers: k = 1000 and 1024 cut inside the NaN block
                  (150, 100),  # per drug k = 128 > 100 candidates: the NaN block and the padding of every row
                  (300, 257)]


@pytest.mark.parametrize("b3", [0.5, 0.0])
@pytest.mark.parametrize("sign", [1, -1])
@pytest.mark.parametrize("shape", SPECIAL_SHAPES)
def test_inf_and_nan_next_to_ties(dev, shape, sign, b3):
    n_drug, n_dis = shape
    rng = np.random.default_rng(9)
    a, c = rng.integers(-3, 4, n_drug).astype(np.float64), rng.integers(-1, 3, n_dis).astype(np.float64)
    a[[3, n_drug - 2]] = np.inf  # a block of sign * inf pairs: two whole drugs and one whole disease
    c[5] = np.inf
    a[[10, 11, n_drug - 1]] = np.nan
    c[[0, 20, n_dis - 1]] = np.nan
    table = R.uniform_table(a, c, sign, b3)
    assert np.isinf(table).any() and np.isnan(table).sum() == 3 * n_dis + 3 * n_drug - 9
    for known in (None, rng.random(shape) < 0.1):
        if shape == (40, 30) and known is None:
            e = R.expected_pairs(table, None, 1024)
            assert not np.isnan(e.logit[:999]).any() and np.isnan(e.logit[999:]).all() and e.logit.size == 1024
            assert np.isinf(e.logit[0 if sign > 0 else 998])
        k0 = 0 if known is None else 100  # the carrying column: one in each 64-column half
        _check(dev, R.uniform(a, c, sign, k0=k0, b3=b3), table, known, FEW_GLOBAL_KS + (1000,), FEW_ROW_KS,
               what="uniform %+d %dx%d" % ((sign,) + shape))


# ---------------------------------------------------------------------------------------------
# (g) the two kernels agree under ties: the global top-1024 regrouped by row is the head of each row's list, with the
# k-th key inside a tie class (test_gpu_rank.py's _cross_check, unchanged)
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("with_known", [False, True])
@pytest.mark.parametrize("shape,layout", FEW_LEVEL_CASES)
def test_kernels_agree_under_ties(dev, shape, layout, with_known):
    (P, Q, W2, b2, w3, b3), table, known = _few_levels(shape, layout, with_known)
    e = R.expected_pairs(table, known, 1025)
    assert e.logit[1023] == e.logit[1024], "the 1024-th key is not inside a tie class"
    dec = R.designed_decoder(W2, b2, w3, b3).to(dev)
    TR._cross_check(dec, P.to(dev), Q.to(dev), *_known_lists(known, dev))


# ---------------------------------------------------------------------------------------------
# (h) strided and offset operands
# ---------------------------------------------------------------------------------------------
def _views(t, kind):
    n = t.shape[0]
    if kind == "wide":        # leading dimension 256, 16-byte aligned rows
        big = torch.full((n, 256), 7.0, device=t.device)
        v = big[:, :128]
    elif kind == "wide_offset":  # leading dimension 384, starting 512 bytes into the row
        big = torch.full((n, 384), 7.0, device=t.device)
        v = big[:, 128:256]
    elif kind == "off_by_4_bytes":  # first element 4 bytes past a 16-byte boundary
        big = torch.full((n, 256), 7.0, device=t.device)
        v = big[:, 1:129]
    else:                     # "odd_stride": leading dimension 129: most rows start off a 16-byte boundary
        big = torch.full((n, 129), 7.0, device=t.device)
        v = big[:, :128]
    v.copy_(t)
    assert v.stride(1) == 1 and not (n > 1 and v.is_contiguous())
    return v


@pytest.mark.parametrize("kind", ["wide", "wide_offset", "off_by_4_bytes", "odd_stride"])
@pytest.mark.parametrize("shape", [(763, 681), (1, 200), (200, 1)])
def test_strided_and_offset_operands(dev, shape, kind):
    from dream_gnn_amd import ops

    design, table, known = _few_levels(shape, 1, True)
    P, Q, *params = (t.to(dev) for t in design)
    kd, ks = _known_lists(known, dev)
    Pv, Qv = _views(P, kind), _views(Q, kind)
    want = ops.pair_mlp_topk(P, Q, *params, kd, ks, 513)
    R.assert_pairs_equal(want, R.expected_pairs(table, known, 513), kind)
    for p, q in ((Pv, Qv), (Pv, Q), (P, Qv)):
        got = ops.pair_mlp_topk(p, q, *params, kd, ks, 513)
        assert all(torch.equal(x, y) for x, y in zip(got[:2], want[:2]))
        assert torch.equal(got[2].view(torch.int32), want[2].view(torch.int32))
    for (X, C, Xv, Cv, kq, kc, T, M) in ((Q, P, Qv, Pv, ks, kd, np.ascontiguousarray(table.T), known.T),
                                         (P, Q, Pv, Qv, kd, ks, table, known)):
        want = ops.pair_mlp_row_topk(X, C, *params, kq, kc, 65)
        R.assert_rows_equal(want, R.expected_rows(T, M, 65), kind)
        for x, c in ((Xv, Cv), (Xv, C), (X, Cv)):
            got = ops.pair_mlp_row_topk(x, c, *params, kq, kc, 65)
            assert torch.equal(got[0], want[0]) and torch.equal(got[2], want[2])
            assert torch.equal(got[1].view(torch.int32), want[1].view(torch.int32))
