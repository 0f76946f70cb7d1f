"""Scoring and ranking GIVEN pairs on the MI355X (csrc/dgmi_pairs_given.hip -> ops.pair_mlp_score_list /
pair_mlp_rank_list -> MLPDecoder.score_pairs / rank_pairs -> predict.score_pairs / rank_pairs).

(a) the list scorer returns the bits the ranking kernels return for the pair; (b) exact ranks on designed decoders
(tests/_rank_cases.py) against the host restatement (tests/_given_cases.py): equality of `above`, `total` and the logit
bits; (c) a rank agrees with the pair's position in the per-row top-k lists; (d) the out-of-range flags; (e) the
reference's own novel-pair lists: scores within 1e-5, and ranks that follow exactly from the lists; (f) predict.rank_pairs
keeps the caller's order and the net's training flag.

Zero tolerance except (e)'s 1e-5 on the score, the bar tests/test_gpu_pairs.py holds top_novel_pairs to."""
import functools
import os
import types

import numpy as np
import pytest
import torch

import _given_cases as GC
import _rank_cases as R

pytestmark = pytest.mark.gpu

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
NAN = float("nan")


def _t(x, dev):
    return torch.from_numpy(np.ascontiguousarray(x)).to(dev)


# ---------------------------------------------------------------------------------------------
# (a) the list scorer: the bits of the ranking kernels, both orientations
# ---------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _random_case(dev):
    """P (70 x 128), Q (45 x 128, a view with leading dimension 132), a random decoder and the (70, 45) table of every
    pair's logit as ops.pair_mlp_above lists it.  Shared; nothing writes to it."""
    from dream_gnn_amd import ops

    g = torch.Generator().manual_seed(11)
    P = torch.randn(70, 128, generator=g).to(dev)
    Q = torch.randn(45, 132, generator=g).to(dev)[:, :128]
    assert Q.stride(0) == 132
    params = tuple(t.to(dev) for t in (torch.randn(64, 128, generator=g) / 8, torch.randn(64, generator=g) / 4,
                                       torch.randn(64, generator=g) / 4, torch.randn(1, generator=g)))
    drug, dis, logit, n = ops.pair_mlp_above(P, Q, *params, None, None, NAN)
    assert n == 70 * 45
    table = np.full((70, 45), np.nan, dtype=np.float32)
    table[drug.cpu().numpy(), dis.cpu().numpy()] = logit.cpu().numpy()
    assert not np.isnan(table).any()
    return P, Q, params, table


def _list(n_pairs, n_a, n_b, seed):
    """n_pairs pairs of an (n_a, n_b) table: a shuffled prefix of all pairs; 3150 + 100: every pair and 100 duplicates."""
    rng = np.random.default_rng(seed)
    flat = rng.permutation(n_a * n_b)
    if n_pairs > flat.size:
        flat = rng.permutation(np.concatenate([flat, rng.integers(0, n_a * n_b, n_pairs - flat.size)]))
    flat = flat[:n_pairs]
    return flat // n_b, flat % n_b


@pytest.mark.parametrize("x_is", ["P", "Q"])
@pytest.mark.parametrize("n_pairs", [0, 1, 31, 32, 33, 64, 65, 3250])
def test_list_scorer_returns_the_ranking_kernels_bits(dev, n_pairs, x_is):
    from dream_gnn_amd import ops

    P, Q, params, table = _random_case(dev)
    drug, dis = _list(n_pairs, 70, 45, n_pairs)
    if n_pairs == 3250:
        assert np.unique(drug * 45 + dis).size == 3150  # every pair, 100 of them twice
    X, C, pq, pc = (P, Q, drug, dis) if x_is == "P" else (Q, P, dis, drug)
    got = ops.pair_mlp_score_list(X, C, *params, _t(pq, dev), _t(pc, dev))
    assert got.shape == (n_pairs,) and got.dtype == torch.float32
    R.assert_same_logits(got.cpu().numpy(), table[drug, dis], "score_list X=%s n=%d" % (x_is, n_pairs))
    # the rank op returns the same logits (int32 ids this time)
    l2, above, total = ops.pair_mlp_rank_list(X, C, *params, _t(pq.astype(np.int32), dev), _t(pc.astype(np.int32), dev))
    assert torch.equal(l2.view(torch.int32), got.view(torch.int32))
    assert above.shape == total.shape == (n_pairs,) and above.dtype == total.dtype == torch.int32


# ---------------------------------------------------------------------------------------------
# (b) exact ranks on designed decoders
# ---------------------------------------------------------------------------------------------
SHAPES = [(1, 1), (3, 31), (33, 127), (40, 128), (37, 129), (5, 300),
          (2, 4100)]  # 40 listed pairs: 2 groups, the candidate axis in 129 segments of 32 (asserted below)
DESIGNS = ["additive", "uniform+", "uniform-", "dead"]
KNOWN = ["none", "random", "full_row", "duplicates", "target"]


@functools.lru_cache(maxsize=None)
def _design(name, shape):
    """(design tensors, (n_query, n_cand) table): the queries are the design's drug side."""
    n_q, n_c = shape
    rng = np.random.default_rng(n_q * 1000 + n_c)
    if name == "additive":  # 5 x 3 levels: most logits tie; b3 = 0 keeps zero logits in play
        a, c = rng.integers(-2, 3, n_q), rng.integers(0, 3, n_c)
        return R.additive(a, c, k0=63, k1=64, h0=31, h1=32, b3=0.0), R.additive_table(a, c, 0.0)
    if name == "dead":
        return R.dead(n_q, n_c, 0.37), R.dead_table(n_q, n_c, np.float32(0.37))
    sign = 1 if name == "uniform+" else -1
    a, c = rng.integers(-3, 4, n_q).astype(np.float64), rng.integers(-1, 3, n_c).astype(np.float64)
    if n_c >= 31:
        c[5] = np.inf                      # a column of sign * inf
        c[[0, 20, n_c - 1]] = np.nan       # NaN columns, first and last candidate included
    if n_q >= 3:
        a[1] = np.inf                      # a whole row of sign * inf (NaN where the column is NaN): one tie class
        a[n_q - 1] = np.nan                # a whole NaN row: ordered by id
    return R.uniform(a, c, sign, k0=100, b3=0.5), R.uniform_table(a, c, sign, 0.5)


def _pairs_and_known(shape, variant):
    """(pair_q, pair_c, known mask or None, known id lists or None) of one case."""
    n_q, n_c = shape
    rng = np.random.default_rng(7 + KNOWN.index(variant))
    if n_q * n_c <= 6000:
        flat = np.arange(n_q * n_c)
        if variant == "target":
            flat = flat[rng.random(flat.size) < 0.34] if flat.size > 1 else flat
        flat = rng.permutation(np.concatenate([flat, rng.choice(flat, min(17, flat.size))]))  # shuffled, some twice
    else:
        flat = rng.integers(0, n_q * n_c, 36)
        flat = rng.permutation(np.concatenate([flat, flat[:4]]))  # 40 listed pairs, 4 of them duplicates
    pq, pc = flat // n_c, flat % n_c
    if variant == "none":
        return pq, pc, None, None
    if variant == "full_row":
        known = np.zeros(shape, dtype=bool)
        known[n_q // 2, :] = True
    else:
        known = rng.random(shape) < 0.3
        if variant == "target":
            known[pq, pc] = True
    kq, kc = np.nonzero(known)
    if variant == "duplicates" and kq.size:
        idx = rng.permutation(np.concatenate([np.arange(kq.size), rng.integers(0, kq.size, kq.size // 2 + 1)]))
        kq, kc = kq[idx], kc[idx]
    return pq, pc, known, (kq, kc)


def test_the_wide_shape_splits_the_candidate_axis():
    n_groups, n_seg, seg, _ = GC.given_plan(2, 4100, 40)
    assert (n_groups, n_seg, seg) == (2, 129, 32)  # a pair's counts are the sum of 129 partial counts
    assert GC.given_plan(40, 128, 40 * 128 + 17)[1] == 4 and GC.given_plan(5, 300, 1517)[1] > 1
    assert GC.given_plan(1, 1, 2)[1] == 1


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%dx%d" % s)
@pytest.mark.parametrize("name", DESIGNS)
def test_exact_ranks_on_designed_decoders(dev, name, shape):
    from dream_gnn_amd import ops

    design, table = _design(name, shape)
    X, C, *params = (t.to(dev) for t in design)
    assert table.shape == shape
    for variant in KNOWN:
        pq, pc, known, lists = _pairs_and_known(shape, variant)
        kq, kc = (None, None) if lists is None else (_t(lists[0], dev), _t(lists[1], dev))
        logit, above, total = ops.pair_mlp_rank_list(X, C, *params, _t(pq, dev), _t(pc, dev), kq, kc)
        e_logit, e_above, e_total = GC.expected_ranks(table, known, pq, pc)
        what = "%s %dx%d known=%s" % ((name,) + shape + (variant,))
        R.assert_same_logits(logit.cpu().numpy(), e_logit, what)
        got_a, got_t = above.cpu().numpy().astype(np.int64), total.cpu().numpy().astype(np.int64)
        assert np.array_equal(got_t, e_total), "%s: total differs at %s" % (what, np.nonzero(got_t != e_total)[0][:5])
        if not np.array_equal(got_a, e_above):
            at = int(np.nonzero(got_a != e_above)[0][0])
            raise AssertionError("%s: pair %d = (%d, %d) has above %d, expected %d of %d"
                                 % (what, at, pq[at], pc[at], got_a[at], e_above[at], e_total[at]))
        if variant == "full_row":
            row = pq == shape[0] // 2
            assert row.any() and not got_a[row].any() and not got_t[row].any()


@pytest.mark.parametrize("name", ["additive", "uniform-"])
def test_exact_ranks_with_segments_longer_than_a_chunk(dev, name):
    """The shapes above give segments of at most 32 candidates.  A long list over a short candidate axis gives few, long
    segments: every pair of a 5 x 333 table 44 times is 2 segments of 167 and 166 candidates, each a full chunk of 128
    (32 per wave) and a second one of 39 or 38 (10 per wave, the last wave 9 or 8).  The expected answer is computed
    once per distinct pair."""
    from dream_gnn_amd import ops

    shape = (5, 333)
    assert GC.given_plan(5, 333, 44 * 5 * 333)[1:3] == (2, 167)
    design, table = _design(name, shape)
    X, C, *params = (t.to(dev) for t in design)
    rng = np.random.default_rng(21)
    known = rng.random(shape) < 0.3
    kq, kc = np.nonzero(known)
    uq, uc = np.divmod(np.arange(5 * 333), 333)
    e_logit, e_above, e_total = GC.expected_ranks(table, known, uq, uc)
    flat = rng.permutation(np.tile(np.arange(5 * 333), 44))
    logit, above, total = ops.pair_mlp_rank_list(X, C, *params, _t(flat // 333, dev), _t(flat % 333, dev), _t(kq, dev), _t(kc, dev))
    R.assert_same_logits(logit.cpu().numpy(), e_logit[flat], name)
    assert np.array_equal(total.cpu().numpy(), e_total[flat]) and np.array_equal(above.cpu().numpy(), e_above[flat])


# ---------------------------------------------------------------------------------------------
# (c) a rank is the pair's position in the per-row list
# ---------------------------------------------------------------------------------------------
def test_ranks_agree_with_the_per_row_lists(dev):
    from dream_gnn_amd import ops

    g = torch.Generator().manual_seed(12)
    X, C = torch.randn(50, 128, generator=g).to(dev), torch.randn(200, 128, generator=g).to(dev)
    params = tuple(t.to(dev) for t in (torch.randn(64, 128, generator=g) / 8, torch.randn(64, generator=g) / 4,
                                       torch.randn(64, generator=g) / 4, torch.randn(1, generator=g)))
    known = torch.rand(50, 200, generator=g) < 0.2
    kq, kc = (t.to(dev) for t in known.nonzero(as_tuple=True))
    cand, row_logit, count = ops.pair_mlp_row_topk(X, C, *params, kq, kc, 128)
    cand, row_logit, count = cand.cpu(), row_logit.cpu(), count.cpu().long()
    assert int(count.min()) == 128  # ~160 novel candidates per row: every list is full and leaves some out
    q = torch.arange(50)[:, None].expand(50, 128).reshape(-1)
    r = torch.arange(128)[None, :].expand(50, 128).reshape(-1)
    logit, above, total = ops.pair_mlp_rank_list(X, C, *params, q.to(dev), cand.reshape(-1).to(dev), kq, kc)
    assert torch.equal(above.cpu().long(), r)
    assert torch.equal(logit.cpu().view(torch.int32), row_logit.reshape(-1).view(torch.int32))
    novel = (~known).sum(1)
    assert torch.equal(total.cpu().long(), novel[q] - 1)
    # the novel pairs a row's list leaves out stand behind it
    listed = torch.zeros(50, 200, dtype=torch.bool)
    listed[q, cand.reshape(-1)] = True
    oq, oc = (~known & ~listed).nonzero(as_tuple=True)
    assert oq.numel() == int(novel.sum()) - 50 * 128 > 0
    _, above, total = ops.pair_mlp_rank_list(X, C, *params, oq.to(dev), oc.to(dev), kq, kc)
    assert bool((above.cpu().long() >= count[oq]).all()) and torch.equal(total.cpu().long(), novel[oq] - 1)
    # a row's left-out pairs take the remaining positions, each exactly once (random logits: no ties)
    for row in (0, 49):
        assert sorted(above.cpu()[oq == row].tolist()) == list(range(128, int(novel[row])))


# ---------------------------------------------------------------------------------------------
# (d) flags
# ---------------------------------------------------------------------------------------------
def test_ids_out_of_range_are_flagged_and_never_read(dev):
    from dream_gnn_amd import ops

    P, Q, params, table = _random_case(dev)
    n_q, n_c = 70, 45
    good_q, good_c = [3, 69, 0, 12], [44, 0, 7, 12]
    for bad_q, bad_c in ((-1, 5), (5, -1), (n_q, 0), (0, n_c), (2 ** 33, 1)):
        pq, pc = torch.tensor(good_q[:2] + [bad_q] + good_q[2:], device=dev), torch.tensor(good_c[:2] + [bad_c] + good_c[2:], device=dev)
        with pytest.raises(RuntimeError, match="listed"):
            ops.pair_mlp_score_list(P, Q, *params, pq, pc)
        with pytest.raises(RuntimeError, match="listed"):
            ops.pair_mlp_rank_list(P, Q, *params, pq, pc)
        # the op itself: the in-range pairs still get their results
        b2, w3, b3 = (t.reshape(-1) for t in params[1:])
        logit, above, total, info = torch.ops.dreamgnn_mi.pair_mlp_rank_list(P, Q, params[0], b2, w3, b3, pq, pc, None, None)
        assert info.tolist() == [1, 0]
        e_logit, e_above, e_total = GC.expected_ranks(table, None, good_q, good_c)
        keep = [0, 1, 3, 4]
        R.assert_same_logits(logit.cpu().numpy()[keep], e_logit, "in-range pairs")
        assert above.cpu().numpy()[keep].tolist() == e_above.tolist() and total.cpu().numpy()[keep].tolist() == e_total.tolist()
        assert bool(torch.isnan(logit[2])) and int(above[2]) == -1 and int(total[2]) == -1
        logit, info = torch.ops.dreamgnn_mi.pair_mlp_score_list(P, Q, params[0], b2, w3, b3, pq, pc)
        assert info.tolist() == [1, 0] and bool(torch.isnan(logit[2]))
        R.assert_same_logits(logit.cpu().numpy()[keep], e_logit, "in-range pairs (score_list)")
    # a known id out of range raises, as for the sibling ops
    pq, pc = torch.tensor(good_q, device=dev), torch.tensor(good_c, device=dev)
    for kq, kc in (([1, n_q], [0, 0]), ([1, 2], [0, -1]), ([2 ** 33, 0], [0, 0]), ([0], [n_c])):
        with pytest.raises(RuntimeError, match="known"):
            ops.pair_mlp_rank_list(P, Q, *params, pq, pc, torch.tensor(kq, device=dev), torch.tensor(kc, device=dev))
    # no candidate rows (or no query rows): every listed pair is out of range
    for X, C in ((P, Q[:0]), (P[:0], Q)):
        with pytest.raises(RuntimeError, match="listed"):
            ops.pair_mlp_rank_list(X, C, *params, pq, pc)
        logit, above, total, info = torch.ops.dreamgnn_mi.pair_mlp_rank_list(X, C, params[0], b2, w3, b3, pq, pc, None, None)
        assert info.tolist() == [1, 0] and bool(torch.isnan(logit).all())
        assert above.tolist() == [-1] * 4 and total.tolist() == [-1] * 4


# ---------------------------------------------------------------------------------------------
# (e) the reference's novel-pair lists, (f) predict.rank_pairs
# ---------------------------------------------------------------------------------------------
def _fixture_batch(g, dev):
    from dream_gnn_amd import graph as G

    def sparse(prefix, n):
        idx = torch.from_numpy(np.vstack([g[prefix + "_row"], g[prefix + "_col"]]).astype(np.int64))
        return torch.sparse_coo_tensor(idx, torch.from_numpy(g[prefix + "_val"]), (n, n)).to(dev)

    nd, ns = int(g["n_drug"]), int(g["n_dis"])
    return {"enc_graph": G.build_enc_graph(torch.from_numpy(g["enc_drug"]), torch.from_numpy(g["enc_dis"]),
                                           torch.from_numpy(g["enc_values"]), nd, ns, symm=True, device=dev).int(),
            "drug_graph": sparse("drug_graph", nd), "disease_graph": sparse("dis_graph", ns),
            "drug_feature_graph": sparse("drug_fg", nd), "disease_feature_graph": sparse("dis_fg", ns),
            "drug_feat": torch.from_numpy(g["drug_feat"]).to(dev), "disease_feat": torch.from_numpy(g["dis_feat"]).to(dev),
            "drug_sim_feat": torch.from_numpy(g["drug_sim"]).to(dev), "disease_sim_feat": torch.from_numpy(g["dis_sim"]).to(dev)}


@functools.lru_cache(maxsize=None)
def _fixture(name, dev):
    """(fixture arrays, net in TRAINING mode on the device, batch) built as in tests/test_gpu_pairs.py."""
    from dream_gnn_amd import model as M

    g = np.load(os.path.join(GOLD, name + ".npz"))
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
    return g, net.to(dev).train(), _fixture_batch(g, dev)


def _position_in_row(row_id):
    """For list entry i: 1 + #{j < i : row_id[j] == row_id[i]}."""
    seen, out = {}, []
    for r in row_id.tolist():
        seen[r] = seen.get(r, 0) + 1
        out.append(seen[r])
    return np.array(out, dtype=np.int64)


@pytest.mark.parametrize("name,per_dis,per_drug", [("novel_top50", 5, 37), ("novel_all", 7, 7)])
def test_the_reference_lists(dev, name, per_dis, per_drug):
    """The reference ranks its novel pairs by score.  Every novel pair of a row that outscores a member of the global
    top-k is itself in the top-k, so a member's rank in its row is its position among the members of that row; the
    fixtures' scores are at least 2.2e-4 apart, 20 times the 1e-5 the scores agree to, so the order is not in doubt."""
    from dream_gnn_amd import predict

    g, net, batch = _fixture(name, dev)
    drug, dis, ref = g["ref_drug_id"], g["ref_disease_id"], g["ref_score"]
    assert (np.diff(ref) <= -2.2e-4).all()  # descending, well separated
    assert np.bincount(dis).max() == per_dis and np.bincount(drug).max() == per_drug  # the ranks are not all 1

    out = predict.score_pairs(net, batch, drug, dis)
    assert net.training  # the flag is restored
    assert np.array_equal(out.drug_id.numpy(), drug) and np.array_equal(out.disease_id.numpy(), dis)  # the caller's order
    assert np.abs(out.score.numpy().astype(np.float64) - ref).max() <= 1e-5
    assert torch.equal(out.score, torch.sigmoid(out.logit))

    assoc = g["association"]
    for by, row_id, axis in (("disease", dis, 0), ("drug", drug, 1)):
        ranks = predict.rank_pairs(net, batch, drug, dis, known=assoc, by=by)
        assert net.training and ranks.by == by and len(ranks) == len(drug)
        assert ranks.rank.dtype == ranks.n_candidates.dtype == torch.int64
        assert np.array_equal(ranks.rank.numpy(), _position_in_row(row_id)), by
        assert torch.equal(ranks.logit.view(torch.int32), out.logit.view(torch.int32))  # one scorer
        if name == "novel_all":  # every novel pair is listed: the list a pair is ranked in is its row's novel pairs
            novel = (assoc == 0).sum(axis)
            assert np.array_equal(ranks.n_candidates.numpy(), novel[row_id]), by
            assert int(ranks.rank.max()) == int(np.bincount(row_id).max())


def test_rank_pairs_keeps_the_callers_order_and_the_training_flag(dev):
    from dream_gnn_amd import predict

    g, net, batch = _fixture("novel_all", dev)
    drug, dis, assoc = g["ref_drug_id"], g["ref_disease_id"], g["association"]
    base = predict.rank_pairs(net, batch, drug, dis, assoc)
    perm = np.random.default_rng(0).permutation(len(drug))
    perm = np.concatenate([perm, perm[:5]])  # and five pairs twice
    for training in (True, False):
        net.train(training)
        got = predict.rank_pairs(net, batch, torch.from_numpy(drug[perm]), dis[perm].tolist(), (assoc != 0).nonzero())
        assert net.training == training
        assert np.array_equal(got.drug_id.numpy(), drug[perm]) and np.array_equal(got.disease_id.numpy(), dis[perm])
        assert torch.equal(got.rank, base.rank[perm]) and torch.equal(got.n_candidates, base.n_candidates[perm])
        assert torch.equal(got.logit.view(torch.int32), base.logit[perm].view(torch.int32))
    net.train(True)
    # known pairs may be listed too (the held-out positive of the filtered protocol): ranked among the row's novel pairs
    kd, ks = (assoc != 0).nonzero()
    held = predict.rank_pairs(net, batch, kd[:20], ks[:20], assoc)
    novel = (assoc == 0).sum(0)
    assert np.array_equal(held.n_candidates.numpy(), novel[ks[:20]] + 1)
    assert bool((held.rank >= 1).all()) and bool((held.rank <= held.n_candidates).all())
    # hits@k and MRR are the ranks' own
    r = base.rank.numpy()
    assert base.hits_at(1) == pytest.approx((r <= 1).mean()) and base.hits_at(3) == pytest.approx((r <= 3).mean())
    assert base.mrr() == pytest.approx((1.0 / r).mean())
    assert list(base.to_frame().columns) == ["drug_id", "disease_id", "score", "rank", "n_candidates"]
    # an empty list
    empty = predict.rank_pairs(net, batch, [], [], assoc)
    assert len(empty) == 0 and empty.rank.dtype == torch.int64
    assert len(predict.score_pairs(net, batch, [], [])) == 0
