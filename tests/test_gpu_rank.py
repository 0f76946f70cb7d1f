"""Per-row decoder top-k on the MI355X (csrc/dgmi_pairs_rows.hip -> ops.pair_mlp_row_topk ->
MLPDecoder.top_pairs_per_row -> predict.top_novel_per_disease / top_novel_per_drug): the reference's own scores on the
two fixtures, bit-identity with the global kernel (dgmi_pairs.hip), fp64 per row, edge rows, NaN, subsets,
determinism and sampled rows at the config-4 node counts.

Tolerance (as tests/test_gpu_pairs.py): a returned logit is within 1e-6 * (sum_h |w3_h| (sum_k |W2_hk h1_k| + |b2_h|)
+ |b3|) of fp64, h1 = relu(P[i] + Q[j]); a row's returned set equals its fp64 top-k except for candidates within twice
that tolerance of the k-th logit."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
REL = 1e-6


def _decoder(dev, seed=0):
    from dream_gnn_amd import model as M

    torch.manual_seed(seed)
    return M.MLPDecoder(128).to(dev).eval()


def _PQ(dec, hd, hs):
    """The decoder's lin1 split, with the same torch expressions ``MLPDecoder.top_pairs_per_row`` uses."""
    F = hd.shape[1]
    w1 = dec.lin1.weight
    return torch.addmm(dec.lin1.bias, hd, w1[:, :F].t()), hs @ w1[:, F:].t()


def _params(dec):
    return dec.lin2.weight, dec.lin2.bias, dec.lin3.weight, dec.lin3.bias


def _all64(P, Q, dec, rows=64):
    """(n_drug, n_dis) fp64 logits and tolerances of every pair, chunked over drugs on the device."""
    W2, b2, w3, b3 = (t.detach().double() for t in (dec.lin2.weight, dec.lin2.bias, dec.lin3.weight.reshape(-1), dec.lin3.bias))
    nd, ns = P.shape[0], Q.shape[0]
    L = torch.empty(nd, ns, dtype=torch.float64, device=P.device)
    T = torch.empty_like(L)
    Qd = Q.double()
    for a in range(0, nd, rows):
        b = min(nd, a + rows)
        h1 = torch.relu(P[a:b, None, :].double() + Qd[None])
        L[a:b] = torch.relu(h1 @ W2.t() + b2) @ w3 + b3
        T[a:b] = REL * ((h1 @ W2.abs().t() + b2.abs()) @ w3.abs() + b3.abs())
    return L, T


def _row64(X, C, dec, q):
    """fp64 logits and tolerances of query row q of X against every row of C, on the device."""
    W2, b2, w3, b3 = (t.detach().double() for t in (dec.lin2.weight, dec.lin2.bias, dec.lin3.weight.reshape(-1), dec.lin3.bias))
    h1 = torch.relu(C.double() + X[q].double()[None])
    return torch.relu(h1 @ W2.t() + b2) @ w3 + b3, REL * ((h1 @ W2.abs().t() + b2.abs()) @ w3.abs() + b3.abs())


def _assert_row(cand, logit, count, L, T, known, k):
    """One row against fp64 logits L / tolerances T of all its candidates (1-D, same device) and its known mask."""
    n_nov = int((~known).sum())
    kk = min(k, n_nov)
    assert int(count) == kk
    assert bool((cand[kk:] == -1).all()) and bool(torch.isnan(logit[kk:]).all()), "padding past the count"
    got = cand[:kk].to(L.device)
    assert not bool(known[got].any()), "a known pair was returned"
    assert torch.unique(got).numel() == kk
    err = (logit[:kk].to(L.device).double() - L[got]).abs()
    assert bool((err <= T[got]).all()), "logit off fp64 by %.3e" % float(err.max())
    if kk == 0:
        return
    flat = L.masked_fill(known, float("-inf"))
    top = torch.topk(flat, kk)
    t_k, tol_k = float(top.values[-1]), float(T[top.indices[-1]])
    for p in set(got.tolist()) ^ set(top.indices.tolist()):
        assert abs(float(flat[p]) - t_k) <= 2 * max(float(T[p]), tol_k), "candidate %d is not a near-tie of the k-th" % p
    _assert_row_order(cand[:kk], logit[:kk])


def _assert_row_order(cand, logit):
    """logit descending, ties by candidate ascending, NaN last."""
    c, l = cand.cpu().numpy(), logit.cpu().numpy()
    nan = np.isnan(l)
    if nan.any():
        assert nan[int(np.argmax(nan)):].all(), "a NaN logit ranks before a number"
    for a in range(len(l) - 1):
        if nan[a] or nan[a + 1]:
            assert nan[a + 1] and (not nan[a] or c[a] < c[a + 1]), a
            continue
        assert l[a] > l[a + 1] or (l[a] == l[a + 1] and c[a] < c[a + 1]), a


def _rows(dec, hd, hs, k, by, known=None, rows=None):
    with torch.no_grad():
        return dec.top_pairs_per_row(hd, hs, k, by=by, known=known, rows=rows)


def _check_all_rows(dec, hd, hs, k, known_mask, kd=None, ks=None):
    """Both directions, every row, against the full fp64 matrix."""
    known = None if kd is None else (kd, ks)
    with torch.no_grad():
        P, Q = _PQ(dec, hd, hs)
        L, T = _all64(P, Q, dec)
    for by, LL, TT, M in (("disease", L.t(), T.t(), known_mask.t()), ("drug", L, T, known_mask)):
        qid, cand, logit, count = _rows(dec, hd, hs, k, by, known)
        assert torch.equal(qid.cpu(), torch.arange(LL.shape[0]))
        assert cand.shape == (LL.shape[0], k) and logit.shape == (LL.shape[0], k) and count.shape == (LL.shape[0],)
        for q in range(LL.shape[0]):
            _assert_row(cand[q], logit[q], count[q], LL[q], TT[q], M[q], k)


# ---------------------------------------------------------------------------------------------
# (1) the reference's own scores, row by row
# ---------------------------------------------------------------------------------------------
def _fixture_net_batch(g, dev):
    import types

    from dream_gnn_amd import graph as G
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

    def sparse(prefix, n):
        idx = torch.from_numpy(np.vstack([g[prefix + "_row"], g[prefix + "_col"]]).astype(np.int64))
        return torch.sparse_coo_tensor(idx, torch.from_numpy(g[prefix + "_val"]), (n, n)).to(dev)

    batch = {"enc_graph": G.build_enc_graph(torch.from_numpy(g["enc_drug"]), torch.from_numpy(g["enc_dis"]),
                                            torch.from_numpy(g["enc_values"]), nd, ns, symm=True, device=dev).int(),
             "drug_graph": sparse("drug_graph", nd), "disease_graph": sparse("dis_graph", ns),
             "drug_feature_graph": sparse("drug_fg", nd), "disease_feature_graph": sparse("dis_fg", ns),
             "drug_feat": torch.from_numpy(g["drug_feat"]).to(dev), "disease_feat": torch.from_numpy(g["dis_feat"]).to(dev),
             "drug_sim_feat": torch.from_numpy(g["drug_sim"]).to(dev), "disease_sim_feat": torch.from_numpy(g["dis_sim"]).to(dev)}
    return net.to(dev).train(), batch


def _lists(net, batch, known):
    from dream_gnn_amd import predict

    return {"disease": predict.top_novel_per_disease(net, batch, known, k=128),
            "drug": predict.top_novel_per_drug(net, batch, known, k=128)}


def test_novel_all_rows_match_the_reference_scores(dev):
    g = np.load(os.path.join(GOLD, "novel_all.npz"))
    net, batch = _fixture_net_batch(g, dev)
    out = _lists(net, batch, g["association"])
    d, s, sc = g["ref_drug_id"], g["ref_disease_id"], g["ref_score"].astype(np.float64)
    for by, qcol, ccol in (("disease", s, d), ("drug", d, s)):
        res = out[by]
        n_q = res.count.numel()
        for q in range(n_q):
            sel = np.nonzero(qcol == q)[0]
            sel = sel[np.argsort(-sc[sel], kind="stable")]
            m = len(sel)
            assert int(res.count[q]) == m, (by, q)
            got = (res.drug_id if by == "disease" else res.disease_id)[q, :m].numpy()
            assert np.array_equal(got, ccol[sel]), (by, q)
            assert np.abs(res.score[q, :m].numpy().astype(np.float64) - sc[sel]).max(initial=0.0) <= 1e-5
            assert bool((res.drug_id[q, m:] == -1).all()) and bool((res.disease_id[q, m:] == -1).all())


def test_novel_top50_rows_start_with_the_global_pairs(dev):
    g = np.load(os.path.join(GOLD, "novel_top50.npz"))
    net, batch = _fixture_net_batch(g, dev)
    out = _lists(net, batch, g["association"])
    d, s = g["ref_drug_id"], g["ref_disease_id"]  # in the reference's rank order
    for by, qcol, ccol in (("disease", s, d), ("drug", d, s)):
        res = out[by]
        cand = res.drug_id if by == "disease" else res.disease_id
        for q in range(res.count.numel()):
            sel = np.nonzero(qcol == q)[0]
            assert np.array_equal(cand[q, :len(sel)].numpy(), ccol[sel]), (by, q)


# ---------------------------------------------------------------------------------------------
# (2) bit-identical to the global kernel
# ---------------------------------------------------------------------------------------------
def _key_ge(l, a, b, kl, ka, kb):
    """(l, a, b) ranks at or above (kl, ka, kb): logit descending, then (a, b) ascending (no NaN here)."""
    return (l > kl) | ((l == kl) & ((a < ka) | ((a == ka) & (b <= kb))))


def _cross_check(dec, hd, hs, kd, ks):
    from dream_gnn_amd import ops

    with torch.no_grad():
        P, Q = _PQ(dec, hd, hs)
        gd, gs, gl = ops.pair_mlp_topk(P, Q, *_params(dec), kd, ks, 1024)
    gd, gs, gl = gd.cpu(), gs.cpu(), gl.cpu()
    assert gd.numel() == 1024
    kl, ka, kb = float(gl[-1]), int(gd[-1]), int(gs[-1])
    for by in ("disease", "drug"):
        _, cand, logit, count = _rows(dec, hd, hs, 128, by, (kd, ks))
        cand, logit = cand.cpu(), logit.cpu()
        n_q = cand.shape[0]
        qmat = torch.arange(n_q)[:, None].expand_as(cand)
        valid = cand >= 0
        a, b = (cand, qmat) if by == "disease" else (qmat, cand)  # (drug, disease)
        above = _key_ge(logit.double(), a, b, kl, ka, kb) & valid
        n_above = above.sum(1)
        gq = gs if by == "disease" else gd
        gc = gd if by == "disease" else gs
        per_row = torch.bincount(gq, minlength=n_q)
        assert torch.equal(n_above, torch.clamp(per_row, max=128)), by
        for q in torch.nonzero(per_row).view(-1).tolist():
            sel = torch.nonzero(gq == q).view(-1)[:128]
            m = sel.numel()
            assert torch.equal(cand[q, :m], gc[sel]), (by, q)
            assert torch.equal(logit[q, :m], gl[sel]), (by, q)  # bit for bit, no tolerance
            assert torch.equal(logit[q, :m].view(torch.int32), gl[sel].view(torch.int32))


def test_bit_identical_to_the_global_kernel_lrssl(lrssl):
    _cross_check(lrssl["net"].decoder, lrssl["hd"], lrssl["hs"], *lrssl["known"])


def test_bit_identical_to_the_global_kernel_16k_by_12k(dev):
    nd, ns = 16384, 12288
    dec = _decoder(dev, 5)
    g = torch.Generator(device=dev).manual_seed(6)
    hd, hs = torch.randn(nd, 128, device=dev, generator=g), torch.randn(ns, 128, device=dev, generator=g)
    known = torch.rand(nd, ns, device=dev, generator=g) < 0.01
    kd, ks = known.nonzero(as_tuple=True)
    del known
    _cross_check(dec, hd, hs, kd, ks)


# ---------------------------------------------------------------------------------------------
# (3) fp64 per row
# ---------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lrssl(dev):
    from dream_gnn_amd import model as M
    from dream_gnn_amd import synth

    torch.manual_seed(0)
    batch, labels = synth.dataset_shaped_batch([(763, 681, 3051)], device=dev)
    net = M.Net(synth.net_args()).to(dev).eval()
    drug, dis, _ = batch["enc_pairs"]
    pos = labels.cpu() > 0
    known = (drug[pos].to(dev), dis[pos].to(dev))
    with torch.no_grad():
        hd, hs = net.embed(batch["enc_graph"], batch["drug_graph"], batch["drug_sim_feat"], batch["drug_feat"],
                           batch["disease_graph"], batch["disease_sim_feat"], batch["disease_feat"],
                           batch["drug_feature_graph"], batch["disease_feature_graph"])
    mask = torch.zeros(763, 681, dtype=torch.bool, device=dev)
    mask[known[0].long(), known[1].long()] = True
    return dict(batch=batch, net=net, known=known, mask=mask, hd=hd, hs=hs)


@pytest.mark.parametrize("k", [10, 128])
def test_lrssl_rows_against_fp64(lrssl, k):
    _check_all_rows(lrssl["net"].decoder, lrssl["hd"], lrssl["hs"], k, lrssl["mask"], *lrssl["known"])


def test_2048_by_1536_rows_against_fp64(dev):
    nd, ns = 2048, 1536
    dec = _decoder(dev, 11)
    g = torch.Generator(device=dev).manual_seed(12)
    hd, hs = torch.randn(nd, 128, device=dev, generator=g), torch.randn(ns, 128, device=dev, generator=g)
    mask = torch.rand(nd, ns, device=dev, generator=g) < 0.05
    kd, ks = mask.nonzero(as_tuple=True)
    _check_all_rows(dec, hd, hs, 50, mask, kd, ks)


# ---------------------------------------------------------------------------------------------
# (4) edge rows
# ---------------------------------------------------------------------------------------------
def test_edge_rows(dev):
    dec = _decoder(dev, 1)
    nd, ns = 70, 90
    hd, hs = torch.randn(nd, 128, device=dev), torch.randn(ns, 128, device=dev)
    mask = torch.zeros(nd, ns, dtype=torch.bool, device=dev)
    mask[3, :] = True        # drug 3: every disease known
    mask[:, 7] = True        # disease 7: every drug known
    mask[10, :85] = True     # drug 10: 5 candidates left
    g = torch.Generator().manual_seed(3)
    rd, rs = torch.randint(0, nd, (400,), generator=g), torch.randint(0, ns, (400,), generator=g)
    mask[rd.to(dev), rs.to(dev)] = True
    kd, ks = mask.nonzero(as_tuple=True)
    kd, ks = torch.cat([kd, kd.flip(0), kd[:50]]), torch.cat([ks, ks.flip(0), ks[:50]])  # duplicates, any order
    _, cand, logit, count = _rows(dec, hd, hs, 128, "drug", (kd, ks))
    assert int(count[3]) == 0 and bool((cand[3] == -1).all()) and bool(torch.isnan(logit[3]).all())
    assert int(count[10]) == 5 and sorted(cand[10, :5].tolist()) == [85, 86, 87, 88, 89]
    _, cand, logit, count = _rows(dec, hd, hs, 128, "disease", (kd.int(), ks.int()))
    assert int(count[7]) == 0 and bool((cand[7] == -1).all())
    _check_all_rows(dec, hd, hs, 128, mask, kd, ks)  # k = 128 > 90 and > 70 candidates: counts and padding


def test_out_of_range_known_id_raises(dev):
    dec = _decoder(dev)
    hd, hs = torch.randn(8, 128, device=dev), torch.randn(9, 128, device=dev)
    for by in ("disease", "drug"):
        for kd, ks in (([1, 8], [0, 0]), ([1, 2], [0, -1]), ([2 ** 33, 0], [0, 0])):
            with pytest.raises(RuntimeError, match="outside"):
                _rows(dec, hd, hs, 4, by, (torch.tensor(kd, device=dev), torch.tensor(ks, device=dev)))
        with pytest.raises(RuntimeError, match="outside"):  # also with a query subset
            _rows(dec, hd, hs, 4, by, (torch.tensor([8, 1], device=dev), torch.tensor([0, 9], device=dev)), rows=[1])


@pytest.mark.parametrize("n_cand", [1, 31, 32, 33, 129])
def test_candidate_counts(dev, n_cand):
    dec = _decoder(dev, 2)
    hs = torch.randn(45, 128, device=dev)
    hd = torch.randn(n_cand, 128, device=dev)
    mask = torch.zeros(n_cand, 45, dtype=torch.bool, device=dev)
    with torch.no_grad():
        P, Q = _PQ(dec, hd, hs)
        L, T = _all64(P, Q, dec)
    for k in (1, 32, 128):
        _, cand, logit, count = _rows(dec, hd, hs, k, "disease")
        for q in range(45):
            _assert_row(cand[q], logit[q], count[q], L[:, q], T[:, q], mask[:, q], k)


@pytest.mark.parametrize("n_query", [1, 31, 33, 129])
def test_query_counts(dev, n_query):
    dec = _decoder(dev, 3)
    hd = torch.randn(n_query, 128, device=dev)
    hs = torch.randn(300, 128, device=dev)
    mask = torch.zeros(n_query, 300, dtype=torch.bool, device=dev)
    with torch.no_grad():
        P, Q = _PQ(dec, hd, hs)
        L, T = _all64(P, Q, dec)
    for k in (1, 50, 128):
        _, cand, logit, count = _rows(dec, hd, hs, k, "drug")
        assert cand.shape == (n_query, k)
        for q in range(n_query):
            _assert_row(cand[q], logit[q], count[q], L[q], T[q], mask[q], k)


# ---------------------------------------------------------------------------------------------
# (5) NaN
# ---------------------------------------------------------------------------------------------
def test_nan_rows(dev):
    dec = _decoder(dev, 4)
    hd, hs = torch.randn(40, 128, device=dev), torch.randn(50, 128, device=dev)
    hs[6] = float("nan")   # a NaN disease: a NaN query row per disease, a NaN candidate per drug
    _, cand, logit, count = _rows(dec, hd, hs, 128, "disease")
    assert int(count[6]) == 40 and cand[6, :40].tolist() == list(range(40)) and bool(torch.isnan(logit[6, :40]).all())
    _, cand, logit, count = _rows(dec, hd, hs, 128, "drug")
    for q in range(40):
        assert int(count[q]) == 50 and int(cand[q, 49]) == 6 and bool(torch.isnan(logit[q, 49]))
        assert not bool(torch.isnan(logit[q, :49]).any())
        _assert_row_order(cand[q, :50], logit[q, :50])


# ---------------------------------------------------------------------------------------------
# (6) subsets, (7) determinism
# ---------------------------------------------------------------------------------------------
def test_row_subsets_are_byte_identical(lrssl):
    dec, hd, hs, known = lrssl["net"].decoder, lrssl["hd"], lrssl["hs"], lrssl["known"]
    for by, n in (("disease", 681), ("drug", 763)):
        _, cand, logit, count = _rows(dec, hd, hs, 50, by, known)
        for rows in ([5, 0, n - 1], [17]):
            qid, c2, l2, n2 = _rows(dec, hd, hs, 50, by, known, rows=rows)
            r = torch.tensor(rows, device=cand.device)
            assert qid.tolist() == rows
            assert torch.equal(c2, cand[r]) and torch.equal(n2, count[r])
            assert torch.equal(l2.view(torch.int32), logit[r].view(torch.int32))


def test_deterministic_and_any_stream(dev):
    dec = _decoder(dev, 4)
    hd, hs = torch.randn(3000, 128, device=dev), torch.randn(2000, 128, device=dev)
    kd, ks = torch.randint(0, 3000, (60000,), device=dev), torch.randint(0, 2000, (60000,), device=dev)
    for by in ("disease", "drug"):
        a = _rows(dec, hd, hs, 100, by, (kd, ks))
        b = _rows(dec, hd, hs, 100, by, (kd, ks))
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            c = _rows(dec, hd, hs, 100, by, (kd, ks))
        torch.cuda.current_stream().wait_stream(s)
        torch.cuda.synchronize()
        for x, y, z in zip(a, b, c):
            x, y, z = (t.view(torch.int32) if t.dtype == torch.float32 else t for t in (x, y, z))
            assert torch.equal(x, y) and torch.equal(x, z)


# ---------------------------------------------------------------------------------------------
# (8) config-4 node counts, sampled rows
# ---------------------------------------------------------------------------------------------
def test_config4_node_counts(dev):
    from dream_gnn_amd import synth

    nd, ns, k = 100_000, 50_000, 50
    dec = _decoder(dev, 7)
    g = torch.Generator(device=dev).manual_seed(8)
    hd, hs = torch.randn(nd, 128, device=dev, generator=g), torch.randn(ns, 128, device=dev, generator=g)
    kd, ks = synth.bipartite_edges(nd, ns, 10_000_000, 0, dev)
    kd, ks = kd.long(), ks.long()
    with torch.no_grad():
        P, Q = _PQ(dec, hd, hs)
    r = torch.Generator().manual_seed(9)
    for by, X, C, kq, kc, n_q in (("disease", Q, P, ks, kd, ns), ("drug", P, Q, kd, ks, nd)):
        _, cand, logit, count = _rows(dec, hd, hs, k, by, (kd, ks))
        assert cand.shape == (n_q, k) and int(count.min()) == k
        for q in torch.randperm(n_q, generator=r)[:256].tolist():
            known = torch.zeros(C.shape[0], dtype=torch.bool, device=dev)
            known[kc[kq == q]] = True
            L, T = _row64(X, C, dec, q)
            _assert_row(cand[q], logit[q], count[q], L, T, known, k)


# ---------------------------------------------------------------------------------------------
# (9) the public functions
# ---------------------------------------------------------------------------------------------
def test_public_functions_on_lrssl(lrssl):
    from dream_gnn_amd import predict, top_novel_per_disease, top_novel_per_drug

    net, batch, known = lrssl["net"], lrssl["batch"], lrssl["known"]
    net.train()
    try:
        a = top_novel_per_disease(net, batch, known, k=10)
        assert net.training
        b = top_novel_per_drug(net, batch, known, k=10, drugs=[4, 2])
        assert net.training
    finally:
        net.eval()
    assert isinstance(a, predict.NovelLists) and a.by == "disease" and b.by == "drug"
    qid, cand, logit, count = _rows(net.decoder, lrssl["hd"], lrssl["hs"], 10, "disease", known)
    assert torch.equal(a.query_id, qid.cpu()) and torch.equal(a.drug_id, cand.cpu())
    assert torch.equal(a.logit.view(torch.int32), logit.cpu().view(torch.int32)) and torch.equal(a.count, count.cpu().long())
    assert torch.equal(a.disease_id, torch.where(a.drug_id >= 0, qid.cpu()[:, None].expand(-1, 10), torch.tensor(-1)))
    assert torch.allclose(a.score, torch.sigmoid(a.logit), equal_nan=True)
    qid, cand, logit, count = _rows(net.decoder, lrssl["hd"], lrssl["hs"], 10, "drug", known, rows=[4, 2])
    assert b.query_id.tolist() == [4, 2] and torch.equal(b.disease_id, cand.cpu())
    assert torch.equal(b.drug_id[b.drug_id >= 0].unique(), torch.tensor([2, 4]))
    df = a.to_frame(drug_names=["d%d" % i for i in range(763)])
    assert list(df.columns) == ["query_id", "rank", "drug_id", "disease_id", "score", "drug_name"]
    assert len(df) == int(a.count.sum())
    assert df["rank"].iloc[0] == 1 and df["drug_name"].iloc[0] == "d%d" % int(a.drug_id[0, 0])
