"""All-pairs decoder top-k on the MI355X (csrc/dgmi_pairs.hip -> ops.pair_mlp_topk -> MLPDecoder.top_pairs ->
predict.top_novel_pairs): the reference's get_top_novel_predictions row for row on two fixtures, the existing decoder
path and an fp64 restatement at the lrssl shape, edge shapes, determinism, and exhaustive / sampled checks at scale.

Tolerance: a returned logit is within 1e-6 * (sum_h |w3_h| (sum_k |W2_hk h1_k| + |b2_h|) + |b3|) of fp64, h1 =
relu(P[i] + Q[j]) (f32-MFMA error is ~1.5e-7 of the sum of |a b|); the returned set equals the fp64 top-k except for
pairs within twice that tolerance of the k-th logit."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
REL = 1e-6


def _PQ(dec, hd, hs):
    """The decoder's lin1 split, with the same torch expressions ``MLPDecoder.top_pairs`` uses."""
    F = hd.shape[1]
    w1 = dec.lin1.weight
    return torch.addmm(dec.lin1.bias, hd, w1[:, :F].t()), hs @ w1[:, F:].t()


def _params64(dec):
    return [t.detach().double() for t in (dec.lin2.weight, dec.lin2.bias, dec.lin3.weight.reshape(-1), dec.lin3.bias)]


def _eval64(P, Q, dec, i, j):
    """fp64 logits of the pairs (i, j) and the per-pair tolerance, torch on the device."""
    W2, b2, w3, b3 = _params64(dec)
    h1 = torch.relu(P[i].double() + Q[j].double())
    logit = torch.relu(h1 @ W2.t() + b2) @ w3 + b3
    bound = (h1 @ W2.abs().t() + b2.abs()) @ w3.abs() + b3.abs()
    return logit, REL * bound


def _all64(P, Q, dec, rows=64):
    """(n_drug, n_dis) fp64 logits and tolerances of every pair, chunked over drugs on the device."""
    nd, ns = P.shape[0], Q.shape[0]
    L = torch.empty(nd, ns, dtype=torch.float64, device=P.device)
    T = torch.empty_like(L)
    jj = torch.arange(ns, device=P.device)
    for a in range(0, nd, rows):
        b = min(nd, a + rows)
        ii = torch.arange(a, b, device=P.device).repeat_interleave(ns)
        l, t = _eval64(P, Q, dec, ii, jj.repeat(b - a))
        L[a:b], T[a:b] = l.view(b - a, ns), t.view(b - a, ns)
    return L, T


def _np_all64(P, Q, dec, rows=64):
    """The same restatement in numpy fp64 on the host (the lrssl check)."""
    P, Q = P.detach().cpu().double().numpy(), Q.detach().cpu().double().numpy()
    W2, b2, w3, b3 = (t.cpu().numpy() for t in _params64(dec))
    L = np.empty((P.shape[0], Q.shape[0]))
    T = np.empty_like(L)
    for a in range(0, P.shape[0], rows):
        h1 = np.maximum(P[a:a + rows, None, :] + Q[None], 0.0)
        L[a:a + rows] = np.maximum(h1 @ W2.T + b2, 0.0) @ w3 + b3
        T[a:a + rows] = REL * ((h1 @ np.abs(W2).T + np.abs(b2)) @ np.abs(w3) + abs(float(b3[0])))
    return torch.from_numpy(L), torch.from_numpy(T)


def _assert_ordered(drug, dis, logit):
    """Rank order: logit descending, ties by (drug, disease) ascending, NaN last."""
    d, s, l = drug.cpu().numpy(), dis.cpu().numpy(), logit.cpu().numpy()
    nan = np.isnan(l)
    if nan.any():
        first = int(np.argmax(nan))
        assert nan[first:].all(), "a NaN logit ranks before a number"
    for a in range(len(l) - 1):
        if nan[a + 1] and not nan[a]:
            continue
        if nan[a]:
            assert (d[a], s[a]) < (d[a + 1], s[a + 1])
            continue
        assert l[a] > l[a + 1] or (l[a] == l[a + 1] and (d[a], s[a]) < (d[a + 1], s[a + 1])), a


def _assert_topk(drug, dis, logit, L, T, known, k):
    """The set / tolerance rule against full fp64 logits ``L`` (n_drug x n_dis), tolerances ``T``, ``known`` mask."""
    ns = L.shape[1]
    flat = L.masked_fill(known, float("-inf")).reshape(-1)
    tol = T.reshape(-1)
    n_cand = int((~known).sum())
    kk = min(k, n_cand)
    assert drug.numel() == kk
    got = drug.to(flat.device) * ns + dis.to(flat.device)
    assert not bool(known.reshape(-1)[got].any()), "a known pair was returned"
    assert torch.unique(got).numel() == kk
    ref = flat[got]
    err = (logit.to(flat.device).double() - ref).abs()
    assert bool((err <= tol[got]).all()), "logit off fp64 by %.3e (tol %.3e)" % (float(err.max()), float(tol[got].max()))
    top = torch.topk(flat, kk)
    t_k, tol_k = float(top.values[-1]), float(tol[top.indices[-1]])
    mine, theirs = set(got.tolist()), set(top.indices.tolist())
    for p in mine ^ theirs:
        assert abs(float(flat[p]) - t_k) <= 2 * max(float(tol[p]), tol_k), "pair %d is not a near-tie of the k-th" % p
    _assert_ordered(drug, dis, logit)


# ---------------------------------------------------------------------------------------------
# (a) the reference's own get_top_novel_predictions, row for row
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


@pytest.mark.parametrize("name", ["novel_top50", "novel_all"])
def test_matches_the_reference_top_novel_predictions(dev, name):
    import types

    from dream_gnn_amd import model as M
    from dream_gnn_amd import predict

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
    net = net.to(dev).train()
    out = predict.top_novel_pairs(net, _fixture_batch(g, dev), g["association"], k=int(g["k"]))
    assert net.training  # the flag is restored
    assert np.array_equal(out.drug_id.numpy(), g["ref_drug_id"]) and np.array_equal(out.disease_id.numpy(), g["ref_disease_id"])
    assert np.abs(out.score.numpy().astype(np.float64) - g["ref_score"]).max() <= 1e-5
    df = out.to_frame(drug_names=["d%d" % i for i in range(nd)])
    assert list(df.columns) == ["drug_id", "disease_id", "score", "drug_name"] and len(df) == len(g["ref_drug_id"])
    if name == "novel_all":
        assert len(out) == int((g["association"] == 0).sum()) < int(g["k"])


# ---------------------------------------------------------------------------------------------
# (b) lrssl shape: the existing decoder path and an fp64 restatement
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
        P, Q = _PQ(net.decoder, hd, hs)
    mask = torch.zeros(763, 681, dtype=torch.bool)
    mask[known[0].long().cpu(), known[1].long().cpu()] = True
    return dict(batch=batch, net=net, known=known, mask=mask, hd=hd, hs=hs, P=P, Q=Q)


@pytest.mark.parametrize("k", [1, 200, 1024])
def test_lrssl_against_fp64(lrssl, k):
    net = lrssl["net"]
    with torch.no_grad():
        drug, dis, logit = net.decoder.top_pairs(lrssl["hd"], lrssl["hs"], k, lrssl["known"])
    L, T = _np_all64(lrssl["P"], lrssl["Q"], net.decoder)
    _assert_topk(drug.cpu(), dis.cpu(), logit.cpu(), L, T, lrssl["mask"], k)


@pytest.mark.parametrize("fuse", [True, False])
def test_lrssl_against_the_decoder_forward(lrssl, fuse):
    """An eval Net.forward over a decoder graph of every candidate pair, sorted by the same key."""
    from dream_gnn_amd import graph as G
    from dream_gnn_amd import predict

    net, batch, mask = lrssl["net"], lrssl["batch"], lrssl["mask"]
    cand = (~mask).nonzero()
    dec = G.build_dec_graph(cand[:, 0], cand[:, 1], 763, 681, device=batch["drug_feat"].device).int()
    net.decoder.fuse_lin1 = fuse
    try:
        with torch.no_grad():
            pred, *_ = net(batch["enc_graph"], dec, batch["drug_graph"], batch["drug_sim_feat"], batch["drug_feat"],
                           batch["disease_graph"], batch["disease_sim_feat"], batch["disease_feat"],
                           batch["drug_feature_graph"], batch["disease_feature_graph"])
    finally:
        net.decoder.fuse_lin1 = True
    fwd = pred.view(-1).double().cpu().numpy()
    src, dst = cand[:, 0].numpy(), cand[:, 1].numpy()  # the decoder graph's edge order
    order = np.lexsort((dst, src, -fwd))
    f_at = np.full((763, 681), np.nan)
    f_at[src, dst] = fwd
    _, T = _np_all64(lrssl["P"], lrssl["Q"], net.decoder)
    tol = 10 * T.numpy()  # the forward path rounds lin1 in another order: a looser bound than the kernel's own
    for k in (1, 200, 1024):
        out = predict.top_novel_pairs(net, batch, lrssl["known"], k=k)
        assert len(out) == k
        got = list(zip(out.drug_id.tolist(), out.disease_id.tolist()))
        kth = fwd[order[k - 1]]
        for (i, j), l in zip(got, out.logit.tolist()):
            assert abs(l - f_at[i, j]) <= tol[i, j], (i, j)
        for i, j in set(zip(src[order[:k]].tolist(), dst[order[:k]].tolist())) ^ set(got):
            assert abs(f_at[i, j] - kth) <= 2 * tol[i, j], (i, j)
        _assert_ordered(out.drug_id, out.disease_id, out.logit)


# ---------------------------------------------------------------------------------------------
# (c) edge shapes
# ---------------------------------------------------------------------------------------------
def _decoder(dev, seed=0):
    from dream_gnn_amd import model as M

    torch.manual_seed(seed)
    return M.MLPDecoder(128).to(dev).eval()


@pytest.mark.parametrize("n_dis", [1, 33, 681])
def test_single_drug_rows(dev, n_dis):
    dec = _decoder(dev)
    hd, hs = torch.randn(1, 128, device=dev), torch.randn(n_dis, 128, device=dev)
    with torch.no_grad():
        P, Q = _PQ(dec, hd, hs)
        for k in (1, 5, 1024):
            drug, dis, logit = dec.top_pairs(hd, hs, k)
            L, T = _all64(P, Q, dec)
            _assert_topk(drug, dis, logit, L, T, torch.zeros(1, n_dis, dtype=torch.bool, device=dev), k)


def test_known_lists(dev):
    dec = _decoder(dev, 1)
    nd, ns = 70, 90
    hd, hs = torch.randn(nd, 128, device=dev), torch.randn(ns, 128, device=dev)
    with torch.no_grad():
        P, Q = _PQ(dec, hd, hs)
        L, T = _all64(P, Q, dec)
        empty = torch.zeros(0, dtype=torch.int32, device=dev)
        drug, dis, logit = dec.top_pairs(hd, hs, 100, (empty, empty))
        _assert_topk(drug, dis, logit, L, T, torch.zeros(nd, ns, dtype=torch.bool, device=dev), 100)
        # duplicates, in any order, int64 ids
        g = torch.Generator().manual_seed(3)
        kd, ks = torch.randint(0, nd, (500,), generator=g), torch.randint(0, ns, (500,), generator=g)
        kd, ks = torch.cat([kd, kd.flip(0)]), torch.cat([ks, ks.flip(0)])
        mask = torch.zeros(nd, ns, dtype=torch.bool)
        mask[kd, ks] = True
        drug, dis, logit = dec.top_pairs(hd, hs, 300, (kd.to(dev), ks.to(dev)))
        _assert_topk(drug, dis, logit, L, T, mask.to(dev), 300)
        # every cell known but 3: exactly those come back
        keep = [(5, 7), (0, 0), (69, 89)]
        mask = torch.ones(nd, ns, dtype=torch.bool)
        for a, b in keep:
            mask[a, b] = False
        kd, ks = mask.nonzero(as_tuple=True)
        drug, dis, logit = dec.top_pairs(hd, hs, 200, (kd.int().to(dev), ks.int().to(dev)))
        assert sorted(zip(drug.tolist(), dis.tolist())) == sorted(keep)
        _assert_topk(drug, dis, logit, L, T, mask.to(dev), 200)


def test_nan_row_ranks_last(dev):
    dec = _decoder(dev, 2)
    hd, hs = torch.randn(6, 128, device=dev), torch.randn(40, 128, device=dev)
    hd[2] = float("nan")
    with torch.no_grad():
        drug, dis, logit = dec.top_pairs(hd, hs, 240)
    assert drug.numel() == 240
    assert bool(torch.isnan(logit[200:]).all()) and not bool(torch.isnan(logit[:200]).any())
    assert drug[200:].tolist() == [2] * 40 and dis[200:].tolist() == list(range(40))
    _assert_ordered(drug, dis, logit)


def test_out_of_range_known_id_raises(dev):
    dec = _decoder(dev)
    hd, hs = torch.randn(8, 128, device=dev), torch.randn(9, 128, device=dev)
    for kd, ks in (([1, 8], [0, 0]), ([1, 2], [0, -1]), ([2 ** 33, 0], [0, 0])):
        with pytest.raises(RuntimeError, match="outside"):
            dec.top_pairs(hd, hs, 4, (torch.tensor(kd, device=dev), torch.tensor(ks, device=dev)))


# ---------------------------------------------------------------------------------------------
# (d) determinism and streams
# ---------------------------------------------------------------------------------------------
def test_deterministic_and_any_stream(dev):
    dec = _decoder(dev, 4)
    hd, hs = torch.randn(3000, 128, device=dev), torch.randn(2000, 128, device=dev)
    kd, ks = torch.randint(0, 3000, (60000,), device=dev), torch.randint(0, 2000, (60000,), device=dev)
    with torch.no_grad():
        a = dec.top_pairs(hd, hs, 1000, (kd, ks))
        b = dec.top_pairs(hd, hs, 1000, (kd, ks))
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            c = dec.top_pairs(hd, hs, 1000, (kd, ks))
        torch.cuda.current_stream().wait_stream(s)
    for x, y, z in zip(a, b, c):
        assert torch.equal(x, y) and torch.equal(x, z)
    assert torch.equal(a[2].view(torch.int32), b[2].view(torch.int32))


# ---------------------------------------------------------------------------------------------
# (e) exhaustive check at 16 384 x 12 288, (f) config-4 node counts
# ---------------------------------------------------------------------------------------------
def test_exhaustive_16k_by_12k(dev):
    nd, ns, k = 16384, 12288, 1000
    dec = _decoder(dev, 5)
    g = torch.Generator(device=dev).manual_seed(6)
    hd, hs = torch.randn(nd, 128, device=dev, generator=g), torch.randn(ns, 128, device=dev, generator=g)
    known = torch.rand(nd, ns, device=dev, generator=g) < 0.01
    kd, ks = known.nonzero(as_tuple=True)
    with torch.no_grad():
        drug, dis, logit = dec.top_pairs(hd, hs, k, (kd, ks))
        P, Q = _PQ(dec, hd, hs)
        L, T = _all64(P, Q, dec)
    _assert_topk(drug, dis, logit, L, T, known, k)


def test_config4_node_counts(dev):
    from dream_gnn_amd import synth

    nd, ns, k = 100_000, 50_000, 200
    dec = _decoder(dev, 7)
    g = torch.Generator(device=dev).manual_seed(8)
    hd, hs = torch.randn(nd, 128, device=dev, generator=g), torch.randn(ns, 128, device=dev, generator=g)
    kd, ks = synth.bipartite_edges(nd, ns, 10_000_000, 0, dev)
    with torch.no_grad():
        drug, dis, logit = dec.top_pairs(hd, hs, k, (kd, ks))
        P, Q = _PQ(dec, hd, hs)
        assert drug.numel() == k
        _assert_ordered(drug, dis, logit)
        known_keys = torch.sort(kd.long() * ns + ks.long()).values
        got = drug.to(dev) * ns + dis.to(dev)
        assert not bool(torch.isin(got, known_keys).any())
        l64, tol = _eval64(P, Q, dec, drug.to(dev), dis.to(dev))
        assert bool(((logit.double() - l64).abs() <= tol).all())
        kth, tol_k = float(l64[-1]), float(tol[-1])
        r = torch.Generator(device=dev).manual_seed(9)
        for _ in range(10):
            i = torch.randint(0, nd, (1_000_000,), device=dev, generator=r)
            j = torch.randint(0, ns, (1_000_000,), device=dev, generator=r)
            keys = i * ns + j
            cand = ~torch.isin(keys, known_keys) & ~torch.isin(keys, got)
            l, t = _eval64(P, Q, dec, i[cand], j[cand])
            assert bool((l <= kth + torch.clamp(t, min=tol_k) * 2).all()), float((l - kth).max())
