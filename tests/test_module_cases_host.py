"""The designs and references of ``_module_cases.py`` inside their own zero tolerance, without a GPU: every design has
the properties it claims; the float64 autograd references equal a hand-written int64 evaluation and their own fp32
evaluation bit for bit (what the ``2^24`` assertion promises); the host replay of the kept edges equals
``oracle.keep_mask`` of the descriptions; and every evaluation form of each module equals the reference with
``torch.equal`` on the CPU under ``_cpu_backend.patched()`` — a check of the host logic (layouts, offsets, invert bit,
memo, draw order, caches) in its own right, before any GPU time is spent."""
import numpy as np
import pytest
import torch

import _cpu_backend
import _module_cases as MC

CPU = torch.device("cpu")
DESIGNS = {k: f() for k, f in MC.ENC_DESIGNS.items()}


def _present(design, label):
    """(n_dis, n_drug) bool: the cells of relation ``label``, and how often each is listed."""
    cnt = np.zeros((design.n_dis, design.n_drug), np.int64)
    sel = design.label == label
    np.add.at(cnt, (design.dis[sel], design.drug[sel]), 1)
    return cnt


def test_encoder_designs_have_the_properties_they_claim(monkeypatch):
    from dream_gnn_amd import graph as G

    d = DESIGNS["one_block"]
    p = d.props
    c0, c1 = _present(d, 0), _present(d, 1)
    cells = d.n_drug * d.n_dis
    assert 0.80 < c0.sum() / cells < 0.90 and 0.05 < (c1 > 0).sum() / cells < 0.11
    assert ((c0 + c1) == 0)[:51, :36].sum() > 50 and (c0 + c1)[p["held_out"][1], p["held_out"][0]] == 0   # held-out cells
    assert c1[p["dup_label1"][1], p["dup_label1"][0]] == 2 and c1.max() == 2 and (c1 == 2).sum() == 1 and c0.max() == 1
    assert (c0 + c1)[:, p["drug_isolated"]].sum() == 0 and (c0 + c1)[p["dis_isolated"], :].sum() == 0
    assert c0[p["dis_label1_only"]].sum() == 0 and c1[p["dis_label1_only"]].sum() == 1
    assert c0[:51, p["drug_complete"]].all() and c0[p["dis_complete"], :36].all()
    assert not (c0 > 0)[:51, :36].all(1).all() and np.array_equal(_present(DESIGNS["one_block_swapped"], 1), c0)
    r = DESIGNS["refused"]
    assert _present(r, 0)[r.props["dup_label0"][1], r.props["dup_label0"][0]] == 2 and (_present(r, 0) == 2).sum() == 1
    with _cpu_backend.patched():
        for name, des in DESIGNS.items():
            g = MC.build_enc_graph(des, CPU)
            dense = des.props["dense_label"]
            present = torch.from_numpy(_present(des, dense) > 0)
            for nt, pres in (("disease", present), ("drug", present.t())):
                blocks = G._bipartite_blocks(pres)
                comp = g.fused_relations_complement(nt)
                if des.props["blocks"] is None:
                    assert comp is None and (name != "too_many_blocks" or blocks is None)
                    continue
                blk_dst, blk_src, B = blocks
                assert B == des.props["blocks"]
                csr, cans, i0, blockmat = comp
                n_src = pres.shape[1]
                assert i0 == des.props["i0"] and blockmat.shape == (B, n_src) and csr.n_src == 2 * n_src + B
                E0 = int(pres.sum())
                support = int(((blk_dst.view(-1, 1) == blk_src.view(1, -1)) & (blk_dst.view(-1, 1) >= 0)).sum())
                assert 0.5 * support <= E0 < 0.99 * support                    # on the taken side of the threshold ...
                colsum_edges = (csr.indices >= 2 * n_src).sum()
                assert int(colsum_edges) == int((blk_dst >= 0).sum())          # one per destination WITH a block
                if name.startswith("one_block"):
                    dis_blk, drug_blk = (blk_dst, blk_src) if nt == "disease" else (blk_src, blk_dst)
                    assert dis_blk[51] == -1 and dis_blk[52] == -1 and drug_blk[36] == -1
                    assert (dis_blk[:51] == 0).all() and (drug_blk[:36] == 0).all()
                if name == "two_blocks":
                    dis_blk, drug_blk = (blk_dst, blk_src) if nt == "disease" else (blk_src, blk_dst)
                    assert dis_blk.tolist() == des.props["block_of_dis"] and drug_blk.tolist() == des.props["block_of_drug"]
        monkeypatch.setattr(G, "COMPLEMENT_MIN_DENSITY", 0.99)                 # ... and refused on the other
        g = MC.build_enc_graph(DESIGNS["one_block"], CPU)
        assert g.fused_relations_complement("disease") is None and g.fused_relations_complement("drug") is None
    assert G._bipartite_blocks(torch.from_numpy(_present(DESIGNS["too_many_blocks"], 0) > 0)) is None


def test_decoder_and_adjacency_designs_have_the_properties_they_claim():
    for E in MC.DEC_E:
        src, dst = MC.decoder_edges(E)
        assert src.size == E and src[0] == 0 and dst[0] == MC.DEC_N_DIS - 1
        if E > 1:
            assert src[-1] == MC.DEC_N_DRUG - 1 and dst[-1] == 0
            pairs = src * 100 + dst
            assert np.unique(pairs).size < E                                    # repeated pairs
            assert MC.DEC_N_DRUG // 2 not in src and MC.DEC_N_DIS // 2 not in dst
    assert MC.DEC_E[2] // 64 == 5 and MC.DEC_E[2] % 64 == 17 and MC.DEC_E[1] < 64
    with _cpu_backend.patched():
        for salt in (0, 1):
            rows, cols, M = MC.adjacency_edges(salt)
            assert np.array_equal(M, M.T) and set(np.unique(M)) == {0, 1, 2, 3}
            rs = M.sum(1)
            assert rs[MC.ADJ_HUB] == 128 and set(rs[1:]) == {4, 8, 16} and (M[MC.ADJ_HUB] > 0).sum() >= 70
            adj, _ = MC.build_adjacency(CPU, salt)
            idx, val = adj._indices().numpy(), adj._values().numpy()
            assert val.dtype == np.float32 and idx.shape[1] == (M > 0).sum()
            m = M[idx[0], idx[1]]
            assert np.array_equal(val.astype(np.float64), m / rs[idx[0]])
            assert np.all(np.frexp(val.astype(np.float64) / m)[0] == 0.5)      # a power of two times a multiplicity in 1..3


def _int64_gcmc(design, cfg, params, inp, kept, drops, masks):
    """The shared-weight layer by hand, in int64: forward in units of 1/64, the gradients of ``att`` and of both inputs
    likewise; every aggregation spelled out with ``np.add.at``."""
    I = lambda t: np.rint(np.asarray(t, np.float64)).astype(np.int64)
    att, basis = I(params["att"]), I(params["basis"])
    W = np.einsum("rb,bio->rio", att, basis)
    Wl, bl = I(params["ufc.weight"]), I(params["ufc.bias"])
    X = {"drug": I(inp["x_drug"]), "disease": I(inp["x_dis"])}
    Gd = {"drug": I(inp["g_drug"]), "disease": I(inp["g_dis"])}
    n = {"drug": design.n_drug, "disease": design.n_dis}
    edges, scales = MC.relation_edges(design), MC.node_scales(design)
    out, dX, dW = {}, {nt: np.zeros_like(X[nt]) for nt in X}, np.zeros_like(W)
    for nt_dst, nt_src in (("drug", "disease"), ("disease", "drug")):
        ci4 = I(scales[nt_dst]["ci"] * 4).reshape(-1, 1)
        agg = np.zeros((n[nt_dst], cfg.width), np.int64)
        rels = []
        for r, name in enumerate(MC.REL_NAMES):
            can = (nt_src, name if nt_src == "drug" else "rev-" + name, nt_dst)
            src, dst = edges[can]
            k = np.flatnonzero(np.asarray(kept[can]) > 0)
            d4 = I(np.asarray(drops[can]) * 4).reshape(-1, 1)                  # dropout(cj) in quarters
            msg = (X[nt_src] @ W[r]) * d4
            np.add.at(agg, dst[k], msg[src[k]])
            rels.append((r, src[k], dst[k], d4))
        y16 = agg * ci4                                                          # sixteenths
        y64 = np.where(y16 > 0, 4 * y16, y16)                                    # leaky ReLU, slope 1/4
        m2 = 2 * I(masks[nt_dst])
        out[nt_dst] = (y64 * m2) @ Wl.T + 64 * bl
        gq = (Gd[nt_dst] @ Wl) * m2
        gq = np.where(y16 > 0, 4 * gq, gq)                                       # quarters
        g16 = gq * ci4
        for r, src, dst, d4 in rels:
            gm = np.zeros((n[nt_src], cfg.width), np.int64)
            np.add.at(gm, src, g16[dst])
            gh = gm * d4                                                         # sixty-fourths
            dX[nt_src] += gh @ W[r].T
            dW[r] += X[nt_src].T @ gh
    datt = np.einsum("rio,bio->rb", dW, basis)
    f = lambda a: torch.from_numpy(a.astype(np.float64) / 64)
    return {"out_drug": f(out["drug"]), "out_dis": f(out["disease"]), "x_drug.grad": f(dX["drug"]), "x_dis.grad": f(dX["disease"]),
            "grad/att": f(datt)}


def _host_draws(design, cfg, seed):
    """Arbitrary 0/1 draws for the references' own tests (numpy; the module tests replay torch's)."""
    rng = np.random.default_rng(seed)
    scales = MC.node_scales(design)
    drops = {can: torch.from_numpy(scales[can[0]]["cj"].reshape(-1).astype(np.float64) * 2 * rng.integers(0, 2, scales[can[0]]["cj"].size))
             for can in MC.CANS}
    masks = {"drug": torch.from_numpy(rng.integers(0, 2, (design.n_drug, cfg.width)).astype(np.float64)),
             "disease": torch.from_numpy(rng.integers(0, 2, (design.n_dis, cfg.width)).astype(np.float64))}
    return drops, masks


def _layer_operands(design, cfg):
    with _cpu_backend.patched():
        layer = MC.make_layer(cfg, CPU)
    params = {k: p.detach().clone() for k, p in layer.named_parameters()}
    inp = MC.gcmc_inputs(design, cfg)
    return params, inp, {"drug": inp["x_drug"], "disease": inp["x_dis"]}, {"drug": inp["g_drug"], "disease": inp["g_dis"]}


@pytest.mark.parametrize("name", ["one_block", "two_blocks"])
@pytest.mark.parametrize("width", [7, 8])
def test_gcmc_reference_equals_an_int64_evaluation(oracle, name, width):
    design, cfg = DESIGNS[name], MC.LayerCfg(True, width)
    params, inp, x, g = _layer_operands(design, cfg)
    kept = MC.replay_edge_dropout(design, oracle, "select", 3)
    drops, masks = _host_draws(design, cfg, 9)
    want = _int64_gcmc(design, cfg, params, inp, kept, drops, masks)
    got = MC.gcmc_reference(design, cfg, params, x, g, kept, drops, masks)
    assert all(torch.equal(got[k], want[k]) for k in want) and float(want["grad/att"].abs().max()) > 0
    assert float(want["out_dis"].abs().max()) > 64 and float(want["x_drug.grad"].abs().max()) > 1


@pytest.mark.parametrize("name", list(DESIGNS))
@pytest.mark.parametrize("cfg", MC.LAYER_CFGS, ids=lambda c: "%s-%d" % ("shared" if c.shared else "own", c.width))
def test_gcmc_reference_equals_its_fp32_evaluation(oracle, name, cfg):
    design = DESIGNS[name]
    params, inp, x, g = _layer_operands(design, cfg)
    kept = MC.replay_edge_dropout(design, oracle, "randperm", 4)
    drops, masks = _host_draws(design, cfg, 10)
    f64 = MC.gcmc_reference(design, cfg, params, x, g, kept, drops, masks)
    f32 = MC.gcmc_reference(design, cfg, params, x, g, kept, drops, masks, dtype=torch.float32)
    assert set(f32) == set(f64) and all(f32[k].dtype == torch.float32 and torch.equal(f32[k].double(), f64[k]) for k in f64)
    assert ("grad/att" in f64) == cfg.shared and ("grad/ifc.weight" in f64) == (not cfg.shared)


def test_decoder_and_adjacency_references_equal_their_fp32_evaluation(oracle):
    with _cpu_backend.patched():
        dec, gcn = MC.make_decoder(CPU), MC.make_gcn(CPU)
        adj, _ = MC.build_adjacency(CPU)
    params = {k: p.detach().clone() for k, p in dec.named_parameters()}
    rng = np.random.default_rng(1)
    for E in MC.DEC_E:
        src, dst = MC.decoder_edges(E)
        inp = MC.decoder_inputs(E)
        m1, m2 = (torch.from_numpy(rng.integers(0, 2, (E, w)).astype(np.float64)) for w in (128, 64))
        for a, b in ((m1, m2), (None, None)):
            f64 = MC.decoder_reference(params, inp, src, dst, a, b)
            f32 = MC.decoder_reference(params, inp, src, dst, a, b, dtype=torch.float32)
            assert all(torch.equal(f32[k].double(), f64[k]) for k in f64)
            if E > 1:
                assert all(float(v.abs().max()) > 0 for v in f64.values())
    params = {k: p.detach().clone() for k, p in gcn.named_parameters()}
    inp = MC.adjacency_inputs()
    idx, val = adj._indices(), adj._values()
    alive = rng.integers(0, 2, val.shape[0]).astype(np.float64)
    mask = torch.from_numpy(rng.integers(0, 2, (MC.ADJ_N, MC.ADJ_HID)).astype(np.float64))
    for which, al, m in (("conv", None, None), ("conv", alive, None), ("gcn", alive, mask), ("gcn", None, None)):
        f64 = MC.adjacency_reference(params, inp, idx, val, al, m, which)
        f32 = MC.adjacency_reference(params, inp, idx, val, al, m, which, dtype=torch.float32)
        assert all(torch.equal(f32[k].double(), f64[k]) for k in f64) and float(f64["x.grad"].abs().max()) > 0
    # the dense reference by hand for the plain convolution: np.add.at over the entries
    out = np.zeros((MC.ADJ_N, MC.ADJ_HID))
    sup = inp["x"].double().numpy() @ params["gc1.weight"].double().numpy()
    np.add.at(out, idx[0].numpy(), (val.double().numpy() * alive)[:, None] * sup[idx[1].numpy()])
    assert np.array_equal(out + params["gc1.bias"].double().numpy(), MC.adjacency_reference(params, inp, idx, val, alive, None, "conv")["out"].numpy())


@pytest.mark.parametrize("name", list(DESIGNS))
@pytest.mark.parametrize("cfg", MC.LAYER_CFGS, ids=lambda c: "%s-%d" % ("shared" if c.shared else "own", c.width))
def test_every_gcmc_form_equals_the_reference_on_the_cpu_backend(oracle, monkeypatch, name, cfg):
    """per-slice, fused, fused with the epilogue, complement (both) x eval / train x un-dropped / select / randperm."""
    with _cpu_backend.patched():
        assert MC.check_gcmc(monkeypatch, oracle, CPU, DESIGNS[name], cfg) == 30


@pytest.mark.parametrize("name", ["one_block", "one_block_swapped", "two_blocks"])
def test_complement_memo_on_the_cpu_backend(monkeypatch, name):
    with _cpu_backend.patched():
        MC.check_memo(monkeypatch, CPU, DESIGNS[name], MC.LayerCfg(True, 7))


def test_dropped_children_in_complement_form_shift_and_invert_the_descriptions(oracle):
    with _cpu_backend.patched():
        for name in ("one_block", "one_block_swapped", "two_blocks"):
            design = DESIGNS[name]
            graph = MC.build_enc_graph(design, CPU)
            child, kept = MC.enc_graph_of_kind(graph, design, oracle, "select")
            MC.check_complement_structure(graph, child, design)


@pytest.mark.parametrize("E", MC.DEC_E)
def test_every_decoder_form_equals_the_reference_on_the_cpu_backend(monkeypatch, E):
    with _cpu_backend.patched():
        assert MC.check_decoder(monkeypatch, CPU, E) == 4


def test_every_dropped_adjacency_equals_the_reference_on_the_cpu_backend(oracle):
    with _cpu_backend.patched():
        assert MC.check_adjacency(oracle, CPU) == 3 * len(MC.ADJ_KINDS)
        MC.check_adjacency_views(oracle, CPU)
