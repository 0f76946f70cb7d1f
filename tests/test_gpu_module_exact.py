"""The modules that compose the kernels — ``GCMCLayer``, ``MLPDecoder``, ``GraphConvolution`` / ``GCN.from_support`` — on
the device at ZERO tolerance: on the designed operands of ``_module_cases.py`` (small integers and powers of two) every
evaluation form must give the bits of the float64 reference, hence of every other form.  No tolerance anywhere in this
file: every comparison is ``torch.equal`` (zeros by value).

The random draws never come from the code under test.  Kept edges: the host replays the seeds (``select``: one
``randint`` per relation handed to ``oracle.random_subset_mask``, which must equal ``oracle.keep_mask`` of each
description) or the permutations (``randperm``) of a CPU generator seeded alike.  Dropout masks: torch's own draws on the
device under the same ``torch.manual_seed`` — for the layer one ``F.dropout(cj)`` per relation in canonical order, then
the layer masks drug before disease at the UNPADDED width; every form, the per-slice ``nn.Dropout`` path included, must
leave ``torch.cuda.get_rng_state()`` where that replay leaves it.  For the decoder every form (gather-concat + lin1,
``gather_add_relu_dropout``, the ``_EdgeLinear*`` functions) draws the same two tensors: dropout over (E, 128), then over
(E, 64)."""
import numpy as np
import pytest
import torch

import _module_cases as MC

pytestmark = pytest.mark.gpu

DESIGNS = {k: f() for k, f in MC.ENC_DESIGNS.items()}
ROUTES = {"default": (None, True), "sliced-compact": ("sliced", True), "sliced-onthefly": ("sliced", False)}
CFG_IDS = lambda c: "%s-%d" % ("shared" if c.shared else "own", c.width)


def _set_route(monkeypatch, route):
    from dream_gnn_amd import ops

    force, compact = ROUTES[route]
    monkeypatch.setattr(ops, "FORCE_KERNEL", force)
    monkeypatch.setattr(ops, "COMPACT_DROPPED", compact)
    return force, compact


def test_premise_the_gemm_library_is_exact_on_the_designed_operands(oracle, dev):
    """``torch.mm`` and ``nn.Linear`` on the device equal the int64 product on the operands the second stages see: the
    ``ufc`` / ``ifc`` inputs of the layer (multiples of 1/64) and the decoder's lin2 / lin3 inputs (integers up to a few
    thousand), whatever the library does with its inputs.  A failure here is a finding about the GEMM library."""
    stages = []
    design, cfg = DESIGNS["one_block"], MC.LayerCfg(False, 7)
    layer = MC.make_layer(cfg, torch.device("cpu"))
    params = {k: p.detach().clone() for k, p in layer.named_parameters()}
    inp = MC.gcmc_inputs(design, cfg)
    rng = np.random.default_rng(2)
    scales = MC.node_scales(design)
    drops = {can: torch.from_numpy(scales[can[0]]["cj"].reshape(-1).astype(np.float64) * 2 * rng.integers(0, 2, scales[can[0]]["cj"].size))
             for can in MC.CANS}
    masks = {nt: torch.from_numpy(rng.integers(0, 2, (n, cfg.width)).astype(np.float64)) for nt, n in (("drug", design.n_drug), ("disease", design.n_dis))}
    taps = {}
    MC.gcmc_reference(design, cfg, params, {"drug": inp["x_drug"], "disease": inp["x_dis"]},
                      {"drug": inp["g_drug"], "disease": inp["g_dis"]}, None, drops, masks, taps=taps)
    stages += [(64, v) for v in taps.values()]
    dec = MC.make_decoder(torch.device("cpu"))
    E = MC.DEC_E[2]
    src, dst = MC.decoder_edges(E)
    m1, m2 = (torch.from_numpy(rng.integers(0, 2, (E, w)).astype(np.float64)) for w in (128, 64))
    taps = {}
    MC.decoder_reference({k: p.detach().clone() for k, p in dec.named_parameters()}, MC.decoder_inputs(E), src, dst, m1, m2, taps=taps)
    stages += [(1, v) for v in taps.values()]
    assert len(stages) == 5
    for unit, (a, w, b) in stages:
        ai, wi, bi = (np.rint(t.numpy() * u).astype(np.int64) for t, u in ((a, unit), (w, 1), (b, unit)))
        want = torch.from_numpy((ai @ wi.T + bi).astype(np.float64) / unit)
        assert float(want.abs().max()) > 0
        a32, w32, b32 = a.float().to(dev), w.float().to(dev), b.float().to(dev)
        assert torch.equal(torch.mm(a32, w32.t()).cpu().double() + b.double(), want)
        assert torch.equal(torch.nn.functional.linear(a32, w32, b32).cpu().double(), want)


# ---------------------------------------------------------------------------------------------
# (a) GCMCLayer
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("route", list(ROUTES))
@pytest.mark.parametrize("cfg", MC.LAYER_CFGS, ids=CFG_IDS)
@pytest.mark.parametrize("name", list(DESIGNS))
def test_every_gcmc_form_gives_the_bits_of_the_reference(oracle, dev, monkeypatch, name, cfg, route):
    """per-slice / fused / fused + epilogue / complement / complement + epilogue x eval / train x un-dropped / ``select``
    / ``randperm`` (30 runs of one design, layout, width and route): outputs, every gradient and the generator state.
    ``refused`` and ``too_many_blocks`` have no complement form: the layer must fall back with unchanged results."""
    design = DESIGNS[name]
    force, compact = _set_route(monkeypatch, route)
    seen = set()

    def hook(form, kind, train, parent, gr, layer):
        for nt in ("drug", "disease"):
            if form == "slice":
                views = [gr[c].csr for c in MC.CANS if c[2] == nt]
            elif form.startswith("complement") and design.props["blocks"] is not None:
                views = [gr.fused_relations_complement(nt)[0]]
                if kind == "select":
                    MC.check_complement_structure(parent, gr, design)
                seen.add("complement")
            else:
                assert not form.startswith("complement") or gr.fused_relations_complement(nt) is None
                views = [gr.fused_relations(nt)[0]]
            for v in views:  # the route was taken
                assert (v._sliced is not None) == (force == "sliced") and (v._sliced_t is not None) == (force == "sliced")
                if kind == "select":
                    assert v._keep is not None and (("sliced" in v._c and "sliced_t" in v._c) == (force == "sliced" and compact))
                else:
                    assert v._keep is None and not v._c

    assert MC.check_gcmc(monkeypatch, oracle, dev, design, cfg, hook=hook) == 30
    assert ("complement" in seen) == (design.props["blocks"] is not None)


@pytest.mark.parametrize("name", ["one_block", "one_block_swapped", "two_blocks"])
def test_complement_memo(dev, monkeypatch, name):
    MC.check_memo(monkeypatch, dev, DESIGNS[name], MC.LayerCfg(True, 7))
    MC.check_memo(monkeypatch, dev, DESIGNS[name], MC.LayerCfg(False, 8))


# ---------------------------------------------------------------------------------------------
# (b) MLPDecoder
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("gates", ["default", "patched"])
@pytest.mark.parametrize("E", MC.DEC_E)
def test_every_decoder_form_gives_the_bits_of_the_reference(dev, monkeypatch, E, gates):
    """``fuse_lin1`` off (gather-concat, then lin1) and on, dropout active (``gather_add_relu_dropout``) and inactive.
    ``patched``: ``_EdgeLinear.MIN_ROWS = 1`` and ``CHUNK = 64``, so that ``_EdgeLinear``, ``_ReluDropout``,
    ``_EdgeLinearReluDropout`` and the split-K weight gradient run at E = 337 (five chunks and a tail of 17), 50 (tail
    only) and 1."""
    from dream_gnn_amd import model as M

    calls = {"split": 0, "relu_dropout": 0, "edge_linear": 0, "fused2": 0}
    split = M._split_k_weight_grad

    def counted(dy, x, chunk):
        calls["split"] += 1
        assert chunk == 64 and x.shape[0] == E
        return split(dy, x, chunk)

    monkeypatch.setattr(M, "_split_k_weight_grad", counted)
    for key, cls in (("relu_dropout", M._ReluDropout), ("edge_linear", M._EdgeLinear), ("fused2", M._EdgeLinearReluDropout)):
        def fwd(ctx, *a, _f=cls.forward, _k=key):
            calls[_k] += 1
            return _f(ctx, *a)
        monkeypatch.setattr(cls, "forward", staticmethod(fwd))
    patched = gates == "patched"
    assert MC.check_decoder(monkeypatch, dev, E, *((1, 64) if patched else ())) == 4
    if patched:  # eval: lin1 (concat form), lin2, lin3 through _EdgeLinear in both forms; train: the fused functions
        assert calls["split"] == 6 and calls["relu_dropout"] == 1 and calls["fused2"] == 2 and calls["edge_linear"] == 8
    else:
        assert not any(calls.values())


# ---------------------------------------------------------------------------------------------
# (c) GraphConvolution and GCN.from_support on the designed adjacency
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("route", ["default", "sliced-mult", "sliced-values"])
def test_every_dropped_adjacency_gives_the_bits_of_the_reference(oracle, dev, monkeypatch, route):
    """The tensor itself, a dropped tensor (``_dgmi_parent``), a tensor of a tensor (positions relative to the root),
    ``as_view`` with ``select`` (a description) and ``randperm`` (a mask), a dropout of each kind of view, and
    ``random_edge_dropout_sparse_views`` on two adjacencies."""
    from dream_gnn_amd import layers as L, ops

    sliced = route != "default"
    monkeypatch.setattr(ops, "FORCE_KERNEL", "sliced" if sliced else None)
    monkeypatch.setattr(ops, "MULT_FORM", route != "sliced-values")

    def hook(kind, adj, handed):
        base, view = L.adjacency_csr(adj), L.adjacency_csr(handed)
        assert (base._sliced is not None) == sliced
        mf = base._mult_form()
        if ops.MULT_FORM:
            assert mf is not None and mf[0] == "row" and int(mf[2].max()) == 2 and int(mf[2].min()) == 0
        else:
            assert mf is None
        if kind == "tensor":
            assert view is base
        elif kind in ("view_select", "views"):    # a description: the parent's values, its own compacted layouts
            assert view._keep is not None and view._v is base._v and view._c is not base._c and view._S is base._S
            assert (view._mult_form() is not None) == ops.MULT_FORM and (("sliced" in view._c) == sliced)
        else:                                      # a mask folded into the values: no multiplicity form
            assert view._keep is None and view._mask is not None and view._mult_form() is None and view._S is base._S

    assert MC.check_adjacency(oracle, dev, hook=hook) == 3 * len(MC.ADJ_KINDS)
    MC.check_adjacency_views(oracle, dev, hook=hook)
