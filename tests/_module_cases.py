"""Designed inputs and plain references for the modules that COMPOSE the kernels (helper, like ``_edge_cases.py``):
``GCMCLayer`` in every evaluation form, ``MLPDecoder`` in its three first stages, ``GraphConvolution`` / ``GCN.from_support``
over every kind of dropped adjacency.  The modules are linear maps, a leaky ReLU and 0/1 masks, so on small integers and
powers of two every evaluation form gives the SAME BITS, and those bits are computable on the host.

Exactness rule (that of ``_spmm_cases.py``): every operand is an integer or a power of two — features and upstream
gradients integers in [-2, 2], weights sparse with entries in {-1, 0, 1, 2}, biases integers in [-2, 2], ``cj`` / ``ci`` in
{0, 0.25, 0.5, 1, 2}, slope 0.25, every dropout probability 0.5 (scale 2) — all exact in bf16 and TF32 as well.  Every
reference is a float64 ``torch.autograd`` evaluation on the CPU written from the COO triplets alone, and checks itself
product by product (``Products``): for every ``C = A @ B`` of the forward, and for both products of its backward,
``sum|terms|`` — ``|A| @ |B|``, ``|dC| @ |B|^T``, ``|A|^T @ |dC|`` on the TRUE operands — stays below ``2^22`` granules, as
does every intermediate tensor and gradient.  Each stage is then exact under any association given exact inputs, and by
induction every form sees the same intermediates.  Every cell of the relation with the most edges is counted twice more
in these bounds (a complement form replaces that relation by a column sum minus the missing cells: sums over the same
cells); the factor 4 to ``2^24`` covers a gradient accumulated from up to four uses.

The random draws never come from the code under test: kept edges are replayed from the seeds / permutations of a CPU
generator the test owns, dropout masks from torch's own draws on the same device under the same ``torch.manual_seed`` in
the documented order (``replay_gcmc_draws``, ``replay_decoder_draws``)."""
from collections import namedtuple

import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

SLOPE = 0.25
P_DROP = 0.5
EDGE_DROP = 0.3
ROOM = 2 ** 22
GRAN_GCMC = 2.0 ** -6        # cj (1/4) x ci (1/4) x slope (1/4), forward and backward alike
GRAN_DEC = 1.0               # integers throughout (dropout scale 2)
CJ_VALUES = np.array([0.25, 0.5, 1.0, 0.5, 1.0, 0.25, 2.0], np.float32)
CI_VALUES = np.array([0.5, 1.0, 0.25, 1.0, 2.0, 0.5, 0.25], np.float32)


class Products:
    """The products and intermediates of one float64 evaluation, for the exactness condition (module docstring)."""

    def __init__(self, granularity, what):
        self.gran, self.what, self.mms, self.kept = granularity, what, [], []

    def mm(self, a, b, a_bound=None):
        """``a @ b``; ``a_bound``: what stands for ``|a|`` in the bounds (an adjacency with cells counted more often)."""
        c = a @ b
        if c.requires_grad:
            c.retain_grad()
        self.mms.append((a, b, c, a_bound))
        return c

    def keep(self, t):
        if t.requires_grad:
            t.retain_grad()
        self.kept.append(t)
        return t

    def check(self, extra=()):
        worst = 0.0
        for a, b, c, a_bound in self.mms:
            A, B = (a.detach().abs() if a_bound is None else a_bound), b.detach().abs()
            cands = [A @ B]
            if c.grad is not None:
                cands += [c.grad.abs() @ B.t(), A.t() @ c.grad.abs()]
            worst = max([worst] + [float(t.max()) for t in cands if t.numel()])
        for t in list(self.kept) + [c for _, _, c, _ in self.mms] + list(extra):
            for v in (t, getattr(t, "grad", None)):
                if v is not None and v.numel():
                    worst = max(worst, float(v.detach().abs().max()))
        assert worst / self.gran < ROOM, (self.what, worst / self.gran)
        return worst / self.gran


def ints(rng, shape, lo=-2, hi=2):
    return rng.integers(lo, hi + 1, shape).astype(np.float32)


def sparse_ints(rng, shape, density):
    """Entries in {-1, 0, 1, 2}, about ``density`` of them non-zero, no all-zero tensor."""
    v = rng.choice(np.array([-1.0, 1.0, 2.0], np.float32), size=shape) * (rng.random(shape) < density)
    if not v.any():
        v.reshape(-1)[0] = 1.0
    return v.astype(np.float32)


def rng_state(device):
    return torch.cuda.get_rng_state(device) if torch.device(device).type == "cuda" else torch.get_rng_state()


# ---------------------------------------------------------------------------------------------
# encoder graphs
# ---------------------------------------------------------------------------------------------
EncDesign = namedtuple("EncDesign", "name n_drug n_dis drug dis label props")


def _triplets(L, rng, extra=()):
    """Cells of the label matrix ``L`` (drug x disease; -1: no cell) plus ``extra`` repeated cells, in a shuffled order."""
    d, s = np.nonzero(L >= 0)
    lab = L[d, s]
    for (ed, es) in extra:
        d, s, lab = np.append(d, ed), np.append(s, es), np.append(lab, L[ed, es])
    order = rng.permutation(d.size)
    return d[order].astype(np.int64), s[order].astype(np.int64), lab[order].astype(np.float32)


def _one_block_labels():
    rng = np.random.default_rng(11)
    n_drug, n_dis = 37, 53
    u = rng.random((n_drug, n_dis))
    L = np.where(u < 0.85, 0, np.where(u < 0.93, 1, -1)).astype(np.int64)
    props = dict(drug_isolated=36, dis_isolated=52, dis_label1_only=51, drug_complete=5, dis_complete=7)
    L[props["drug_isolated"], :] = -1
    L[:, props["dis_isolated"]] = -1
    L[:, props["dis_label1_only"]] = -1
    L[3, props["dis_label1_only"]] = 1                 # its only edge is a label-1 edge: no block, no column-sum edge
    L[props["drug_complete"], :51] = 0
    L[:36, props["dis_complete"]] = 0
    L[2, 9], L[4, 11] = 1, -1                            # a label-1 cell to repeat, and a held-out cell for certain
    props.update(dup_label1=(2, 9), held_out=(4, 11))
    return L, props


def one_block(swap=False, dup_dense=False):
    """37 drugs x 53 diseases, label 0 on ~85 % of the cells, label 1 on ~8 %, the rest held out; one label-1 cell listed
    twice; a drug and a disease with no edge; a disease whose only edge is a label-1 edge; a drug row and a disease
    column complete in relation 0.  ``swap``: the labels exchanged (the dense relation is then i0 = 1); ``dup_dense``: one
    cell of the DENSE relation listed twice as well (the complement form must refuse)."""
    L, props = _one_block_labels()
    extra = [props["dup_label1"]]
    if dup_dense:
        props["dup_label0"] = (6, 13)
        assert L[6, 13] == 0
        extra.append(props["dup_label0"])
    if swap:
        L = np.where(L >= 0, 1 - L, L)
    d, s, lab = _triplets(L, np.random.default_rng(12), extra)
    name = "refused" if dup_dense else ("one_block_swapped" if swap else "one_block")
    props.update(blocks=None if dup_dense else 1, i0=1 if swap else 0, dense_label=1 if swap else 0)
    return EncDesign(name, 37, 53, d, s, lab, props)


def two_blocks():
    """(20 x 30) + (17 x 23), ~90 % of each block's cells (8 % of them label 1), nothing across, plus one isolated pair
    joined by a single label-1 edge: B == 2 and one node of each type with block -1."""
    rng = np.random.default_rng(13)
    L = np.full((38, 54), -1, np.int64)
    for (d0, nd, s0, ns) in ((0, 20, 0, 30), (20, 17, 30, 23)):
        u = rng.random((nd, ns))
        blk = np.where(u < 0.82, 0, np.where(u < 0.90, 1, -1))
        blk[0, :], blk[:, 0] = 0, 0                      # every node of the block has a relation-0 cell
        L[d0:d0 + nd, s0:s0 + ns] = blk
    L[37, 53] = 1
    d, s, lab = _triplets(L, np.random.default_rng(14))
    return EncDesign("two_blocks", 38, 54, d, s, lab, dict(blocks=2, i0=0, dense_label=0, drug_no_block=37, dis_no_block=53,
                                                           block_of_drug=[0] * 20 + [1] * 17 + [-1],
                                                           block_of_dis=[0] * 30 + [1] * 23 + [-1]))


def too_many_blocks():
    """Nine dense 4 x 4 blocks (one label-1 cell each): more than 8 components, the complement form must refuse."""
    L = np.full((36, 36), -1, np.int64)
    for b in range(9):
        L[4 * b:4 * b + 4, 4 * b:4 * b + 4] = 0
        L[4 * b + b % 4, 4 * b + (b + 1) % 4] = 1
    d, s, lab = _triplets(L, np.random.default_rng(15))
    return EncDesign("too_many_blocks", 36, 36, d, s, lab, dict(blocks=None, i0=0, dense_label=0))


ENC_DESIGNS = {"one_block": one_block, "one_block_swapped": lambda: one_block(swap=True), "two_blocks": two_blocks,
               "refused": lambda: one_block(dup_dense=True), "too_many_blocks": too_many_blocks}
REL_NAMES = ("0", "1")
CANS = (("disease", "rev-0", "drug"), ("disease", "rev-1", "drug"), ("drug", "0", "disease"), ("drug", "1", "disease"))


def relation_edges(design):
    """canonical relation -> (src ids, dst ids) in the order ``build_enc_graph`` lists them (input order per label)."""
    out = {}
    for r, name in enumerate(REL_NAMES):
        sel = np.flatnonzero(design.label == r)
        out[("drug", name, "disease")] = (design.drug[sel], design.dis[sel])
        out[("disease", "rev-" + name, "drug")] = (design.dis[sel], design.drug[sel])
    return out


def node_scales(design):
    """Designed ``cj`` / ``ci`` per node type (0 for a node without an edge), overwriting the square roots."""
    out = {}
    for nt, ids, n in (("drug", design.drug, design.n_drug), ("disease", design.dis, design.n_dis)):
        deg = np.bincount(ids, minlength=n)
        i = np.arange(n)
        salt = 0 if nt == "drug" else 3
        out[nt] = dict(cj=np.where(deg > 0, CJ_VALUES[(i * 5 + salt) % 7], 0).astype(np.float32).reshape(-1, 1),
                       ci=np.where(deg > 0, CI_VALUES[(i * 3 + salt) % 7], 0).astype(np.float32).reshape(-1, 1))
    return out


def build_enc_graph(design, device):
    from dream_gnn_amd import graph as G

    g = G.build_enc_graph(torch.from_numpy(design.drug), torch.from_numpy(design.dis), torch.from_numpy(design.label),
                          design.n_drug, design.n_dis, device=device).int()
    assert tuple(g.canonical_etypes) == CANS
    for nt, d in node_scales(design).items():
        for k, v in d.items():
            g.nodes[nt].data[k] = torch.from_numpy(v).to(device)
    return g


def replay_edge_dropout(design, oracle, selection, seed):
    """The kept-edge masks of ``graph.random_edge_dropout(g, EDGE_DROP, generator=Generator(seed), selection=...)``
    replayed on the host: one draw per relation in canonical order — a 62-bit seed handed to ``oracle.random_subset_mask``
    ("select"), or ``torch.randperm(E)[:keep]`` ("randperm")."""
    gen = torch.Generator().manual_seed(seed)
    edges = relation_edges(design)
    kept = {}
    for can in CANS:
        E = int(edges[can][0].size)
        keep = max(1, int(E * (1 - EDGE_DROP)))
        if selection == "select":
            s = int(torch.randint(0, 2 ** 62, (1,), generator=gen).item())
            kept[can] = np.asarray(oracle.random_subset_mask(E, keep, s), np.float64)
        else:
            m = np.zeros(E, np.float64)
            m[torch.randperm(E, generator=gen)[:keep].numpy()] = 1.0
            kept[can] = m
        assert kept[can].sum() == keep
    return kept


def dropped_enc_graph(graph, selection, seed):
    from dream_gnn_amd import graph as G

    return G.random_edge_dropout(graph, EDGE_DROP, generator=torch.Generator().manual_seed(seed), selection=selection)


# ---------------------------------------------------------------------------------------------
# GCMC layer
# ---------------------------------------------------------------------------------------------
LayerCfg = namedtuple("LayerCfg", "shared width")
LAYER_CFGS = (LayerCfg(True, 7), LayerCfg(True, 8), LayerCfg(False, 7), LayerCfg(False, 8))
OUT_UNITS = 6
IN_DRUG = 12


def in_units(cfg):
    return (IN_DRUG, IN_DRUG if cfg.shared else 5)


def make_layer(cfg, device):
    """A ``GCMCLayer`` (agg 'sum', LeakyReLU(0.25) passed as a module, dropout 0.5) with designed parameters.  Width 7 is
    reached as layer 0 is (``ini=True``: 21 // 3) and takes the pad to 8; width 8 takes none."""
    from dream_gnn_amd import layers as L

    ind, ins = in_units(cfg)
    layer = L.GCMCLayer([0, 1], ind, ins, 21 if cfg.width == 7 else 8, OUT_UNITS, dropout_rate=P_DROP, agg="sum",
                        agg_act=nn.LeakyReLU(SLOPE), ini=cfg.width == 7, share_user_item_param=cfg.shared, basis_units=2)
    assert layer.msg_units == cfg.width and (layer.W_r is not None) == cfg.shared
    rng = np.random.default_rng(100 + 10 * cfg.width + cfg.shared)
    with torch.no_grad():
        for name, p in layer.named_parameters():
            if name.endswith("bias"):
                v = ints(rng, tuple(p.shape))
            elif name == "att":
                v = np.array([[1.0, 0.0], [-1.0, 2.0]], np.float32)
            else:
                v = sparse_ints(rng, tuple(p.shape), 0.2 if name == "basis" else 0.3)
            p.copy_(torch.from_numpy(v))
    return layer.to(device)


def gcmc_inputs(design, cfg):
    rng = np.random.default_rng(200 + cfg.width)
    ind, ins = in_units(cfg)
    t = lambda a: torch.from_numpy(a)
    return dict(x_drug=t(ints(rng, (design.n_drug, ind))), x_dis=t(ints(rng, (design.n_dis, ins))),
                g_drug=t(ints(rng, (design.n_drug, OUT_UNITS))), g_dis=t(ints(rng, (design.n_dis, OUT_UNITS))))


def replay_gcmc_draws(graph, cfg, device, seed, train):
    """The layer's dropout draws replayed with torch's own consumer on the same device, in the documented order: one
    ``F.dropout(cj, 0.5, True)`` per relation in canonical order, then the layer masks, drug then disease, of shape
    ``(n_dst, width)`` UNPADDED.  Returns (drops, masks, generator state afterwards); eval: ``cj`` itself and no masks."""
    torch.manual_seed(seed)
    drops, masks = {}, {"drug": None, "disease": None}
    for can in graph.canonical_etypes:
        cj = graph[can].srcdata["cj"]
        drops[can] = (F.dropout(cj, P_DROP, True) if train else cj).reshape(-1).cpu().double()
    if train:
        for nt in ("drug", "disease"):
            ones = torch.ones((graph.number_of_nodes(nt), cfg.width), dtype=torch.float32, device=device)
            masks[nt] = (F.dropout(ones, P_DROP, True) != 0).cpu().double()
    return drops, masks, rng_state(device)


def gcmc_reference(design, cfg, params, x, g, kept, drops, masks, dtype=torch.float64, taps=None):
    """Per destination type ``ci . sum_r A_r^kept (drop_r . X W_r)``, the leaky ReLU, ``mask . 2``, the Linear; the loss
    ``(out . G).sum()``; outputs and the gradient of every parameter and of both inputs, from the COO triplets and dense
    per-relation count matrices alone.  ``kept``: relation -> 0/1 over its edges (None: all); ``drops``: relation ->
    the values ``dropout(cj)`` took; ``masks``: node type -> 0/1 (n, width) or None.  ``dtype=torch.float32``: the same
    expression in fp32 (no exactness check of its own)."""
    n = {"drug": design.n_drug, "disease": design.n_dis}
    edges, scales = relation_edges(design), node_scales(design)
    pr = Products(GRAN_GCMC, "gcmc " + design.name)
    P = {k: v.detach().cpu().to(dtype).clone().requires_grad_(True) for k, v in params.items()}
    X = {nt: x[nt].detach().cpu().to(dtype).clone().requires_grad_(True) for nt in x}
    W = None
    if cfg.shared:
        W = pr.mm(P["att"], P["basis"].view(2, -1)).view(2, in_units(cfg)[0], cfg.width)
    dense = int(np.argmax([(design.label == r).sum() for r in range(2)]))  # the relation a complement form rewrites
    out = {}
    for nt_dst, nt_src in (("drug", "disease"), ("disease", "drug")):
        acc = None
        for r, name in enumerate(REL_NAMES):
            can = (nt_src, name if nt_src == "drug" else "rev-" + name, nt_dst)
            src, dst = edges[can]
            k = torch.ones(src.size, dtype=dtype) if kept is None else torch.from_numpy(np.asarray(kept[can])).to(dtype)
            A = torch.zeros((n[nt_dst], n[nt_src]), dtype=dtype)
            A.index_put_((torch.from_numpy(dst), torch.from_numpy(src)), k, accumulate=True)  # duplicates sum
            w = W[r] if cfg.shared else P["conv.mods.%s.weight" % can[1]]
            h = pr.keep(pr.mm(X[nt_src], w) * drops[can].to(dtype).reshape(-1, 1))
            m = pr.mm(A, h, a_bound=A + 2.0 if r == dense else None)
            acc = m if acc is None else pr.keep(acc + m)
        y = pr.keep(acc * torch.from_numpy(scales[nt_dst]["ci"]).to(dtype))
        y = pr.keep(F.leaky_relu(y, SLOPE))
        if masks[nt_dst] is not None:
            y = pr.keep(y * masks[nt_dst].to(dtype) * 2.0)
        lin = "ufc" if (cfg.shared or nt_dst == "disease") else "ifc"
        if taps is not None:  # the operands of the second-stage GEMM, for the premise check of the GPU file
            taps[nt_dst] = (y.detach(), P[lin + ".weight"].detach(), P[lin + ".bias"].detach())
        out[nt_dst] = pr.keep(pr.mm(y, P[lin + ".weight"].t()) + P[lin + ".bias"])
    loss = (out["drug"] * g["drug"].cpu().to(dtype)).sum() + (out["disease"] * g["disease"].cpu().to(dtype)).sum()
    loss.backward()
    res = {"out_drug": out["drug"].detach(), "out_dis": out["disease"].detach(), "x_drug.grad": X["drug"].grad,
           "x_dis.grad": X["disease"].grad}
    for k, p in P.items():
        if p.grad is not None:
            res["grad/" + k] = p.grad
    if dtype == torch.float64:
        pr.check(res.values())
    return res


FORMS = {  # GCMCLayer class attributes per evaluation form
    "slice": dict(fuse_relations=False, fuse_epilogue=True, complement_form=False),
    "fused": dict(fuse_relations=True, fuse_epilogue=False, complement_form=False),
    "fused_epi": dict(fuse_relations=True, fuse_epilogue=True, complement_form=False),
    "complement": dict(fuse_relations=True, fuse_epilogue=False, complement_form=True),
    "complement_epi": dict(fuse_relations=True, fuse_epilogue=True, complement_form=True),
}


def set_form(monkeypatch, form):
    from dream_gnn_amd import layers as L

    for k, v in FORMS[form].items():
        monkeypatch.setattr(L.GCMCLayer, k, v)


def run_gcmc(layer, graph, inp, device, train, seed):
    """One forward + backward of the layer under ``torch.manual_seed(seed)``: the reference's keys, as CPU tensors."""
    layer.train(train)
    layer.zero_grad(set_to_none=True)
    xd = inp["x_drug"].to(device).clone().requires_grad_(True)
    xs = inp["x_dis"].to(device).clone().requires_grad_(True)
    torch.manual_seed(seed)
    od, os_ = layer(graph, xd, xs)
    ((od * inp["g_drug"].to(device)).sum() + (os_ * inp["g_dis"].to(device)).sum()).backward()
    res = {"out_drug": od.detach().cpu(), "out_dis": os_.detach().cpu(), "x_drug.grad": xd.grad.cpu(), "x_dis.grad": xs.grad.cpu()}
    for k, p in layer.named_parameters():
        res["grad/" + k] = None if p.grad is None else p.grad.cpu()
    return res, rng_state(device)


def same(got, want):
    """Every tensor of ``want`` equal in ``got`` (zeros by value); a gradient the reference does not have is None or 0."""
    bad = []
    for k in set(got) | set(want):
        a, b = got.get(k), want.get(k)
        if b is None:
            if a is not None and bool(a.any()):
                bad.append(k)
        elif a is None or a.shape != b.shape or not torch.equal(a.double(), b.double()):
            bad.append(k)
    return sorted(bad)


# ---------------------------------------------------------------------------------------------
# decoder
# ---------------------------------------------------------------------------------------------
DEC_N_DRUG, DEC_N_DIS, DEC_IN = 29, 31, 6
DEC_E = (1, 50, 5 * 64 + 17)


def decoder_edges(E):
    """Edge lists that repeat pairs, name node 0 and the last node of each side and leave one node of each side unnamed
    (E = 1: the pair (0, last))."""
    import _edge_cases as EC

    src, dst = EC.edge_pairs(E, DEC_N_DRUG, DEC_N_DIS)
    return src.astype(np.int64), dst.astype(np.int64)


def make_decoder(device):
    from dream_gnn_amd import model as M

    dec = M.MLPDecoder(DEC_IN, dropout_rate=P_DROP)
    rng = np.random.default_rng(300)
    with torch.no_grad():
        for name, p in dec.named_parameters():
            dens = {"lin1.weight": 0.4, "lin2.weight": 0.08, "lin3.weight": 0.3}.get(name)
            p.copy_(torch.from_numpy(ints(rng, tuple(p.shape)) if dens is None else sparse_ints(rng, tuple(p.shape), dens)))
    return dec.to(device)


def decoder_inputs(E):
    rng = np.random.default_rng(400 + E)
    t = lambda a: torch.from_numpy(a)
    return dict(hd=t(ints(rng, (DEC_N_DRUG, DEC_IN))), hs=t(ints(rng, (DEC_N_DIS, DEC_IN))), g=t(ints(rng, (E, 1))))


def replay_decoder_draws(E, device, seed, train):
    """Every form of the decoder draws the same two tensors from the stream: ``dropout`` over (E, 128), then over (E, 64)."""
    torch.manual_seed(seed)
    if not train:
        return None, None, rng_state(device)
    m = [(F.dropout(torch.ones((E, w), dtype=torch.float32, device=device), P_DROP, True) != 0).cpu().double() for w in (128, 64)]
    return m[0], m[1], rng_state(device)


def decoder_reference(params, inp, src, dst, m1, m2, dtype=torch.float64, taps=None):
    """float64 autograd of ``lin3(drop(relu(lin2(drop(relu(lin1(cat(hd[src], hs[dst]))))))))`` with the masks passed in
    (the gather written as a product with the 0/1 incidence matrix, so that its gradient's segment sums are bounded too)."""
    pr = Products(GRAN_DEC, "decoder")
    P = {k: v.detach().cpu().to(dtype).clone().requires_grad_(True) for k, v in params.items()}
    hd = inp["hd"].to(dtype).clone().requires_grad_(True)
    hs = inp["hs"].to(dtype).clone().requires_grad_(True)
    E = src.size
    Sd, Ss = torch.zeros((E, DEC_N_DRUG), dtype=dtype), torch.zeros((E, DEC_N_DIS), dtype=dtype)
    Sd[torch.arange(E), torch.from_numpy(src)] = 1.0
    Ss[torch.arange(E), torch.from_numpy(dst)] = 1.0
    h = pr.keep(torch.cat([pr.mm(Sd, hd), pr.mm(Ss, hs)], 1))
    for lin, m in (("lin1", m1), ("lin2", m2)):
        if taps is not None:
            taps[lin] = (h.detach(), P[lin + ".weight"].detach(), P[lin + ".bias"].detach())
        h = pr.keep(torch.relu(pr.keep(pr.mm(h, P[lin + ".weight"].t()) + P[lin + ".bias"])))
        if m is not None:
            h = pr.keep(h * m.to(dtype) * 2.0)
    if taps is not None:
        taps["lin3"] = (h.detach(), P["lin3.weight"].detach(), P["lin3.bias"].detach())
    out = pr.keep(pr.mm(h, P["lin3.weight"].t()) + P["lin3.bias"])
    (out * inp["g"].to(dtype)).sum().backward()
    res = {"out": out.detach(), "hd.grad": hd.grad, "hs.grad": hs.grad}
    res.update({"grad/" + k: p.grad for k, p in P.items()})
    if dtype == torch.float64:
        pr.check(res.values())
    return res


def run_decoder(dec, graph, inp, device, train, seed):
    dec.train(train)
    dec.zero_grad(set_to_none=True)
    hd = inp["hd"].to(device).clone().requires_grad_(True)
    hs = inp["hs"].to(device).clone().requires_grad_(True)
    torch.manual_seed(seed)
    out = dec(graph, hd, hs)
    (out * inp["g"].to(device)).sum().backward()
    res = {"out": out.detach().cpu(), "hd.grad": hd.grad.cpu(), "hs.grad": hs.grad.cpu()}
    res.update({"grad/" + k: p.grad.cpu() for k, p in dec.named_parameters()})
    return res, rng_state(device)


# ---------------------------------------------------------------------------------------------
# adjacency
# ---------------------------------------------------------------------------------------------
ADJ_N, ADJ_IN, ADJ_HID, ADJ_OUT = 96, 10, 8, 4
ADJ_HUB = 0
GRAN_ADJ = 2.0 ** -14          # (1/128)^2 over two products, dropout scale 2 an integer


def adjacency_edges(salt=0):
    """Directed unit edges (rows, cols) of a 0/1 neighbour matrix ``A`` on 96 nodes such that every row sum of
    ``M = A + A^T + I`` is a power of two — 4, 8 or 16, and 128 for the hub (node 0, joined to all 95 others: a row of 96
    entries cannot sum to 16) — so that ``D^-1 M`` holds powers of two times a multiplicity in 1..3 (a self-neighbour
    makes the diagonal 3).  Returns (rows, cols, M)."""
    n = ADJ_N
    rng = np.random.default_rng(500 + salt)
    w = np.zeros((n, n), np.int64)                      # off-diagonal A_ij + A_ji
    two = rng.permutation(np.arange(1, n))[:32]         # 63 x 1 + 32 x 2 = 127 = 128 - 1
    w[0, 1:] = 1
    w[0, two] = 2
    w[1:, 0] = w[0, 1:]
    target = np.array([128] + [(4, 8, 16)[(i + salt) % 3] for i in range(1, n)])
    need = target - 1 - w.sum(1)
    preset = (np.arange(n) % 10 == 3) & (target >= 8) & (target < 128)   # self-neighbours: diagonal 3
    need[preset] -= 2
    assert need[0] == 0 and (need[1:] >= 1).all()
    for i in rng.permutation(np.arange(1, n)):
        for j in sorted((j for j in range(1, n) if j != i and w[i, j] == 0 and need[j] > 0), key=lambda j: -need[j]):
            if need[i] <= 0:
                break
            x = min(2, need[i], need[j])
            w[i, j] = w[j, i] = x
            need[i] -= x
            need[j] -= x
    self_loop = (need == 2) & ~preset                   # a self-neighbour adds 2 to the row sum
    need[self_loop] = 0
    self_loop |= preset
    assert (need == 0).all(), need
    a = np.zeros((n, n), np.int64)
    iu, ju = np.nonzero(np.triu(w, 1))
    for k, (i, j) in enumerate(zip(iu, ju)):
        if w[i, j] == 2:
            a[i, j] = a[j, i] = 1
        elif k % 2:
            a[i, j] = 1
        else:
            a[j, i] = 1
    a[np.flatnonzero(self_loop), np.flatnonzero(self_loop)] = 1
    M = a + a.T + np.eye(n, dtype=np.int64)
    rows, cols = np.nonzero(a)
    order = rng.permutation(rows.size)
    return rows[order], cols[order], M


def build_adjacency(device, salt=0):
    from dream_gnn_amd import graph as G

    rows, cols, M = adjacency_edges(salt)
    adj = G._normalized_adjacency(torch.from_numpy(rows).to(device), torch.from_numpy(cols).to(device), ADJ_N, True)
    return adj, M


def make_gcn(device):
    from dream_gnn_amd import layers as L

    gcn = L.GCN(ADJ_IN, ADJ_HID, ADJ_OUT, P_DROP)
    rng = np.random.default_rng(600)
    with torch.no_grad():
        for name, p in gcn.named_parameters():
            p.copy_(torch.from_numpy(ints(rng, tuple(p.shape)) if name.endswith("bias") else sparse_ints(rng, tuple(p.shape), 0.3)))
    return gcn.to(device)


def adjacency_inputs():
    rng = np.random.default_rng(700)
    t = lambda a: torch.from_numpy(a)
    return dict(x=t(ints(rng, (ADJ_N, ADJ_IN))), g1=t(ints(rng, (ADJ_N, ADJ_HID))), g2=t(ints(rng, (ADJ_N, ADJ_OUT))))


def _dense(idx, val, alive, dtype):
    A = torch.zeros((ADJ_N, ADJ_N), dtype=dtype)
    v = val.to(dtype) if alive is None else val.to(dtype) * torch.as_tensor(alive).to(dtype)
    return A.index_put_((idx[0], idx[1]), v, accumulate=True)


def adjacency_reference(params, inp, idx, val, alive, mask, which, dtype=torch.float64):
    """Dense float64 ``adj @ (x @ W) + b`` over the surviving entries (``which == "conv"``: GraphConvolution gc1 alone) or
    the whole ``GCN`` (``"gcn"``: relu, the dropout mask passed in, the second convolution), and the gradients."""
    pr = Products(GRAN_ADJ, "adjacency")
    P = {k: v.detach().cpu().to(dtype).clone().requires_grad_(True) for k, v in params.items()}
    x = inp["x"].to(dtype).clone().requires_grad_(True)
    A = _dense(idx, val, alive, dtype)
    h = pr.keep(pr.mm(A, pr.mm(x, P["gc1.weight"])) + P["gc1.bias"])
    if which == "conv":
        out, g = h, inp["g1"]
    else:
        h = pr.keep(torch.relu(h))
        if mask is not None:
            h = pr.keep(h * mask.to(dtype) * 2.0)
        out, g = pr.keep(pr.mm(A, pr.mm(h, P["gc2.weight"])) + P["gc2.bias"]), inp["g2"]
    (out * g.to(dtype)).sum().backward()
    res = {"out": out.detach(), "x.grad": x.grad}
    res.update({"grad/" + k: p.grad for k, p in P.items() if p.grad is not None})
    if dtype == torch.float64:
        pr.check(res.values())
    return res


def run_adjacency(gcn, adj, inp, device, which, train, seed):
    """``which == "conv"``: ``gcn.gc1(x, adj)``; ``"gcn"``: ``gcn.from_support(x @ gc1.weight, adj)``."""
    gcn.train(train)
    gcn.zero_grad(set_to_none=True)
    x = inp["x"].to(device).clone().requires_grad_(True)
    torch.manual_seed(seed)
    if which == "conv":
        out, g = gcn.gc1(x, adj), inp["g1"]
    else:
        out, g = gcn.from_support(torch.mm(x, gcn.gc1.weight), adj), inp["g2"]
    (out * g.to(device)).sum().backward()
    res = {"out": out.detach().cpu(), "x.grad": x.grad.cpu()}
    res.update({"grad/" + k: (None if p.grad is None else p.grad.cpu()) for k, p in gcn.named_parameters()})
    return res, rng_state(device)


def replay_gcn_draw(device, seed, train):
    torch.manual_seed(seed)
    if not train:
        return None
    return (F.dropout(torch.ones((ADJ_N, ADJ_HID), dtype=torch.float32, device=device), P_DROP, True) != 0).cpu().double()


ADJ_KINDS = ("tensor", "dropped_tensor", "tensor_of_tensor", "view_select", "view_randperm", "dropout_of_select_view",
             "dropout_of_mask_view", "dropout_of_tensor_view")


def dropped_adjacency(kind, adj, oracle, seed):
    """(what the module is handed, 0/1 survivors over the entries of ``adj`` in their stored order) for each kind of
    dropped adjacency, the survivors replayed on the host from a generator seeded alike."""
    from dream_gnn_amd import graph as G

    E = int(adj._values().shape[0])
    gen, rep = torch.Generator().manual_seed(seed), torch.Generator().manual_seed(seed)
    keep_of = lambda e: max(1, int(e * (1 - EDGE_DROP)))

    def perm_mask(positions, e):  # randperm(e)[:keep] among `positions` of the root's entries
        sel = torch.randperm(e, generator=rep)[:keep_of(e)].numpy()
        m = np.zeros(E)
        m[positions[sel]] = 1.0
        return m

    def select_mask():
        s = int(torch.randint(0, 2 ** 62, (1,), generator=rep).item())
        return np.asarray(oracle.random_subset_mask(E, keep_of(E), s), np.float64)

    every = np.arange(E)
    if kind == "tensor":
        return adj, None
    if kind == "dropped_tensor":
        return G.random_edge_dropout_sparse(adj, EDGE_DROP, generator=gen), perm_mask(every, E)
    if kind == "tensor_of_tensor":
        once = G.random_edge_dropout_sparse(adj, EDGE_DROP, generator=gen)
        first = torch.randperm(E, generator=rep)[:keep_of(E)].numpy()        # entry k of `once` is entry first[k] of the root
        twice = G.random_edge_dropout_sparse(once, EDGE_DROP, generator=gen)
        return twice, perm_mask(first, first.size)
    if kind == "view_select":
        return G.random_edge_dropout_sparse(adj, EDGE_DROP, generator=gen, as_view=True, selection="select"), select_mask()
    if kind == "view_randperm":
        return G.random_edge_dropout_sparse(adj, EDGE_DROP, generator=gen, as_view=True, selection="randperm"), perm_mask(every, E)
    if kind == "dropout_of_select_view":
        view = G.random_edge_dropout_sparse(adj, EDGE_DROP, generator=gen, as_view=True, selection="select")
        alive = np.flatnonzero(select_mask())
    elif kind == "dropout_of_mask_view":
        view = G.random_edge_dropout_sparse(adj, EDGE_DROP, generator=gen, as_view=True, selection="randperm")
        alive = np.flatnonzero(perm_mask(every, E))
    elif kind == "dropout_of_tensor_view":
        from dream_gnn_amd import layers as L

        view = L.adjacency_csr(G.random_edge_dropout_sparse(adj, EDGE_DROP, generator=gen))
        alive = np.flatnonzero(perm_mask(every, E))
    else:
        raise ValueError(kind)
    # a dropout of a dropped view keeps an exact count of the SURVIVORS, in ascending order of their positions
    return G.random_edge_dropout_sparse(view, EDGE_DROP, generator=gen, as_view=True), perm_mask(alive, alive.size)


# ---------------------------------------------------------------------------------------------
# the checks, shared by the host file (CPU backend) and the GPU file
# ---------------------------------------------------------------------------------------------
GRAPH_KINDS = ("full", "select", "randperm")
EDGE_SEED, DRAW_SEED = 77, 5


def enc_graph_of_kind(graph, design, oracle, kind):
    """(graph the layer is handed, kept-edge masks replayed on the host or None); for a dropped child the host masks
    must be what its descriptions (``oracle.keep_mask``) or its permutation prefix say."""
    if kind == "full":
        return graph, None
    child = dropped_enc_graph(graph, kind, EDGE_SEED)
    kept = replay_edge_dropout(design, oracle, kind, EDGE_SEED)
    for can in CANS:
        rel, E = child[can], int(kept[can].size)
        assert rel.number_of_edges() == int(kept[can].sum())
        if kind == "select":
            assert rel.desc is not None and np.array_equal(oracle.keep_mask(rel.desc.cpu().numpy(), E), kept[can])
        else:
            assert rel.desc is None and np.array_equal(rel.keep_mask().cpu().numpy(), kept[can])
    return child, kept


def check_gcmc(monkeypatch, oracle, device, design, cfg, forms=tuple(FORMS), kinds=GRAPH_KINDS, modes=(False, True), hook=None):
    """Every form x mode x graph kind of one design and layer layout: outputs and all gradients ``torch.equal`` to the
    reference (hence to each other), the generator left where the replay left it.  Returns the number of runs."""
    graph = build_enc_graph(design, device)
    layer = make_layer(cfg, device)
    params = {k: p.detach().cpu().clone() for k, p in layer.named_parameters()}
    inp = gcmc_inputs(design, cfg)
    x = {"drug": inp["x_drug"], "disease": inp["x_dis"]}
    g = {"drug": inp["g_drug"], "disease": inp["g_dis"]}
    runs = 0
    for kind in kinds:
        gr, kept = enc_graph_of_kind(graph, design, oracle, kind)
        for train in modes:
            drops, masks, state = replay_gcmc_draws(gr, cfg, device, DRAW_SEED, train)
            want = gcmc_reference(design, cfg, params, x, g, kept, drops, masks)
            for form in forms:
                set_form(monkeypatch, form)
                got, after = run_gcmc(layer, gr, inp, device, train, DRAW_SEED)
                bad = same(got, want)
                assert not bad, (design.name, cfg, kind, "train" if train else "eval", form, bad)
                assert torch.equal(after, state), (design.name, cfg, kind, train, form, "generator state")
                runs += 1
                if hook is not None:
                    hook(form, kind, train, graph, gr, layer)
    return runs


DECODER_FORMS = (False, True)  # MLPDecoder.fuse_lin1


def check_decoder(monkeypatch, device, E, min_rows=None, chunk=None):
    """fuse_lin1 off / on x eval / train at one edge count; ``min_rows`` / ``chunk``: patched ``_EdgeLinear`` gates."""
    from dream_gnn_amd import graph as G, model as M

    if min_rows is not None:
        monkeypatch.setattr(M._EdgeLinear, "MIN_ROWS", min_rows)
        monkeypatch.setattr(M._EdgeLinear, "CHUNK", chunk)
    src, dst = decoder_edges(E)
    graph = G.build_dec_graph(torch.from_numpy(src), torch.from_numpy(dst), DEC_N_DRUG, DEC_N_DIS, device=device).int()
    dec = make_decoder(device)
    params = {k: p.detach().cpu().clone() for k, p in dec.named_parameters()}
    inp = decoder_inputs(E)
    runs = 0
    for train in (False, True):
        m1, m2, state = replay_decoder_draws(E, device, DRAW_SEED, train)
        want = decoder_reference(params, inp, src, dst, m1, m2)
        for fuse in DECODER_FORMS:
            monkeypatch.setattr(M.MLPDecoder, "fuse_lin1", fuse)
            got, after = run_decoder(dec, graph, inp, device, train, DRAW_SEED)
            bad = same(got, want)
            assert not bad, (E, "train" if train else "eval", "fuse_lin1=%s" % fuse, min_rows, bad)
            assert torch.equal(after, state)
            runs += 1
    return runs


def check_adjacency(oracle, device, kinds=ADJ_KINDS, hook=None):
    """GraphConvolution (eval) and GCN.from_support (train) on every kind of dropped adjacency."""
    adj, _ = build_adjacency(device)
    adj = adj.coalesce() if not adj.is_coalesced() else adj
    gcn = make_gcn(device)
    params = {k: p.detach().cpu().clone() for k, p in gcn.named_parameters()}
    inp = adjacency_inputs()
    idx, val = adj._indices().cpu(), adj._values().cpu()
    runs = 0
    for kind in kinds:
        handed, alive = dropped_adjacency(kind, adj, oracle, EDGE_SEED)
        for which, train in (("conv", False), ("gcn", True), ("gcn", False)):
            mask = replay_gcn_draw(device, DRAW_SEED, train and which == "gcn")
            want = adjacency_reference(params, inp, idx, val, alive, mask, which)
            got, _ = run_adjacency(gcn, handed, inp, device, which, train, DRAW_SEED)
            bad = same(got, want)
            assert not bad, (kind, which, train, bad)
            runs += 1
        if hook is not None:
            hook(kind, adj, handed)
    return runs


def check_memo(monkeypatch, device, design, cfg):
    """The column-sum coefficients kept beside the graph (complement form, eval): a second call reuses the very tensors;
    ``cj`` changed in place, then replaced by a new object, is noticed; in train mode the memo is not consulted (it is
    poisoned with NaN for that call)."""
    set_form(monkeypatch, "complement_epi")
    graph = build_enc_graph(design, device)
    layer = make_layer(cfg, device)
    params = {k: p.detach().cpu().clone() for k, p in layer.named_parameters()}
    inp = gcmc_inputs(design, cfg)
    x = {"drug": inp["x_drug"], "disease": inp["x_dis"]}
    g = {"drug": inp["g_drug"], "disease": inp["g_dis"]}

    def both(train):
        drops, masks, _ = replay_gcmc_draws(graph, cfg, device, DRAW_SEED, train)
        want = gcmc_reference(design, cfg, params, x, g, None, drops, masks)
        got, _ = run_gcmc(layer, graph, inp, device, train, DRAW_SEED)
        return same(got, want)

    assert not both(False)
    memo = dict(graph._complement_memo)
    assert set(memo) == {"drug", "disease"}
    assert not both(False)
    assert all(graph._complement_memo[nt][1] is memo[nt][1] and graph._complement_memo[nt][2] is memo[nt][2] for nt in memo)
    graph.nodes["drug"].data["cj"].mul_(2)                       # in place: same object, another version
    assert not both(False), "cj changed in place"
    assert graph._complement_memo["disease"][1] is not memo["disease"][1]   # drug cj feeds the products that END in disease
    old = graph.nodes["disease"].data["cj"]
    graph.nodes["disease"].data["cj"] = torch.where(old == 0.25, torch.ones_like(old), old)   # a new object, other values
    assert not both(False), "cj replaced"
    poisoned = {}
    for nt, (key, coef, scale, cjs) in graph._complement_memo.items():
        poisoned[nt] = (key, torch.full_like(coef, float("nan")), torch.full_like(scale, float("nan")), cjs)
    graph.__dict__["_complement_memo"] = dict(poisoned)
    assert not both(True), "train mode"
    assert all(graph._complement_memo[nt] is poisoned[nt] for nt in poisoned)
    del graph.__dict__["_complement_memo"]
    assert not both(False)


def check_complement_structure(graph, child, design):
    """A ``select`` child in complement form: a view of the PARENT's structure whose description table holds relation
    i's edge offset in words 0 and 1 and the invert bit (word 6) for relation i0 alone."""
    for nt in ("drug", "disease"):
        view, cans, i0, _ = child.fused_relations_complement(nt)
        struct = graph._complement_struct(nt, True)
        assert i0 == design.props["i0"] and view.indptr is struct[0].indptr and view.nnz == struct[0].nnz
        table = view._keep.cpu().numpy()
        assert table.shape == (len(cans), 8)
        start = 0
        for i, can in enumerate(cans):
            desc = child[can].desc.cpu().numpy()
            E = graph[can].number_of_edges()
            assert struct[4][i] == start and table[i, 0] == start and table[i, 1] == start + E
            assert table[i, 6] == (1 if i == i0 else 0) and desc[6] == 0
            assert np.array_equal(table[i, 2:6], desc[2:6]) and table[i, 7] == desc[7]
            start += E


def check_adjacency_views(oracle, device, hook=None):
    """``random_edge_dropout_sparse_views`` on two adjacencies: one seed per graph, in the given order."""
    from dream_gnn_amd import graph as G

    adjs = [build_adjacency(device, salt)[0] for salt in (0, 1)]
    gcn = make_gcn(device)
    params = {k: p.detach().cpu().clone() for k, p in gcn.named_parameters()}
    inp = adjacency_inputs()
    views = G.random_edge_dropout_sparse_views(adjs, EDGE_DROP, generator=torch.Generator().manual_seed(EDGE_SEED), selection="select")
    rep = torch.Generator().manual_seed(EDGE_SEED)
    for adj, view in zip(adjs, views):
        E = int(adj._values().shape[0])
        s = int(torch.randint(0, 2 ** 62, (1,), generator=rep).item())
        alive = np.asarray(oracle.random_subset_mask(E, max(1, int(E * (1 - EDGE_DROP))), s), np.float64)
        for which, train in (("conv", False), ("gcn", True)):
            mask = replay_gcn_draw(device, DRAW_SEED, train)
            want = adjacency_reference(params, inp, adj._indices().cpu(), adj._values().cpu(), alive, mask, which)
            got, _ = run_adjacency(gcn, view, inp, device, which, train, DRAW_SEED)
            bad = same(got, want)
            assert not bad, ("views", which, bad)
        if hook is not None:
            hook("views", adj, view)
