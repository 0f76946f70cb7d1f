"""The plain CSR SpMM (a wave per row, and per item of a launch plan: csrc/dgmi_spmm.hip, dgmi_segment.h, dgmi_plan.hip)
on the designed integer operands of _csr_cases.py, ZERO tolerance: ``torch.equal`` against the integer reference, so empty
and fully dropped rows are exactly 0 and no Inf / NaN behind a dropped edge reaches an output.  (a) every kernel form
and width, (b) dropped / kept edges on chosen lanes of chosen id batches under every kind of description table, (c) the
plan buffer word for word, (d) the grid strides of the reduce pass and the plan builders, (e) the same through
``CSRGraph``."""
import itertools

import numpy as np
import pytest
import torch

import _csr_cases as C

pytestmark = pytest.mark.gpu

FORMS = list(itertools.product((False, True), (False, True), (False, True)))  # value stream, src_scale, dropout on the fly
FORM_IDS = ["%s%s%s" % ("vals" if v else "unit", "-ss" if s else "", "-keep" if k else "") for v, s, k in FORMS]
COMBOS = list(itertools.product((False, True), (False, True)))                # dst_scale, epilogue
OTHER_WIDTHS = [F for F in C.VEC4_WIDTHS + C.DWORD_WIDTHS if F not in C.FORM_WIDTHS]
VIEWS = ("x_off_16_bytes", "x_odd_row_stride", "mask_off_16_bytes")           # F = 128 through the dword kernel


def _t(a, dev):
    return None if a is None else torch.from_numpy(np.array(a)).to(dev)  # a copy: the designs are read-only


_staged = {}


def _stage(oracle, dev, key, d, desc=None):
    """A design on the device, once: the CSR (checked against the oracle's), the values in CSR order, the plans, the
    subset descriptions (checked against the host mask)."""
    from dream_gnn_amd import ops

    if key not in _staged:
        E = d.dst.size
        g = ops.CSRGraph(_t(d.dst, dev), _t(d.src, dev), d.n_dst, d.n_src, vals=_t(d.vals, dev))
        indptr, indices, eid = oracle.csr_from_coo(d.dst, d.src, d.n_dst)
        assert np.array_equal(g.indptr.cpu().numpy(), indptr) and np.array_equal(g.indices.cpu().numpy(), indices)
        assert np.array_equal(g.eid.cpu().numpy(), eid)
        if desc is None:
            desc = ops.random_subset_select(E, int(E * C.DROP_KEEP), C.DROP_SEED, dev)
        else:
            desc = _t(desc, dev)
        desc = ops._prep_keep(desc)  # (n, 8)
        assert np.array_equal(ops.keep_mask(desc, E).cpu().numpy().astype(bool), d.kept)
        _staged[key] = dict(d=d, g=g, gu=g.with_values(None), desc=desc, vals=g.vals.contiguous(), ss=_t(d.ss, dev), ds=_t(d.ds, dev),
                            plans={"none": None, "default": g.plan, 16: ops.build_plan(g.indptr, g.nnz, chunk=16),
                                   64: ops.build_plan(g.indptr, g.nnz, chunk=64)})
    return _staged[key]


def _differs(y, want):
    bad = (y != want) | torch.isnan(y)
    return "%d elements differ, first row %d" % (int(bad.sum()), int(bad.any(1).nonzero()[0])) if bool(bad.any()) else ""


def _forms(oracle, dev, F, form, plans=("none", "default", 16), view=None):
    """One kernel form at one width on ``plain_design()``: every plan, with and without ``dst_scale`` and the mask + leaky
    epilogue, against the integer reference."""
    from dream_gnn_amd import ops

    st = _stage(oracle, dev, "plain", C.plain_design())
    d, g = st["d"], st["g"]
    has_vals, has_ss, dropped = form
    seed = 11 * F + 1
    X, mask = C.features(d.n_src, F, seed), C.out_mask(d.n_dst, F, seed + 1)
    combos = [c for c in COMBOS if c[1]] if view == "mask_off_16_bytes" else COMBOS
    want = {(has_ds, epi): _t(C.reference(d.dst, d.src, d.n_dst, X, d.vals if has_vals else None, d.ss if has_ss else None,
                                          d.ds if has_ds else None, d.kept if dropped else None, mask if epi else None, epi), dev)
            for has_ds, epi in combos}
    empty = torch.tensor(C.PLAIN_EMPTY, device=dev)
    assert all(bool((y[empty] == 0).all()) and bool(torch.isfinite(y).all()) for y in want.values())
    # Inf / NaN in the source rows that only dropped edges read
    Xd, mask_d = _t(C.features(d.n_src, F, seed, dead=d.dead) if dropped else X, dev), _t(mask, dev)
    if view == "x_off_16_bytes":       # rows of a wider tensor, one float off a 16-byte boundary
        wide = torch.zeros(d.n_src, F + 4, device=dev)
        wide[:, 1:F + 1] = Xd
        Xd = wide[:, 1:F + 1]
        assert Xd.data_ptr() % 16 == 4 and Xd.stride(0) % 4 == 0
    elif view == "x_odd_row_stride":   # ldx = 131
        wide = torch.zeros(d.n_src, F + 3, device=dev)
        wide[:, :F] = Xd
        Xd = wide[:, :F]
        assert Xd.data_ptr() % 16 == 0 and Xd.stride(0) % 4 == 3
    elif view == "mask_off_16_bytes":  # an aligned X, the epilogue's mask off a 16-byte boundary
        wide = torch.zeros(d.n_dst, F + 4, device=dev)
        wide[:, 1:F + 1] = mask_d
        mask_d = wide[:, 1:F + 1]
        assert mask_d.data_ptr() % 16 == 4 and Xd.data_ptr() % 16 == 0
    for name in plans:
        for has_ds, epi in combos:
            y = ops._launch_spmm(dev, g.indptr, g.indices, st["vals"] if has_vals else None, Xd, st["ss"] if has_ss else None,
                                 st["ds"] if has_ds else None, None, st["plans"][name], d.n_dst, d.n_src, F, F, eid=g.eid,
                                 keep=st["desc"] if dropped else None, epi=(1, C.SLOPE, mask_d, C.MASK_SCALE) if epi else None)
            assert torch.equal(y, want[has_ds, epi]), "plan %s dst_scale=%s epilogue=%s: %s" % (
                name, has_ds, epi, _differs(y, want[has_ds, epi]))


# ---------------------------------------------------------------------------------------------
# (a) kernel forms
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("F", C.FORM_WIDTHS)
@pytest.mark.parametrize("form", FORMS, ids=FORM_IDS)
def test_every_form_unplanned_and_planned(oracle, dev, form, F):
    """All eight forms (value stream x ``src_scale`` x dropout on the fly) at one width per lane-group width (8, 16, 32,
    64) and at layer 0's 341 (the dword kernel), a wave per row, under the default plan and under 16-edge chunks: rows on
    both sides of every batch edge and of every tail-batch break, a 3 000-edge row, duplicate edges."""
    _forms(oracle, dev, F, form)


@pytest.mark.parametrize("F", OTHER_WIDTHS)
@pytest.mark.parametrize("form", [FORMS[0], FORMS[-1]], ids=[FORM_IDS[0], FORM_IDS[-1]])
def test_every_other_width(oracle, dev, form, F):
    """The remaining widths for unit values and for value stream + ``src_scale`` + dropout: one column tile of one lane
    (4), ragged last column tiles (100, 344), three full tiles (768), the dword kernel at 1, 3 and 65 columns."""
    _forms(oracle, dev, F, form)


@pytest.mark.parametrize("view", VIEWS)
@pytest.mark.parametrize("form", [FORMS[0], FORMS[-1]], ids=[FORM_IDS[0], FORM_IDS[-1]])
def test_aligned_width_through_the_dword_kernel(oracle, dev, form, view):
    """F = 128 takes the dword kernel when ``X`` starts off a 16-byte boundary, when its row stride is odd, and when
    only the epilogue's mask is misaligned."""
    _forms(oracle, dev, 128, form, view=view)


# ---------------------------------------------------------------------------------------------
# (b) dropout patterns
# ---------------------------------------------------------------------------------------------
def _no_xcd_local_form(G):
    S = G._S
    assert S.sliced is None and S.sliced_t is None and S.split is None and S.split_t is None


@pytest.mark.parametrize("F", [64, 128, 341])
@pytest.mark.parametrize("weighted", [False, True], ids=["unit", "weighted"])
@pytest.mark.parametrize("kind", C.KINDS)
def test_dropout_patterns(oracle, dev, kind, weighted, F):
    """Rows whose first, middle or tail id batch is dropped whole, a row that loses every edge, one survivor per batch at
    lane 0 / lane 63, alternating lanes, a FULL batch that loses one edge, under 1, 2, 3 and 8 descriptions (disjoint,
    nested, inverted, hand-made words whose ends are pinned): a wave per row, chunks of 16 (a chunk boundary inside a
    dropped batch) and of 64 (every chunk one FULL batch), and ``CSRGraph.dropped`` forward, transposed and autograd."""
    from dream_gnn_amd import ops

    d = C.pattern_design(kind)
    st = _stage(oracle, dev, kind, d, d.desc)
    g, desc = (st["g"] if weighted else st["gu"]), st["desc"]
    w, s_np, d_np = (d.vals, d.ss, d.ds) if weighted else (None, None, None)
    ss, ds = (st["ss"], st["ds"]) if weighted else (None, None)
    X, W = C.features(d.n_src, F, F), C.features(d.n_dst, F, F + 1)
    Xd, Wd = _t(C.features(d.n_src, F, F, dead=d.dead), dev), _t(W, dev)
    y_ref = _t(C.reference(d.dst, d.src, d.n_dst, X, w, s_np, d_np, d.kept), dev)
    dx_ref = _t(C.reference(d.src, d.dst, d.n_src, W, w, d_np, s_np, d.kept), dev)
    gone = torch.tensor([d.rows["d_every_edge_dropped"], d.rows["h_single_dropped_edge"]] + list(C.PATTERN_EMPTY), device=dev)
    assert bool((y_ref[gone] == 0).all()) and bool((dx_ref[torch.tensor(d.dead, device=dev)] == 0).all())
    for name in ("none", 16, 64):
        y = ops.spmm_csr_raw(g.indptr, g.indices, g.vals, Xd, ss, ds, plan=st["plans"][name], eid=g.eid, keep=desc)
        assert torch.equal(y, y_ref), "plan %s: %s" % (name, _differs(y, y_ref))
    view = g.dropped(desc)
    y = view.spmm(Xd, ss, ds)
    assert torch.equal(y, y_ref), _differs(y, y_ref)
    dx = view.spmm_t(Wd, ss, ds)
    assert torch.equal(dx, dx_ref), _differs(dx, dx_ref)
    x = Xd.clone().requires_grad_(True)
    y = ops.spmm_csr(view, x, ss, ds)
    y.backward(Wd)
    assert torch.equal(y.detach(), y_ref) and torch.equal(x.grad, dx_ref)
    _no_xcd_local_form(view)  # these products ran the plain kernels


# ---------------------------------------------------------------------------------------------
# (c) plans
# ---------------------------------------------------------------------------------------------
def _check_plan(plan, indptr_np, chunk):
    """The plan buffer: 16 header words, ``items_cap`` items, then the long rows."""
    want = C.plan_items(indptr_np, chunk)
    words = plan.buf.view(torch.int32).cpu().numpy()
    assert words.size == C.PLAN_HEADER_WORDS + 4 * (want.items_cap + want.long_cap) and plan.chunk == chunk
    assert np.array_equal(words[:C.PLAN_HEADER_WORDS], want.header)
    items = words[C.PLAN_HEADER_WORDS:C.PLAN_HEADER_WORDS + 4 * want.items.shape[0]].reshape(-1, 4)
    assert np.array_equal(items, want.items)
    at = C.PLAN_HEADER_WORDS + 4 * want.items_cap
    assert np.array_equal(words[at:at + 4 * want.long_rows.shape[0]].reshape(-1, 4), want.long_rows)
    return want


def _planned_product(dev, g, plan, F, seed, unplanned=True):
    """Value stream, both scales: the planned (and the unplanned) product against the reference."""
    from dream_gnn_amd import ops

    X = C.features(g.n_src, F, seed)
    want = _t(C.reference(g.dst, g.src, g.n_dst, X, g.vals, g.ss, g.ds), dev)
    indptr, indices, eid = ops.csr_from_coo(_t(g.dst, dev), _t(g.src, dev), g.n_dst, g.n_src)
    vals = _t(g.vals, dev)[eid.long()].contiguous()
    for p in ((None, plan) if unplanned else (plan,)):
        y = ops.spmm_csr_raw(indptr, indices, vals, _t(X, dev), _t(g.ss, dev), _t(g.ds, dev), plan=p)
        assert torch.equal(y, want), "%s: %s" % ("unplanned" if p is None else "planned", _differs(y, want))


@pytest.mark.parametrize("design", ["chunks", "plain"])
@pytest.mark.parametrize("chunk", C.CHUNKS)
def test_plan_buffer_word_for_word_and_its_product(oracle, dev, chunk, design):
    """Header, items and long rows of ``build_plan(chunk=...)`` equal the host restatement, on rows of 1, 1, 2, 2, 3, 8, 8,
    9, 16 and 17 chunks (the reduce pass: nothing to add, a chain, one tree, tree + 1, two trees, + 1) and on the 331-row
    design; the planned product is exact at F = 128 (vec4, 64-column reduce tiles) and F = 3 (dword)."""
    from dream_gnn_amd import ops

    g = C.chunk_design(chunk) if design == "chunks" else C.plain_design()
    indptr_np = oracle.csr_from_coo(g.dst, g.src, g.n_dst)[0]
    plan = ops.build_plan(_t(indptr_np, dev), g.dst.size, chunk=chunk)
    want = _check_plan(plan, indptr_np, chunk)
    if design == "chunks":
        assert sorted(want.long_rows[:, 2].tolist()) == ([2, 2, 3, 8, 8, 9, 16, 17] if chunk < 65536 else [2])
    for F in (128, 3):
        _planned_product(dev, g, plan, F, chunk + F, unplanned=(chunk == 16))


# ---------------------------------------------------------------------------------------------
# (d) grid strides
# ---------------------------------------------------------------------------------------------
def test_reduce_pass_grid_stride(oracle, dev):
    """4 100 rows of 17 edges under 16-edge chunks: more long rows than the reduce pass's 1 024 blocks x 4 waves."""
    from dream_gnn_amd import ops

    rng = np.random.default_rng(17)
    n_dst, n_src = 4100, 50
    dst = rng.permutation(np.repeat(np.arange(n_dst), 17)).astype(np.int32)
    src = rng.integers(0, n_src, dst.size).astype(np.int32)
    vals, ss, ds = C.weights(rng, dst.size, n_src, n_dst)
    g = C.ChunkGraph(n_dst, n_src, dst, src, vals, ss, ds, None)
    indptr_np = oracle.csr_from_coo(dst, src, n_dst)[0]
    plan = ops.build_plan(_t(indptr_np, dev), dst.size, chunk=16)
    want = _check_plan(plan, indptr_np, 16)
    assert want.long_rows.shape[0] == 4100 > 1024 * 4 and want.long_cap == 4100
    _planned_product(dev, g, plan, 64, 1, unplanned=False)


def test_plan_builders_grid_stride(oracle, dev):
    """1 048 576 + 300 rows (more than the plan builders' 4 096 blocks x 256 threads), the edges confined to the first and
    last 300 rows, long rows at both ends: the plan word for word, the product exact at F = 4, unplanned and planned."""
    from dream_gnn_amd import ops

    rng = np.random.default_rng(23)
    n_dst, n_src = 4096 * 256 + 300, 100
    deg = np.zeros(n_dst, np.int64)
    deg[:300], deg[-300:] = rng.integers(0, 13, 300), rng.integers(0, 13, 300)
    deg[[2, 150, n_dst - 298, n_dst - 1]] = (40, 17, 33, 129)
    dst = rng.permutation(np.repeat(np.arange(n_dst), deg)).astype(np.int32)
    src = rng.integers(0, n_src, dst.size).astype(np.int32)
    vals, ss, ds = C.weights(rng, dst.size, n_src, n_dst)
    g = C.ChunkGraph(n_dst, n_src, dst, src, vals, ss, ds, None)
    indptr_np = oracle.csr_from_coo(dst, src, n_dst)[0]
    plan = ops.build_plan(_t(indptr_np, dev), dst.size, chunk=16)
    want = _check_plan(plan, indptr_np, 16)
    assert want.items.shape[0] > 4096 * 256 and want.long_rows[:, 0].tolist() == [2, 150, n_dst - 298, n_dst - 1]
    assert 2000 <= dst.size <= 6000
    _planned_product(dev, g, plan, 4, 2)


# ---------------------------------------------------------------------------------------------
# (e) through CSRGraph
# ---------------------------------------------------------------------------------------------
def test_plain_design_through_csrgraph(oracle, dev):
    """``CSRGraph.spmm`` / ``spmm_t`` / ``ops.spmm_csr`` backward on the 331-row design (the default plan cuts its long
    rows): unweighted, value stream, both scales, dropped on the fly, and the epilogue forward and backward."""
    from dream_gnn_amd import ops

    st = _stage(oracle, dev, "plain", C.plain_design())
    d, Gv, Gu, desc, ss, ds = st["d"], st["g"], st["gu"], st["desc"], st["ss"], st["ds"]
    F = 128
    t = lambda a: _t(a, dev)
    X, W = C.features(d.n_src, F, 1), C.features(d.n_dst, F, 2)
    X_bad = C.features(d.n_src, F, 1, dead=d.dead)
    assert Gv._S.max_deg == 3000 > Gv.plan.chunk

    def check(view, w, scaled, kept, what):
        s_np, d_np = (d.ss, d.ds) if scaled else (None, None)
        s_t, d_t = (ss, ds) if scaled else (None, None)
        Xd, Wd = t(X if kept is None else X_bad), t(W)
        y_ref = t(C.reference(d.dst, d.src, d.n_dst, X, w, s_np, d_np, kept))
        dx_ref = t(C.reference(d.src, d.dst, d.n_src, W, w, d_np, s_np, kept))
        assert torch.equal(view.spmm(Xd, s_t, d_t), y_ref), what
        assert torch.equal(view.spmm_t(Wd, s_t, d_t), dx_ref), what
        x = Xd.clone().requires_grad_(True)
        y = ops.spmm_csr(view, x, s_t, d_t)
        y.backward(Wd)
        assert torch.equal(y.detach(), y_ref) and torch.equal(x.grad, dx_ref), what
        _no_xcd_local_form(view)

    check(Gu, None, False, None, "unweighted")
    check(Gv, d.vals, False, None, "value stream")
    check(Gv, d.vals, True, None, "scaled")
    check(Gu, None, True, None, "unweighted, scaled")
    check(Gv.dropped(desc), d.vals, True, d.kept, "dropped")
    check(Gu.dropped(desc), None, False, d.kept, "unweighted, dropped")
    # the epilogue and its backward: dX = diag(ss) A^T diag(ds) (dY * act'(Y) * mask * 2)
    mask = C.out_mask(d.n_dst, F, 3)
    for view, kept in ((Gv, None), (Gv.dropped(desc), d.kept)):
        pre = C.reference(d.dst, d.src, d.n_dst, X, d.vals, d.ss, d.ds, kept)
        y_ref = t(C.reference(d.dst, d.src, d.n_dst, X, d.vals, d.ss, d.ds, kept, mask, True))
        g_pre = (W * np.where(pre > 0, 1.0, C.SLOPE) * mask * C.MASK_SCALE).astype(np.float32)
        dx_ref = t(C.reference(d.src, d.dst, d.n_src, g_pre, d.vals, d.ds, d.ss, kept, x_gran=0.5))
        x = t(X if kept is None else X_bad).requires_grad_(True)
        y = ops.spmm_csr_act_dropout(view, x, ss, ds, 1, C.SLOPE, t(mask), C.MASK_SCALE)
        y.backward(t(W))
        assert torch.equal(y.detach(), y_ref) and torch.equal(x.grad, dx_ref), kept is None
        assert torch.equal(view.spmm(x.detach(), ss, ds, epi=(1, C.SLOPE, t(mask), C.MASK_SCALE)), y_ref)
