"""The XCD-local SpMM on the designed integer operands of _spmm_cases.py, ZERO tolerance: every launch shape the
``sliced_*`` tuning knobs reach on a 307-row graph (row chunks, rows per lane group, lane-group width against F, 64-bit
row addresses, toucher blocks) in all 12 template variants, and ``ops._SplitSliced`` on 300-row graphs, every row.  The only
tolerance in the file is the project's elementwise 1e-5 rule, for one ``randn`` case through the split form."""
import itertools
import os

import numpy as np
import pytest
import torch

import _spmm_cases as C

pytestmark = pytest.mark.gpu

VARIANTS = list(itertools.product(("unit", "vals", "mult"), (False, True), (False, True)))  # values, src_scale, dropped
COMBOS = list(itertools.product((False, True), (False, True)))                              # dst_scale, epilogue


@pytest.fixture(scope="module", autouse=True)
def _knobs_back_to_default():
    from dream_gnn_amd import _lib

    try:
        yield
    finally:
        for name, value in C.DEFAULTS.items():
            _lib.set_tuning(name, value)


def _t(a, dev):
    return None if a is None else torch.from_numpy(np.array(a)).to(dev)  # a copy: the designs are read-only


_staged = {}


def _stage(oracle, dev, n_slices):
    """The design on the device, once: layout (checked against the oracle's), values and id words in sliced order, the
    subset description (checked against the host mask)."""
    from dream_gnn_amd import ops

    if n_slices not in _staged:
        assert ops.MULT_SHIFT == C.MULT_SHIFT
        d = C.sliced_design(n_slices)
        sl = ops.SlicedCSR(_t(d.dst, dev), _t(d.src, dev), d.n_dst, d.n_src, n_slices=n_slices)
        segptr, indices, eid = oracle.csr_sliced_from_coo(d.dst, d.src, d.n_dst, d.n_src, n_slices)
        assert np.array_equal(sl.segptr.cpu().numpy(), segptr) and np.array_equal(sl.indices.cpu().numpy(), indices)
        assert np.array_equal(sl.eid.cpu().numpy(), eid) and int(sl.range_flag) == 0
        E = d.dst.size
        desc = ops.random_subset_select(E, int(E * C.DROP_KEEP), C.DROP_SEED, dev)
        assert np.array_equal(ops.keep_mask(desc, E).cpu().numpy().astype(bool), d.kept)
        order = sl.eid.long()
        _staged[n_slices] = dict(
            d=d, sl=sl, desc=desc, vals=_t(d.vals, dev)[order].contiguous(), ss=_t(d.ss, dev), ds=_t(d.ds, dev),
            ids=(sl.indices | ((_t(d.mult, dev) - 1)[order] << ops.MULT_SHIFT)).contiguous())
    return _staged[n_slices]


def _sweep(oracle, dev, n_slices, F, variant, settings):
    """One variant at one width under every knob setting of ``settings``, with and without ``dst_scale`` and the
    epilogue: ``torch.equal`` against the integer reference."""
    from dream_gnn_amd import _lib

    st = _stage(oracle, dev, n_slices)
    d, sl = st["d"], st["sl"]
    kind, has_ss, dropped = variant
    seed = 7 * F + n_slices
    X = C.features(d.n_src, F, seed)
    mask = C.out_mask(d.n_dst, F, seed + 1)
    w = {"unit": None, "vals": d.vals, "mult": d.mult}[kind]
    want = {(has_ds, epi): _t(C.reference(d.dst, d.src, d.n_dst, X, w, d.ss if has_ss else None, d.ds if has_ds else None,
                                          d.kept if dropped else None, mask if epi else None, epi), dev)
            for has_ds, epi in COMBOS}
    empty = torch.tensor(C.EMPTY_ROWS, device=dev)
    assert all(bool((y[empty] == 0).all()) for y in want.values())
    # Inf / NaN in the source rows that only dropped edges read
    Xd = _t(C.features(d.n_src, F, seed, dead=d.dead) if dropped else X, dev)
    mask_d = _t(mask, dev)
    kw = dict(vals=st["vals"] if kind == "vals" else None, keep=st["desc"] if dropped else None)
    if kind == "mult":
        kw.update(indices=st["ids"], id_mult=True)
    for i, knobs in enumerate(settings):
        for name, value in knobs.items():
            _lib.set_tuning(name, value)
        for has_ds, epi in COMBOS:
            y = sl.spmm(Xd, st["ss"] if has_ss else None, st["ds"] if has_ds else None,
                        epi=(1, C.SLOPE, mask_d, C.MASK_SCALE) if epi else None, full_width=bool(i % 2), **kw)
            assert torch.equal(y, want[has_ds, epi]), "%s dst_scale=%s epilogue=%s: %d elements differ, first row %d" % (
                knobs, has_ds, epi, int((y != want[has_ds, epi]).sum()),
                int((y != want[has_ds, epi]).any(1).nonzero()[0]))
    for name, value in C.DEFAULTS.items():
        _lib.set_tuning(name, value)


@pytest.mark.parametrize("F", [4, 128, 344])
@pytest.mark.parametrize("variant", VARIANTS, ids=["%s%s%s" % (k, "-ss" if s else "", "-keep" if kp else "") for k, s, kp in VARIANTS])
def test_sliced_every_variant_each_knob_alone_and_in_pairs(oracle, dev, variant, F):
    """All 12 template variants (unit / value stream / multiplicity x src_scale x dropout on the fly) at F = 4 / 128 /
    344: the default launch, each knob alone, (lpr, rows), (chunk_rows, touch_lead) and a toucher in a later chunk; then
    64-bit row addresses at every width — with them every one of the 96 instantiations of the fp32 gather is launched."""
    _sweep(oracle, dev, 8, F, variant, C.one_at_a_time(C.N_DST) + C.no_off32_at_every_width())


@pytest.mark.parametrize("lpr", [0, 8, 16, 32, 64])
@pytest.mark.parametrize("variant", [("unit", False, False), ("vals", True, True)], ids=["unit", "vals-ss-keep"])
def test_sliced_full_knob_cross(oracle, dev, variant, lpr):
    """The full cross rows x chunk_rows x no_off32 x touch_lead (192 settings per lane-group width) at F = 128: unit
    values, and the value stream with ``src_scale`` and dropout on the fly (the toucher's ``vals[p]`` / ``eid[p]`` loads)."""
    _sweep(oracle, dev, 8, 128, variant, C.full_cross(C.N_DST, lpr))


@pytest.mark.parametrize("n_slices", [3, 1, 64])
@pytest.mark.parametrize("variant", [("unit", False, False), ("vals", True, True), ("mult", True, True)], ids=["unit", "vals-ss-keep", "mult-ss-keep"])
def test_sliced_other_slice_counts(oracle, dev, variant, n_slices):
    """3 slices, 1 slice, and 64 slices over 40 sources (``n_src < n_slices``, empty trailing slices): the generic plane
    reduce, under the same one-at-a-time sweep."""
    for F in (4, 128):
        _sweep(oracle, dev, n_slices, F, variant, C.one_at_a_time(C.N_DST))


# ---------------------------------------------------------------------------------------------
# the split form
# ---------------------------------------------------------------------------------------------
def _split_setup(monkeypatch, dev, kind, layout):
    from dream_gnn_amd import ops

    monkeypatch.setattr(ops, "SPLIT_MIN_TABLE_BYTES", 0)
    if layout == "16/4":
        monkeypatch.setattr(ops, "SPLIT_ROW_EDGES", 16)
        monkeypatch.setattr(ops, "SPLIT_LIGHT_ROW_EDGES", 4)
    g = C.split_graph(kind)
    E = g.dst.size
    assert not ops.CSRGraph._is_regular(int(g.deg.max()), E, g.n_dst) and g.deg.max() == 3000
    assert not ops.CSRGraph._is_regular(int(g.deg_t.max()), E, g.n_src)
    return ops, g, E


def _check_split(ops, G, g):
    """Both directions took the split form, with the virtual rows the host restatement expects."""
    S = G._S
    assert S.regular is False and S.regular_t is False and S.sliced is None and S.sliced_t is None
    for split, deg in ((S.split, g.deg), (S.split_t, g.deg_t)):
        want = C.split_geometry(deg, ops.SPLIT_ROW_EDGES, ops.SPLIT_LIGHT_ROW_EDGES)
        assert split is not None and (split.has_light, split.n_virtual) == (want.has_light, want.n_virtual)
        # second-stage entries per row: a heavy row's virtual rows, a light row's own edges
        assert np.array_equal(np.diff(split.c_indptr.cpu().numpy()), np.where(want.per_row == 0, deg, want.per_row))


@pytest.mark.skipif(bool(os.environ.get("DGMI_FORCE_KERNEL")), reason="kernel choice is forced")
@pytest.mark.parametrize("layout", ["256/24", "16/4"])
@pytest.mark.parametrize("kind", ["light", "heavy"])
def test_split_form_every_row_exact(oracle, dev, monkeypatch, kind, layout):
    """``CSRGraph.spmm`` / ``spmm_t`` / autograd through ``_SplitSliced`` (heavy rows cut into virtual rows, light rows
    through the second stage) on the designed 300-row graphs: unweighted, value stream, scaled, with the epilogue,
    edge-dropped after compaction and on the fly, dropped twice, under an inverted description — ``torch.equal`` against
    the integer reference and against the planned kernel, with Inf / NaN behind the dropped edges of both stages."""
    ops, g, E = _split_setup(monkeypatch, dev, kind, layout)
    F = 128
    t = lambda a: _t(a, dev)
    X, W = C.features(g.n_src, F, 1), C.features(g.n_dst, F, 2)
    X_bad, W_bad = C.features(g.n_src, F, 1, dead=g.dead_src), C.features(g.n_dst, F, 2, dead=g.dead_dst)
    ss, ds = t(g.ss), t(g.ds)
    desc = ops.random_subset_select(E, int(E * C.DROP_KEEP), C.DROP_SEED, dev)
    desc2 = ops.random_subset_select(E, E // 2, 5, dev)
    inverted = desc.clone()
    inverted[6] = 1  # kKeepInvert (graph.fused_relations_complement builds these): the edges the description drops take part
    assert np.array_equal(oracle.keep_mask(inverted.cpu().numpy(), E).astype(bool), ~g.kept)
    Gu = ops.CSRGraph(t(g.dst), t(g.src), g.n_dst, g.n_src)
    Gv = ops.CSRGraph(t(g.dst), t(g.src), g.n_dst, g.n_src, vals=t(g.vals))

    def check(view, w, scaled, kept, bad, what):
        s_np, d_np = (g.ss, g.ds) if scaled else (None, None)
        s_t, d_t = (ss, ds) if scaled else (None, None)
        Xd, Wd = t(X_bad if bad else X), t(W_bad if bad else W)
        y_ref = t(C.reference(g.dst, g.src, g.n_dst, X, w, s_np, d_np, kept))
        dx_ref = t(C.reference(g.src, g.dst, g.n_src, W, w, d_np, s_np, kept))
        keep = view._keep
        assert torch.equal(view.spmm(Xd, s_t, d_t), y_ref), what
        assert torch.equal(view.spmm_t(Wd, s_t, d_t), dx_ref), what
        _check_split(ops, view, g)
        assert torch.equal(ops.spmm_csr_raw(view.indptr, view.indices, view.vals, Xd, s_t, d_t, plan=view.plan, eid=view.eid,
                                            keep=keep), y_ref), what
        it, ix, vt, plan_t = view.transposed()
        assert torch.equal(ops.spmm_csr_raw(it, ix, vt, Wd, d_t, s_t, plan=plan_t, eid=view._t_struct()[2], keep=keep), dx_ref), what
        x = Xd.clone().requires_grad_(True)
        y = ops.spmm_csr(view, x, s_t, d_t)
        y.backward(Wd)
        assert torch.equal(y.detach(), y_ref) and torch.equal(x.grad, dx_ref), what

    check(Gu, None, False, None, False, "unweighted")
    assert Gu._S.split.has_light == (kind == "light")  # the background degree decides it, under both layouts
    check(Gv, g.vals, False, None, False, "value stream")
    check(Gv, g.vals, True, None, False, "scaled")
    check(Gu, None, True, None, False, "unweighted, scaled")
    for compact in (True, False):
        monkeypatch.setattr(ops, "COMPACT_DROPPED", compact)
        for G0, w in ((Gv, g.vals), (Gu, None)):
            view = G0.dropped(desc)
            check(view, w, True, g.kept, True, "dropped, compact=%s" % compact)
            assert ("split" in view._c and "split_t" in view._c) == compact
            check(view.dropped(desc2), w, True, g.kept & g.kept2, True, "dropped twice, compact=%s" % compact)
            check(G0.dropped(inverted), w, False, ~g.kept, False, "inverted description, compact=%s" % compact)
    # the epilogue (second stage) and its backward: dX = diag(ss) A^T diag(ds) (dY * act'(Y) * mask * 2)
    mask = C.out_mask(g.n_dst, F, 3)
    for compact, dropped in ((True, False), (True, True), (False, True)):
        monkeypatch.setattr(ops, "COMPACT_DROPPED", compact)
        view, kept = (Gv.dropped(desc), g.kept) if dropped else (Gv, None)
        pre = C.reference(g.dst, g.src, g.n_dst, X, g.vals, g.ss, g.ds, kept)
        y_ref = t(C.reference(g.dst, g.src, g.n_dst, X, g.vals, g.ss, g.ds, kept, mask, True))
        g_pre = (W * np.where(pre > 0, 1.0, C.SLOPE) * mask * C.MASK_SCALE).astype(np.float32)
        dx_ref = t(C.reference(g.src, g.dst, g.n_src, g_pre, g.vals, g.ds, g.ss, kept, x_gran=0.5))
        x = t(X_bad if dropped else X).requires_grad_(True)
        y = ops.spmm_csr_act_dropout(view, x, ss, ds, 1, C.SLOPE, t(mask), C.MASK_SCALE)
        y.backward(t(W))
        assert torch.equal(y.detach(), y_ref) and torch.equal(x.grad, dx_ref), (compact, dropped)
        assert torch.equal(view.spmm(x.detach(), ss, ds, epi=(1, C.SLOPE, t(mask), C.MASK_SCALE)), y_ref)
    assert np.all(C.reference(g.dst, g.src, g.n_dst, X, g.vals, g.ss, g.ds, g.kept)[list(C.SPLIT_EMPTY) + list(g.dead_dst)] == 0)


@pytest.mark.skipif(bool(os.environ.get("DGMI_FORCE_KERNEL")), reason="kernel choice is forced")
@pytest.mark.parametrize("layout", ["256/24", "16/4"])
def test_split_form_randn_every_row_elementwise(oracle, dev, monkeypatch, layout):
    """``randn`` operands through the split form, both directions, dropped and not: the project's elementwise rule
    against the f64 oracle, ``|y - y64| <= 1e-5 * sum |terms|`` for every element and ``<= 1e-5 * max |y64|``."""
    ops, g, E = _split_setup(monkeypatch, dev, "light", layout)
    rng = np.random.default_rng(11)
    F = 64
    t = lambda a: _t(a, dev)
    X, W = rng.standard_normal((g.n_src, F)).astype(np.float32), rng.standard_normal((g.n_dst, F)).astype(np.float32)
    vals = rng.standard_normal(E).astype(np.float32)
    ss, ds = rng.uniform(0.5, 1.5, g.n_src).astype(np.float32), rng.uniform(0.5, 1.5, g.n_dst).astype(np.float32)
    G = ops.CSRGraph(t(g.dst), t(g.src), g.n_dst, g.n_src, vals=t(vals))
    desc = ops.random_subset_select(E, int(E * C.DROP_KEEP), C.DROP_SEED, dev)
    for view, kept in ((G, np.ones(E, bool)), (G.dropped(desc), g.kept)):
        for rows, cols, n_rows, Z, a, b, got in ((g.dst, g.src, g.n_dst, X, ss, ds, view.spmm(t(X), t(ss), t(ds))),
                                                 (g.src, g.dst, g.n_src, W, ds, ss, view.spmm_t(t(W), t(ss), t(ds)))):
            ip, ix, e0 = oracle.csr_from_coo(rows[kept], cols[kept], n_rows)
            y64 = oracle.spmm_csr(ip, ix, vals[kept][e0], Z, a, b, acc="f64")
            yabs = oracle.spmm_csr(ip, ix, vals[kept][e0], Z, a, b, acc="abs")
            err = np.abs(got.cpu().numpy().astype(np.float64) - y64)
            assert np.all(err <= 1e-5 * yabs + 1e-30) and err.max() <= 1e-5 * np.abs(y64).max()
        _check_split(ops, view, g)


# ---------------------------------------------------------------------------------------------
# the record sort's other tile order
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(300_000, 1000, 70_001), (513, 90, 16_385)])
def test_sort_plain_tiles_builds_the_same_layouts(dev, shape):
    """``sort_plain_tiles = 1`` (tile = blockIdx.x instead of the XCD-aware order): the CSR and both sliced layouts are
    bit-identical to the default order's, at two shapes of ``test_record_sort_builds_every_layout_bit_exact``."""
    from dream_gnn_amd import _lib, ops

    n_dst, n_src, E = shape
    rng = np.random.default_rng(E)
    d, s = _t(rng.integers(0, n_dst, E).astype(np.int32), dev), _t(rng.integers(0, n_src, E).astype(np.int32), dev)

    def build():
        indptr, indices, eid, flag = ops.csr_from_coo(d, s, n_dst, n_src, return_flag=True)
        a = ops.SlicedCSR(d, s, n_dst, n_src)
        b = ops.SlicedCSR.from_csr(indptr, indices, eid, n_dst, n_src)
        return [indptr, indices, eid, flag, a.segptr, a.indices, a.eid, b.segptr, b.indices, b.eid]

    default = build()
    _lib.set_tuning("sort_plain_tiles", 1)
    try:
        plain = build()
    finally:
        _lib.set_tuning("sort_plain_tiles", 0)
    assert int(default[3]) == 0 and all(torch.equal(x, y) for x, y in zip(default, plain))
    assert torch.equal(default[4], default[7]) and torch.equal(default[5], default[8]) and torch.equal(default[6], default[9])
