"""The canonical row sums of the XCD-local SpMM: within a (row, slice) segment ``acc`` starts at +0 and
takes the edges in layout order, ``acc + x`` or ``fmaf(w, x, acc)``; the planes are added in slice order.  A product is
then a function of the layout and the operands alone, which is checked on random-normal operands (every add rounds):
bitwise equality under every launch geometry, across the two element widths of the table, against a numpy restatement
of the order, and between dropout on the fly and the compacted layout.  The tapered tail (``sliced_taper_rows``) is
held to zero tolerance on the designed integer operands of _spmm_cases.py in all 12 + 6 template variants."""
import itertools

import numpy as np
import pytest
import torch

import _spmm_cases as C

pytestmark = pytest.mark.gpu
BF16 = torch.bfloat16
KNOBS = dict(C.DEFAULTS, sliced_taper_rows=0)
KINDS = ("unit", "vals", "mult")


@pytest.fixture(scope="module", autouse=True)
def _knobs_back_to_default():
    try:
        yield
    finally:
        _set(KNOBS)


def _set(knobs):
    from dream_gnn_amd import _lib

    for name, value in knobs.items():
        _lib.set_tuning(name, value)


def _t(a, dev):
    return None if a is None else torch.from_numpy(np.array(a)).to(dev)


def _bf16_valued(a):
    """float32 values with 8 significant bits (round to nearest even, like the library's conversion), none tiny: a
    product of two of them, and its sum with a float32, is exact in float64."""
    a = torch.from_numpy(np.asarray(a, np.float32)).to(BF16).float().numpy()
    return np.where(np.abs(a) < 2.0 ** -10, np.float32(2.0 ** -10), a).astype(np.float32)


_staged = {}


def _stage(dev):
    """The 307-row design of _spmm_cases.py on the device with random operands, once."""
    from dream_gnn_amd import ops

    if not _staged:
        d = C.sliced_design(8)
        sl = ops.SlicedCSR(_t(d.dst, dev), _t(d.src, dev), d.n_dst, d.n_src, n_slices=8)
        E = d.dst.size
        desc = ops.random_subset_select(E, int(E * C.DROP_KEEP), C.DROP_SEED, dev)
        assert np.array_equal(ops.keep_mask(desc, E).cpu().numpy().astype(bool), d.kept)
        order = sl.eid.cpu().numpy().astype(np.int64)
        rng = np.random.default_rng(2024)
        vals = _bf16_valued(rng.standard_normal(E))[order]        # sliced order
        ss = _bf16_valued(rng.uniform(0.5, 1.5, d.n_src))
        ds = rng.uniform(0.5, 1.5, d.n_dst).astype(np.float32)
        mult = d.mult[order]
        _staged.update(d=d, sl=sl, desc=desc, order=order, vals=vals, ss=ss, ds=ds, mult=mult, kept=d.kept[order],
                       segptr=sl.segptr.cpu().numpy().astype(np.int64), indices=sl.indices.cpu().numpy().astype(np.int64),
                       vals_d=_t(vals, dev), ss_d=_t(ss, dev), ds_d=_t(ds, dev),
                       ids=(sl.indices | ((_t(d.mult, dev) - 1)[sl.eid.long()] << ops.MULT_SHIFT)).contiguous())
    return _staged


def _table(n, F, seed, bf16_valued):
    X = np.random.default_rng(seed).standard_normal((n, F)).astype(np.float32)
    return _bf16_valued(X) if bf16_valued else X


def _product(st, X, kind, has_ss, dropped, table, layout=None, **extra):
    """``table``: "f32" (the fp32 kernel), "bf16" (X is a bf16 tensor) or "via" (fp32 X converted by the library, the
    source scale folded into the conversion)."""
    kw = dict(vals=st["vals_d"] if kind == "vals" else None, keep=st["desc"] if dropped else None)
    if kind == "mult":
        kw.update(indices=st["ids"], id_mult=True)
    if layout is not None:
        kw = {}
    return (layout or st["sl"]).spmm(X, st["ss_d"] if has_ss else None, st["ds_d"], gather_dtype=BF16 if table == "via" else None,
                                     **kw, **extra)


# ---------------------------------------------------------------------------------------------
# (1) geometry invariance
# ---------------------------------------------------------------------------------------------
def geometry_settings(n_dst):
    return [dict(sliced_lpr=a, sliced_rows=b, sliced_chunk_rows=c, sliced_taper_rows=t)
            for a in (0, 8, 16, 32, 64) for b in (1, 3, 7, 15) for c in (0, 1, 37) for t in (-1, 0, 5, 64, n_dst)]


@pytest.mark.parametrize("F", [128, 344])
@pytest.mark.parametrize("dropped", [False, True], ids=["all", "keep"])
@pytest.mark.parametrize("has_ss", [False, True], ids=["plain", "ss"])
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("table", ["f32", "bf16"])
def test_result_does_not_depend_on_the_launch_geometry(dev, table, kind, has_ss, dropped, F):
    """Random-normal operands: the product under every lane-group width x rows per group x row chunks x taper equals the
    default launch bitwise (a bf16 table takes its source scale through the conversion pass)."""
    st = _stage(dev)
    d = st["d"]
    X = _t(_table(d.n_src, F, F + 1, False), dev)
    if table == "bf16":
        table, X = ("via", X) if has_ss else ("bf16", X.to(BF16))
    try:
        _set(KNOBS)
        want = _product(st, X, kind, has_ss, dropped, table)
        assert float(want.abs().max()) > 1.0 and bool(torch.isfinite(want).all())
        for i, knobs in enumerate(geometry_settings(d.n_dst)):
            _set(knobs)
            y = _product(st, X, kind, has_ss, dropped, table, full_width=bool(i % 2))
            assert torch.equal(y, want), "%s: %d elements differ" % (knobs, int((y != want).sum()))
    finally:
        _set(KNOBS)


@pytest.mark.parametrize("F", [128, 344])
@pytest.mark.parametrize("kind", KINDS)
def test_element_width_of_the_table_does_not_matter(dev, kind, F):
    """The fp32 kernel on the upcast bf16 table equals the bf16 kernel, each at its own rows per lane group."""
    st = _stage(dev)
    Xb = _t(_table(st["d"].n_src, F, F + 2, False), dev).to(BF16)
    try:
        for rows_b, rows_f, chunk_b, taper_f in ((1, 15, 0, -1), (7, 3, 37, 64), (0, 5, 0, 0), (15, 1, 1, 307)):
            for dropped in (False, True):
                _set(dict(KNOBS, sliced_rows=rows_b, sliced_chunk_rows=chunk_b))
                a = _product(st, Xb, kind, False, dropped, "bf16")
                _set(dict(KNOBS, sliced_rows=rows_f, sliced_taper_rows=taper_f))
                b = _product(st, Xb.float(), kind, False, dropped, "f32")
                assert torch.equal(a, b), (rows_b, rows_f, dropped, int((a != b).sum()))
        assert float(a.abs().max()) > 1.0
    finally:
        _set(KNOBS)


# ---------------------------------------------------------------------------------------------
# (2) the order itself, restated in numpy
# ---------------------------------------------------------------------------------------------
def canonical(st, X, w=None, kept=None):
    """float32 ``Y`` before the epilogue: per (row, slice) segment ``acc = +0``, then edge by edge in layout order
    ``acc + x`` (``w is None``) or ``fmaf(w, x, acc)`` — evaluated exactly in float64 (see ``_bf16_valued``) and rounded
    once —, dropped edges skipped; the planes added in slice order; times ``dst_scale`` in float32."""
    d, segptr, indices = st["d"], st["segptr"], st["indices"]
    n_seg = 8 * d.n_dst
    start, length = segptr[:-1], np.diff(segptr)
    acc = np.zeros((n_seg, X.shape[1]), np.float32)
    for k in range(int(length.max())):
        seg = np.flatnonzero(length > k)
        p = start[seg] + k
        if kept is not None:
            seg, p = seg[kept[p]], p[kept[p]]
        x = X[indices[p]]
        if w is None:
            acc[seg] = acc[seg] + x
        else:
            acc[seg] = (w[p].astype(np.float64)[:, None] * x.astype(np.float64) + acc[seg].astype(np.float64)).astype(np.float32)
    planes = acc.reshape(8, d.n_dst, -1)
    y = planes[0].copy()
    for s in range(1, 8):
        y = y + planes[s]
    return y * st["ds"][:, None]


@pytest.mark.parametrize("F", [128, 344])
@pytest.mark.parametrize("table", ["f32", "bf16"])
def test_bitwise_against_the_order_restated_on_the_host(dev, table, F):
    """Unweighted on a random-normal table (float32 adds in layout order); weighted (value stream, multiplicities, with
    and without a source scale, with and without dropout on the fly) with bf16-valued weights and table entries."""
    st = _stage(dev)
    d = st["d"]
    assert st["segptr"][-1] == d.dst.size and np.diff(st["segptr"]).max() == max(C.DESIGNED_LENGTHS)
    up = lambda X: _t(X, dev).to(BF16) if table == "bf16" else _t(X, dev)
    X = _table(d.n_src, F, F + 3, table == "bf16")
    for dropped in (False, True):
        got = _product(st, up(X), "unit", False, dropped, table).cpu().numpy()
        want = canonical(st, X, None, st["kept"] if dropped else None)
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), ("unit", dropped, int((got != want).sum()))
    Xw = _table(d.n_src, F, F + 4, True)
    base = {"unit": np.ones(d.dst.size, np.float32), "vals": st["vals"], "mult": st["mult"].astype(np.float32)}
    for kind, has_ss, dropped in itertools.product(KINDS, (False, True), (False, True)):
        if kind == "unit" and not has_ss:
            continue  # the unweighted form: above
        kept = st["kept"] if dropped else None
        if table == "bf16" and has_ss:
            # a bf16 table takes the scale in its conversion pass: powers of two keep scale x entry bf16-valued
            ss2 = np.exp2(np.random.default_rng(7).integers(-1, 2, d.n_src)).astype(np.float32)
            kw = {"unit": {}, "vals": dict(vals=st["vals_d"]), "mult": dict(indices=st["ids"], id_mult=True)}[kind]
            y = st["sl"].spmm(_t(Xw, dev), _t(ss2, dev), st["ds_d"], gather_dtype=BF16, keep=st["desc"] if dropped else None, **kw)
            want = canonical(st, Xw * ss2[:, None], None if kind == "unit" else base[kind], kept)
        else:
            # vals x scale (8 x 8 bits) and scale x multiplicity (8 x 4 bits) are exact in float32
            w = base[kind] * st["ss"][st["indices"]] if has_ss else base[kind]
            y = _product(st, up(Xw), kind, has_ss, dropped, table)
            want = canonical(st, Xw, w, kept)
        got = y.cpu().numpy()
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), (kind, has_ss, dropped, int((got != want).sum()))
        assert np.abs(want).max() > 1.0


# ---------------------------------------------------------------------------------------------
# (3) dropout on the fly == the compacted layout
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("F", [128, 344])
@pytest.mark.parametrize("table", ["f32", "bf16"])
def test_dropout_on_the_fly_equals_the_compacted_layout(dev, table, F):
    """Random floats: a dropped edge adds an exact zero and moves nobody else's place in the order, so the KEEP kernels
    equal the plain kernels on the layout with the dropped edges removed — with Inf / NaN in the source rows that only
    dropped edges read."""
    st = _stage(dev)
    d, sl = st["d"], st["sl"]
    X = _table(d.n_src, F, F + 5, False)
    X[list(d.dead)[0::2]] = np.inf
    X[list(d.dead)[1::2]] = np.nan
    Xd = _t(X, dev).to(BF16) if table == "bf16" else _t(X, dev)
    for kind, has_ss in itertools.product(KINDS, (False, True)):
        if table == "bf16" and has_ss:
            continue  # the conversion pass, not the gather, takes the scale
        layout = sl.compacted(st["desc"], st["vals_d"] if kind == "vals" else None, indices=st["ids"] if kind == "mult" else None,
                              id_mult=kind == "mult")
        a = _product(st, Xd, kind, has_ss, True, table)
        b = _product(st, Xd, kind, has_ss, False, table, layout=layout)
        assert bool(torch.isfinite(a).all()) and torch.equal(a, b), (kind, has_ss, int((a != b).sum()))


@pytest.mark.parametrize("weighted", [False, True], ids=["unit", "vals"])
def test_dropped_view_is_the_same_compacted_or_on_the_fly(dev, monkeypatch, weighted):
    """``CSRGraph.dropped(desc).spmm`` / ``spmm_t`` with ``ops.COMPACT_DROPPED`` on and off: bitwise the same."""
    from dream_gnn_amd import ops
    from oracle import oracle as O

    monkeypatch.setattr(ops, "FORCE_KERNEL", "sliced")
    rng = np.random.default_rng(5 + weighted)
    n_dst, n_src, E, F = 700, 900, 30000, 128
    dst, src = rng.integers(0, n_dst, E).astype(np.int32), rng.integers(0, n_src, E).astype(np.int32)
    vals = rng.standard_normal(E).astype(np.float32) if weighted else None
    keep_n = int(E * 0.05)  # few survivors: many source rows are read by dropped edges only
    mask = O.random_subset_mask(E, keep_n, 77).astype(bool)
    dead = np.flatnonzero((np.bincount(src, minlength=n_src) > 0) & (np.bincount(src[mask], minlength=n_src) == 0))
    assert dead.size >= 20
    X = rng.standard_normal((n_src, F)).astype(np.float32)
    X[dead[0::2]] = np.inf
    X[dead[1::2]] = np.nan
    W = rng.standard_normal((n_dst, F)).astype(np.float32)
    ss, ds = rng.uniform(0.5, 1.5, n_src).astype(np.float32), rng.uniform(0.5, 1.5, n_dst).astype(np.float32)
    g = ops.CSRGraph(_t(dst, dev), _t(src, dev), n_dst, n_src, vals=_t(vals, dev))
    out = {}
    for compact in (True, False):
        monkeypatch.setattr(ops, "COMPACT_DROPPED", compact)
        view = g.dropped(ops.random_subset_select(E, keep_n, 77, dev))
        out[compact] = (view.spmm(_t(X, dev), _t(ss, dev), _t(ds, dev)), view.spmm_t(_t(W, dev), _t(ss, dev), _t(ds, dev)))
        assert ("sliced" in view._c) == compact
    for a, b in zip(out[True], out[False]):
        assert bool(torch.isfinite(a).all()) and float(a.abs().max()) > 1.0 and torch.equal(a, b), int((a != b).sum())


# ---------------------------------------------------------------------------------------------
# (4) the tapered tail covers every row once: zero tolerance on the integer designs
# ---------------------------------------------------------------------------------------------
VARIANTS = [(k, s, kp, "f32") for k, s, kp in itertools.product(KINDS, (False, True), (False, True))] + \
           [(k, False, kp, "bf16") for k, kp in itertools.product(KINDS, (False, True))]
# 307 rows: the taper starts inside the only chunk (100, 5), covers it (307), starts inside a later chunk (chunks of 150:
# the last 64 rows of the chunks at r0 = 0 and 150, and the whole 7-row chunk at r0 = 300), covers every chunk (37 <= 64)
TAPERS_307 = [dict(sliced_taper_rows=100), dict(sliced_taper_rows=5, sliced_rows=3), dict(sliced_taper_rows=307, sliced_rows=15),
              dict(sliced_taper_rows=64, sliced_chunk_rows=150), dict(sliced_taper_rows=64, sliced_chunk_rows=150, sliced_lpr=8),
              dict(sliced_taper_rows=64, sliced_chunk_rows=37, sliced_touch_lead=1),
              dict(sliced_taper_rows=100, sliced_lpr=64, sliced_rows=63), dict(sliced_taper_rows=33, sliced_lpr=16, sliced_rows=1),
              dict(sliced_taper_rows=-1), dict(sliced_taper_rows=0)]


@pytest.mark.parametrize("variant", VARIANTS, ids=["%s%s%s-%s" % (k, "-ss" if s else "", "-keep" if kp else "", t) for k, s, kp, t in VARIANTS])
def test_tapered_tail_every_row_exact(dev, variant):
    """The 307-row design, F = 128 and 344 (a ragged column tile): every row equals the integer reference under tapers
    that start inside a chunk, inside a later chunk, and cover a whole chunk.  A gap in the mapping leaves rows of the
    planes unwritten (whatever an earlier product left there), an overlap writes them from two groups."""
    kind, has_ss, dropped, table = variant
    st = _stage(dev)
    d, sl = st["d"], st["sl"]
    order = _t(st["order"], dev)
    vals_d, ss_d, ds_d = _t(d.vals, dev)[order].contiguous(), _t(d.ss, dev), _t(d.ds, dev)
    kw = dict(vals=vals_d if kind == "vals" else None, keep=st["desc"] if dropped else None)
    if kind == "mult":
        kw.update(indices=st["ids"], id_mult=True)
    w = {"unit": None, "vals": d.vals, "mult": d.mult}[kind]
    try:
        for F in (128, 344):
            X = C.features(d.n_src, F, 13 * F)
            want = _t(C.reference(d.dst, d.src, d.n_dst, X, w, d.ss if has_ss else None, d.ds, d.kept if dropped else None), dev)
            Xd = _t(C.features(d.n_src, F, 13 * F, dead=d.dead) if dropped else X, dev)
            Xd = Xd.to(BF16) if table == "bf16" else Xd
            for i, knobs in enumerate(TAPERS_307):
                _set(dict(KNOBS, **knobs))
                sl.spmm(torch.full_like(Xd, 3.0), None, None)  # planes a gap would show through
                y = sl.spmm(Xd, ss_d if has_ss else None, ds_d, full_width=bool(i % 2), **kw)
                assert torch.equal(y, want), "%s F=%d: rows %s differ" % (knobs, F, (y != want).any(1).nonzero().flatten().tolist()[:8])
    finally:
        _set(KNOBS)


@pytest.mark.parametrize("table", ["f32", "bf16"])
def test_tapered_tail_with_touchers_at_work(dev, table):
    """3 000 rows at F = 128 (47 worker blocks of 64 rows at the fp32 kernel's width untapered: the touchers 24 blocks
    ahead are at work), integer operands, value stream with dropout on the fly: exact under tapers inside the chunk, over
    the chunk, in later chunks and with a short lead, at several rows per group."""
    from dream_gnn_amd import ops

    rng = np.random.default_rng(3000)
    n_dst, n_src, F = 3000, 157, 128
    deg = rng.integers(0, 13, n_dst)
    deg[[5, 1500, 2990]] = (200, 0, 97)
    dst = np.repeat(np.arange(n_dst), deg).astype(np.int32)
    src = rng.integers(0, n_src, dst.size).astype(np.int32)
    E = dst.size
    vals = (rng.integers(1, 5, E) * rng.choice([-1, 1], E)).astype(np.float32)
    ds = rng.choice([0.25, 0.5, 1.0, 2.0], n_dst).astype(np.float32)
    kept = C.drop_mask(E)
    X = C.features(n_src, F, 9)
    sl = ops.SlicedCSR(_t(dst, dev), _t(src, dev), n_dst, n_src)
    desc = ops.random_subset_select(E, int(E * C.DROP_KEEP), C.DROP_SEED, dev)
    vals_d = _t(vals, dev)[sl.eid.long()].contiguous()
    Xd = _t(X, dev).to(BF16) if table == "bf16" else _t(X, dev)
    want = {False: _t(C.reference(dst, src, n_dst, X, vals, None, ds), dev),
            True: _t(C.reference(dst, src, n_dst, X, vals, None, ds, kept), dev)}
    settings = [dict(sliced_taper_rows=t, sliced_rows=r, sliced_chunk_rows=c, sliced_touch_lead=lead)
                for t in (-1, 0, 700, 3000) for r in (0, 3, 15) for c, lead in ((0, -1), (1100, 3))]
    try:
        for knobs in settings:
            _set(dict(KNOBS, **knobs))
            sl.spmm(torch.full_like(Xd, 3.0), None, None)
            for dropped in (False, True):
                y = sl.spmm(Xd, None, _t(ds, dev), vals=vals_d, keep=desc if dropped else None)
                assert torch.equal(y, want[dropped]), "%s: rows %s differ" % (knobs, (y != want[dropped]).any(1).nonzero().flatten().tolist()[:8])
    finally:
        _set(KNOBS)
