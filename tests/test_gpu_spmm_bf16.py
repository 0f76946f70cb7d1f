"""The XCD-local SpMM gathering from a bf16 table.  The designed integer operands of _spmm_cases.py are exact
in bf16 and their sums exact in fp32, so the kernel is held to ``torch.equal`` in every launch shape and form; the
conversion pass is held to the bits of ``Tensor.to(torch.bfloat16)``; random tables pin the summation ORDER against the
fp32 kernel (bitwise) and the accuracy contract against float64 (derived bounds); then the graph, ops, module and
stream-capture levels, each against the explicit ``rows_to_bf16`` + ``SlicedCSR.spmm`` composition, bitwise."""
import os

import numpy as np
import pytest
import torch

import _spmm_cases as C

pytestmark = pytest.mark.gpu
BF16 = torch.bfloat16
COMBOS = [(False, False), (True, False), (False, True), (True, True)]  # dst_scale, epilogue
WIDTHS = (8, 16, 32)


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


def _stage(dev, n_slices):
    """The design on the device, once: layout, values and id words in sliced order, the subset description."""
    from dream_gnn_amd import ops

    if n_slices not in _staged:
        d = C.sliced_design(n_slices)
        sl = ops.SlicedCSR(_t(d.dst, dev), _t(d.src, dev), d.n_dst, d.n_src, n_slices=n_slices)
        assert int(sl.range_flag) == 0
        E = d.dst.size
        desc = ops.random_subset_select(E, int(E * C.DROP_KEEP), C.DROP_SEED, dev)
        assert np.array_equal(ops.keep_mask(desc, E).cpu().numpy().astype(bool), d.kept)
        order = sl.eid.long()
        _staged[n_slices] = dict(
            d=d, sl=sl, desc=desc, vals=_t(d.vals, dev)[order].contiguous(), ss=_t(d.ss, dev), ds=_t(d.ds, dev),
            ids=(sl.indices | ((_t(d.mult, dev) - 1)[order] << ops.MULT_SHIFT)).contiguous())
    return _staged[n_slices]


def pick_lpr_bf16(F):
    """``pick_lpr(F, 8, 32)`` (csrc/dgmi_kernels.h): ``pick_lpr`` of the fp32 kernel on F / 8 lanes, widths 32 / 16 / 8."""
    f8 = (F + 7) // 8
    best, best_util = 8, 0.0
    for lpr in (32, 16, 8):
        util = f8 / (-(-f8 // lpr) * lpr)
        if util >= 0.85:
            return lpr
        if util > best_util + 1e-9:
            best, best_util = lpr, util
    return best


def geometry_bf16(n_rows, F, knobs):
    """``C.sliced_geometry`` at the lane-group width the bf16 launcher takes (64 is not one of its widths: ignored),
    with the column tiles of 8 * LPR columns."""
    lpr = knobs["sliced_lpr"] if knobs["sliced_lpr"] in WIDTHS else pick_lpr_bf16(F)
    g = C.sliced_geometry(n_rows, F, lpr, knobs["sliced_rows"], knobs["sliced_chunk_rows"], knobs["sliced_touch_lead"])
    return g._replace(col_tiles=-(-F // (8 * lpr)), ragged_tile=F % (8 * lpr) != 0)


def _sweep(dev, n_slices, F, kind, dropped, settings, route="bf16", compacted=False):
    """One form at one width under every knob setting, with and without ``dst_scale`` and the epilogue: ``torch.equal``
    against the integer reference.  ``route == "f32"``: the fp32 table with a source scale, converted by the library."""
    from dream_gnn_amd import _lib

    st = _stage(dev, n_slices)
    d, sl = st["d"], st["sl"]
    seed = 11 * F + n_slices
    X = C.features(d.n_src, F, seed)
    mask = C.out_mask(d.n_dst, F, seed + 1)
    w = {"unit": None, "vals": d.vals, "mult": d.mult}[kind]
    has_ss = route == "f32"
    # x_gran = 1: with a source scale `reference` lowers the granularity to min |ss| = 1/2 itself, and ss * X (|.| <= 16 in
    # halves) is exact in bf16's 8 significant bits
    want = {(has_ds, epi): _t(C.reference(d.dst, d.src, d.n_dst, X, w, d.ss if has_ss else None, d.ds if has_ds else None,
                                          d.kept if dropped else None, mask if epi else None, epi, x_gran=1.0), dev)
            for has_ds, epi in COMBOS}
    empty = torch.tensor(C.EMPTY_ROWS, device=dev)
    assert all(bool((y[empty] == 0).all()) for y in want.values())
    Xd = _t(C.features(d.n_src, F, seed, dead=d.dead) if dropped else X, dev)  # Inf / NaN behind the dropped edges
    if route == "bf16":
        assert torch.equal(Xd.to(BF16).float().nan_to_num(7.0, 7.0, 7.0), Xd.nan_to_num(7.0, 7.0, 7.0))  # exact in bf16
        Xd = Xd.to(BF16)
    mask_d = _t(mask, dev)
    layout = sl
    kw = dict(vals=st["vals"] if kind == "vals" else None, keep=st["desc"] if dropped else None)
    if kind == "mult":
        kw.update(indices=st["ids"], id_mult=True)
    if compacted:
        assert dropped
        layout = sl.compacted(st["desc"], st["vals"] if kind == "vals" else None, indices=st["ids"] if kind == "mult" else None,
                              id_mult=kind == "mult")
        kw = {}
    seen = []
    for i, knobs in enumerate(settings):
        for name, value in knobs.items():
            _lib.set_tuning(name, value)
        seen.append(geometry_bf16(d.n_dst, F, knobs))
        for has_ds, epi in COMBOS:
            y = layout.spmm(Xd, st["ss"] if has_ss else None, st["ds"] if has_ds else None,
                            epi=(1, C.SLOPE, mask_d, C.MASK_SCALE) if epi else None, full_width=bool(i % 2),
                            gather_dtype=BF16 if has_ss else None, **kw)
            assert y.dtype == torch.float32
            assert torch.equal(y, want[has_ds, epi]), "%s dst_scale=%s epilogue=%s: %d elements differ, first row %d" % (
                knobs, has_ds, epi, int((y != want[has_ds, epi]).sum()), int((y != want[has_ds, epi]).any(1).nonzero()[0]))
    for name, value in C.DEFAULTS.items():
        _lib.set_tuning(name, value)
    return seen


# ---------------------------------------------------------------------------------------------
# (1) the conversion pass, bitwise
# ---------------------------------------------------------------------------------------------
def _conversion_matrix():
    rng = np.random.default_rng(5)
    n, F = 257, 136
    bits = rng.standard_normal((n, F)).astype(np.float32).view(np.uint32)
    flat = bits.reshape(-1)
    pos = iter(rng.permutation(flat.size))
    special = []
    for b in (0x3f80, 0x3f81, 0x4049, 0x404a, 0xbf80, 0xbf83, 0x0001, 0x0002, 0x7f7e, 0x7f7f, 0xff7f, 0x0080, 0x007f):
        hi = np.uint32(b) << np.uint32(16)
        special += [hi | 0x8000, hi | 0x7fff, hi | 0x8001, hi | 0x0001, hi | 0xffff, hi]  # the tie (both parities of b), around it
    special += [0x00000000, 0x80000000, 0x7f800000, 0xff800000,                  # +-0, +-Inf
                0x00000001, 0x80000001, 0x00008000, 0x00018000, 0x007fffff, 0x807fffff, 0x00400000,  # fp32 denormals
                0x7f7fffff, 0xff7fffff,                                           # +-FLT_MAX: rounds to Inf
                0x7fc00000, 0xffc00000, 0x7f800001, 0x7fffffff, 0xff812345]       # NaN, quiet and signalling
    special += list(np.array([3.3895e38, -3.3895e38, 3.3962e38, -3.3962e38], np.float32).view(np.uint32))
    for k in range(40):  # several copies, so that every value meets every scale
        for b in special:
            flat[next(pos)] = b
    return bits.view(np.float32)


@pytest.mark.parametrize("scaled", [False, True], ids=["plain", "scaled"])
def test_rows_to_bf16_is_bitwise_torch(dev, scaled):
    """257 x 136 viewed with a leading dimension of 144: normals, exact ties of both parities and their neighbours, +-0,
    +-Inf, fp32 denormals, values beyond the largest bf16, NaN — the bits of ``(scale[:, None] * X).to(bfloat16)`` computed
    on the CPU (scales are powers of two), NaN where it is NaN."""
    from dream_gnn_amd import ops

    X = torch.from_numpy(_conversion_matrix())
    n, F = X.shape
    scale = torch.from_numpy(np.random.default_rng(6).choice([0.25, 0.5, 1.0, 2.0], n).astype(np.float32)) if scaled else None
    want = (X if scale is None else scale[:, None] * X).to(BF16)
    buf = torch.full((n, 144), float("nan"), device=dev)
    buf[:, :F] = X.to(dev)
    view = buf[:, :F]
    assert view.stride(0) == 144 and not view.is_contiguous()
    got = ops.rows_to_bf16(view, None if scale is None else scale.to(dev))
    assert got.dtype == BF16 and got.shape == (n, F) and got.is_contiguous()
    got, nan = got.cpu(), want.isnan()
    assert int(nan.sum()) >= 5 * 40 and torch.equal(got.isnan(), nan)
    gb, wb = got.view(torch.int16), want.view(torch.int16)
    assert torch.equal(gb[~nan], wb[~nan]), "%d of %d bit patterns differ" % (int((gb != wb)[~nan].sum()), int((~nan).sum()))
    assert bool(want[~nan].isinf().any()) and bool((want.float()[~nan].abs() < 1.2e-38).any())
    # a contiguous matrix and one thread's worth of columns take the same path
    small = ops.rows_to_bf16(X[:3, :8].contiguous().to(dev), None if scale is None else scale[:3].to(dev)).cpu()
    ok = ~want[:3, :8].isnan()
    assert torch.equal(small.view(torch.int16)[ok], want[:3, :8].contiguous().view(torch.int16)[ok])


# ---------------------------------------------------------------------------------------------
# (2) every launch shape, zero tolerance
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("F", [8, 128, 344])
@pytest.mark.parametrize("form", [("unit", False), ("vals", True)], ids=["unit", "vals-keep"])
def test_every_launch_shape_each_knob_alone_and_in_pairs(dev, form, F):
    """8 slices, 307 rows: the default launch, each ``sliced_*`` knob alone, (lpr, rows), (chunk_rows, touch_lead) and a
    toucher in a later chunk — and the shapes those settings reach, restated on the host."""
    seen = _sweep(dev, 8, F, form[0], form[1], C.one_at_a_time(C.N_DST))
    assert {g.lpr for g in seen} == set(WIDTHS)
    assert {(g.lpr, g.R) for g in seen} >= {(8, 1), (8, 3), (8, 7), (16, 15), (32, 15), (32, 31), (16, 8), (32, 8)}
    assert any(g.chunks > 1 and g.chunk_rows[-1] < g.chunk_rows[0] for g in seen)  # a shorter last chunk
    assert any(sum(g.active_touchers) > 0 for g in seen) and any(sum(g.active_touchers) == 0 for g in seen)
    assert any(g.chunks > 1 and any(a > 0 for a in g.active_touchers[1:]) for g in seen)  # a toucher at work in a chunk with r0 > 0
    assert any(sum(g.tail_groups) > 0 for g in seen)
    if F == 344:
        assert pick_lpr_bf16(F) == 16 and seen[0].col_tiles == 3 and seen[0].ragged_tile
        assert {g.col_tiles for g in seen} == {6, 3, 2}
    if F == 128:
        assert pick_lpr_bf16(F) == 16 and seen[0].col_tiles == 1 and {g.col_tiles for g in seen} == {2, 1}
    if F == 8:
        assert pick_lpr_bf16(F) == 8 and {g.col_tiles for g in seen} == {1}


@pytest.mark.parametrize("lpr", WIDTHS)
def test_full_knob_cross(dev, lpr):
    """rows x chunk_rows x no_off32 x touch_lead in full at every lane-group width, F = 128, the value stream with
    dropout on the fly (the toucher's ``vals[p]`` / ``eid[p]`` loads)."""
    _sweep(dev, 8, 128, "vals", True, C.full_cross(C.N_DST, lpr))


@pytest.mark.parametrize("n_slices", [3, 1, 64])
def test_other_slice_counts(dev, n_slices):
    """3 slices, 1 slice, and 64 slices over 40 sources (empty trailing slices): the generic plane reduce."""
    for F in (8, 128, 344):
        _sweep(dev, n_slices, F, "unit", False, C.one_at_a_time(C.N_DST))
    _sweep(dev, n_slices, 128, "mult", True, C.one_at_a_time(C.N_DST))


# ---------------------------------------------------------------------------------------------
# (3) every form of the kernel, zero tolerance
# ---------------------------------------------------------------------------------------------
FEW = [dict(C.DEFAULTS), dict(C.DEFAULTS, sliced_rows=3, sliced_chunk_rows=37, sliced_touch_lead=1),
       dict(C.DEFAULTS, sliced_lpr=32, sliced_rows=31)] + C.no_off32_at_every_width()  # (64: not a bf16 width, the built-in one)


@pytest.mark.parametrize("F", [8, 128, 344])
@pytest.mark.parametrize("kind", ["unit", "vals", "mult"])
def test_every_form(dev, kind, F):
    """VALS 0 / 1 / 2, each plain, with dropout on the fly (Inf / NaN in the dead rows of the bf16 table) and on the
    compacted layout, with ``dst_scale`` and the epilogue; and the fp32 input route, ``gather_dtype=bfloat16`` with a
    source scale in {0.5, 1, 2} folded into the conversion.  ``FEW`` takes every width with 32-bit and with 64-bit row
    addresses: all 36 instantiations of the bf16 gather are launched here."""
    _sweep(dev, 8, F, kind, False, FEW)
    _sweep(dev, 8, F, kind, True, FEW)
    _sweep(dev, 8, F, kind, True, FEW, compacted=True)
    _sweep(dev, 8, F, kind, False, FEW, route="f32")
    _sweep(dev, 8, F, kind, True, FEW, route="f32")
    _sweep(dev, 8, F, kind, True, FEW, route="f32", compacted=True)


def test_layout_level_refusals(dev):
    from dream_gnn_amd import ops

    st = _stage(dev, 8)
    d, sl = st["d"], st["sl"]
    with pytest.raises(RuntimeError, match="pass the float32 table"):
        sl.spmm(torch.zeros(d.n_src, 8, device=dev, dtype=BF16), st["ss"])
    for X in (torch.zeros(d.n_src, 12, device=dev, dtype=BF16), torch.zeros(d.n_src, 12, device=dev)):
        with pytest.raises(RuntimeError, match="multiple of 8"):
            sl.spmm(X, gather_dtype=BF16)
    with pytest.raises(RuntimeError, match="multiple of 8"):
        ops.rows_to_bf16(torch.zeros(5, 12, device=dev))
    # a view whose rows are not 16-B aligned is copied by the op, never read misaligned
    wide = _t(C.features(d.n_src, 24, 3), dev).to(BF16)
    want = _t(C.reference(d.dst, d.src, d.n_dst, C.features(d.n_src, 24, 3)[:, 4:20]), dev)
    assert torch.equal(sl.spmm(wide[:, 4:20]), want)
    fw = _t(C.features(d.n_src, 24, 3), dev)
    assert torch.equal(sl.spmm(fw[:, 4:20], gather_dtype=BF16), want)
    out = torch.empty(d.n_dst, 16, device=dev)
    assert sl.spmm(wide[:, 4:20], out=out) is out and torch.equal(out, want)


# ---------------------------------------------------------------------------------------------
# (4) bit-identity with the fp32 kernel: the summation ORDER
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("F", [128, 344])
@pytest.mark.parametrize("kind", ["unit", "vals", "mult"])
def test_bit_identical_to_the_fp32_kernel_on_the_upcast_table(dev, kind, F):
    """Random normal bf16 tables (every sum rounds): ``spmm(Xb) == spmm(Xb.float())`` bitwise at the same rows per lane
    group and row chunks — the two kernels use different lane-group widths for the same F, nothing else differs."""
    from dream_gnn_amd import _lib

    st = _stage(dev, 8)
    d, sl = st["d"], st["sl"]
    g = torch.Generator(device="cpu").manual_seed(F)
    Xb = torch.randn(d.n_src, F, generator=g).to(dev).to(BF16)
    vals = torch.randn(st["vals"].shape[0], generator=g).to(dev)
    kw = {"unit": {}, "vals": dict(vals=vals), "mult": dict(indices=st["ids"], id_mult=True)}[kind]
    try:
        for rows, chunk in ((0, 0), (1, 0), (3, 37), (7, 0), (15, 306)):
            _lib.set_tuning("sliced_rows", rows)
            _lib.set_tuning("sliced_chunk_rows", chunk)
            for keep in (None, st["desc"]):
                a = sl.spmm(Xb, None, st["ds"], keep=keep, **kw)
                b = sl.spmm(Xb.float(), None, st["ds"], keep=keep, **kw)
                assert torch.equal(a, b), (rows, chunk, keep is not None, int((a != b).sum()))
                assert torch.equal(a, sl.spmm(Xb, None, st["ds"], keep=keep, **kw))  # reproducible
        assert float(a.abs().max()) > 1.0
    finally:
        for name, value in C.DEFAULTS.items():
            _lib.set_tuning(name, value)


def column_pass_lpr(F, n_src, n_slices, n_dst, elem_bytes):
    """``sliced_lpr`` (csrc/dgmi_sliced_common.h) for a plain product (no ``full_width``, no dropout on the fly, no forced
    width): half the width when the slice one XCD gathers from exceeds its 4 MiB L2."""
    lpr = C.pick_lpr(F) if elem_bytes == 4 else pick_lpr_bf16(F)
    if lpr >= 32 and n_dst >= 32768 and -(-n_src // n_slices) * min(16 * lpr, elem_bytes * F) > 4 << 20:
        lpr //= 2
    return lpr


def test_column_passes_on_bf16_bytes(dev):
    """Bit-identity ACROSS the column-pass threshold on bf16 bytes.  32 768 rows (the rule's floor), F = 256, 8 slices:
    at 65 537 sources a bf16 slice is 8 193 rows x 512 B, one row over 4 MiB, where the rule asks for two half-width
    passes; at 65 536 it does not (the fp32 product halves at both).  Random normal bf16 tables, so every sum rounds: the
    product equals, bitwise, its own single full-width pass and the fp32 kernel's full-width pass over the upcast table —
    also with 16-lane groups forced.  Half and full width are bit-identical by design, so this does NOT observe which
    width the library launched: the threshold itself is asserted on the host restatement ``column_pass_lpr`` only."""
    from dream_gnn_amd import _lib, ops

    n_dst, F, n_slices = 32768, 256, 8
    assert [column_pass_lpr(F, n, n_slices, n_dst, 2) for n in (65537, 65536)] == [16, 32]
    assert [column_pass_lpr(F, n, n_slices, n_dst, 4) for n in (65537, 65536)] == [32, 32] and C.pick_lpr(F) == 64
    assert column_pass_lpr(F, 65537, n_slices, n_dst - 1, 2) == 32
    rng = np.random.default_rng(256)
    try:
        for n_src in (65537, 65536):
            dst = np.repeat(np.arange(n_dst), rng.integers(0, 9, n_dst)).astype(np.int32)  # about 4 edges per row
            src = rng.integers(0, n_src, dst.size).astype(np.int32)
            sl = ops.SlicedCSR(_t(dst, dev), _t(src, dev), n_dst, n_src, n_slices=n_slices)
            g = torch.Generator(device="cpu").manual_seed(n_src)
            Xb = torch.randn(n_src, F, generator=g).to(dev).to(BF16)
            for lpr in (0, 16):
                _lib.set_tuning("sliced_lpr", lpr)
                y = sl.spmm(Xb)
                assert torch.equal(y, sl.spmm(Xb, full_width=True)), (n_src, lpr)
                assert torch.equal(y, sl.spmm(Xb.float(), full_width=True)), (n_src, lpr)
            assert float(y.abs().max()) > 1.0
    finally:
        for name, value in C.DEFAULTS.items():
            _lib.set_tuning(name, value)


# ---------------------------------------------------------------------------------------------
# (5) the accuracy contract on random values
# ---------------------------------------------------------------------------------------------
def _f64_rows(dst, terms, n_dst):
    order = np.argsort(dst, kind="stable")
    rows, terms = dst[order], terms[order]
    starts = np.flatnonzero(np.diff(rows, prepend=-1))
    y = np.zeros((n_dst, terms.shape[1]))
    y[rows[starts]] = np.add.reduceat(terms, starts, axis=0)
    return y


@pytest.mark.parametrize("graph", ["knn2500", "bipartite4096x2048"])
def test_accuracy_contract(dev, graph):
    """(a) against float64 on the ROUNDED table: elementwise <= 1e-5 * sum |w x~| — the project's parity bar, the
    accumulation being the fp32 kernel's.  (b) against float64 on the UNROUNDED table: <= (2**-8 + 1e-5) * sum |w ss x|,
    2**-8 being the unit roundoff of bf16's 8 significant bits (every |ss x| is a normal number).  Worst observed
    fractions of the two bounds (MI355X): knn2500 0.020 / 0.63, bipartite 0.007 / 0.70."""
    from dream_gnn_amd import ops

    rng = np.random.default_rng(17)
    F = 128
    if graph == "knn2500":
        n_dst = n_src = 2500
        dst = np.repeat(np.arange(n_dst), 16)
        src = rng.integers(0, n_src, dst.size)
        w = rng.uniform(0.05, 1.0, dst.size).astype(np.float32)
    else:
        n_dst, n_src = 4096, 2048
        dst = np.repeat(np.arange(n_dst), rng.integers(8, 41, n_dst))
        src = rng.integers(0, n_src, dst.size)
        w = None
    X = rng.standard_normal((n_src, F)).astype(np.float32)
    ss = rng.uniform(0.5, 1.5, n_src).astype(np.float32)
    ds = rng.uniform(0.5, 1.5, n_dst).astype(np.float32)
    sl = ops.SlicedCSR(_t(dst.astype(np.int32), dev), _t(src.astype(np.int32), dev), n_dst, n_src, vals=_t(w, dev))
    y = sl.spmm(_t(X, dev), _t(ss, dev), _t(ds, dev), gather_dtype=BF16).cpu().numpy().astype(np.float64)
    xb = ops.rows_to_bf16(_t(X, dev), _t(ss, dev))
    assert torch.equal(sl.spmm(xb, None, _t(ds, dev)).cpu(), torch.from_numpy(y.astype(np.float32)))
    xr = xb.float().cpu().numpy().astype(np.float64)
    we = np.ones(dst.size) if w is None else w.astype(np.float64)
    d64 = ds.astype(np.float64)[:, None]
    t_r = we[:, None] * xr[src]
    t_u = we[:, None] * (ss.astype(np.float64)[:, None] * X.astype(np.float64))[src]
    assert np.abs(ss[:, None] * X).min() > 1.2e-38
    err_a = np.abs(y - d64 * _f64_rows(dst, t_r, n_dst))
    bound_a = 1e-5 * d64 * _f64_rows(dst, np.abs(t_r), n_dst)
    err_b = np.abs(y - d64 * _f64_rows(dst, t_u, n_dst))
    bound_b = (2.0 ** -8 + 1e-5) * d64 * _f64_rows(dst, np.abs(t_u), n_dst)
    print("%s: worst fraction of bound (a) %.4f, (b) %.4f" % (graph, (err_a / bound_a).max(), (err_b / bound_b).max()))
    assert np.all(err_a <= bound_a) and np.all(err_b <= bound_b)


# ---------------------------------------------------------------------------------------------
# (6) graph level
# ---------------------------------------------------------------------------------------------
_graphs = {}


def _graph(dev, name):
    """``wide``: 2 048 destination rows x 64 edges over 12 288 sources — at F = 128 the smallest table (6.3 MB) that takes
    the XCD-local form by the existing rule; its transpose (a 1 MB table) does not.  ``square``: 12 288 x 12 288, 48 edges
    per row — both directions take it."""
    from dream_gnn_amd import ops

    if name not in _graphs:
        rng = np.random.default_rng(len(name))
        n_dst, n_src, deg = {"wide": (2048, 12288, 64), "square": (12288, 12288, 48)}[name]
        dst = np.repeat(np.arange(n_dst), deg).astype(np.int32)
        src = rng.integers(0, n_src, dst.size).astype(np.int32)
        F = 128
        g = dict(n_dst=n_dst, n_src=n_src, dst=_t(dst, dev), src=_t(src, dev), F=F,
                 X=_t(rng.standard_normal((n_src, F)).astype(np.float32), dev),
                 dY=_t(rng.standard_normal((n_dst, F)).astype(np.float32), dev),
                 ss=_t(rng.uniform(0.5, 1.5, n_src).astype(np.float32), dev),
                 ds=_t(rng.uniform(0.5, 1.5, n_dst).astype(np.float32), dev),
                 vals=_t(rng.uniform(0.1, 1.0, dst.size).astype(np.float32), dev))
        g["G"] = ops.CSRGraph(g["dst"], g["src"], n_dst, n_src)
        g["sl"] = ops.SlicedCSR(g["dst"], g["src"], n_dst, n_src)
        g["sl_t"] = ops.SlicedCSR(g["src"], g["dst"], n_src, n_dst)
        _graphs[name] = g
    return _graphs[name]


def _explicit(g, X, ss, ds, layout="sl", **kw):
    """The product written out: one conversion pass with the gathered side's scale, then the bf16 gather."""
    from dream_gnn_amd import ops

    return g[layout].spmm(ops.rows_to_bf16(X, ss), None, ds, **kw)


@pytest.mark.skipif(bool(os.environ.get("DGMI_FORCE_KERNEL")), reason="kernel choice is forced")
@pytest.mark.parametrize("name", ["wide", "square"])
def test_graph_and_ops_level(dev, name):
    from dream_gnn_amd import ops

    g = _graph(dev, name)
    G, X, dY, ss, ds, F = g["G"], g["X"], g["dY"], g["ss"], g["ds"], g["F"]
    both = name == "square"
    assert G.takes_bf16_gather(F) and G.takes_bf16_gather(F, transposed=True) == both
    assert not G.takes_bf16_gather(12) and not G.takes_bf16_gather(132) and G.takes_bf16_gather(136)
    y_ref = _explicit(g, X, ss, ds)
    y_f32 = G.spmm(X, ss, ds)
    assert not torch.equal(y_ref, y_f32) and torch.allclose(y_ref, y_f32, rtol=0, atol=0.02 * float(y_f32.abs().max()))
    assert torch.equal(G.spmm(X, ss, ds, gather_dtype=BF16), y_ref)
    assert torch.equal(G.spmm(X, ss, ds, gather_dtype=torch.float32), y_f32)
    assert torch.equal(G.spmm(ops.rows_to_bf16(X, ss), None, ds), y_ref)            # a bf16 table handed in
    out = torch.empty_like(y_ref)
    assert G.spmm(X, ss, ds, out=out, gather_dtype=BF16) is out and torch.equal(out, y_ref)
    with pytest.raises(RuntimeError, match="pass the float32 table"):
        G.spmm(X.to(BF16), ss, ds)
    # the transposed product: dX = diag(ss) A^T diag(ds) dY, ds folded into the conversion of dY, ss applied by the reduce
    dx_f32 = G.spmm_t(dY, ss, ds)
    dx_ref = _explicit(g, dY, ds, ss, "sl_t") if both else dx_f32
    assert torch.equal(G.spmm_t(dY, ss, ds, gather_dtype=BF16), dx_ref) and (not both or not torch.equal(dx_ref, dx_f32))
    if not both:
        with pytest.raises(RuntimeError, match="does not take the plain XCD-local form"):
            G.spmm_t(dY.to(BF16))
    # ops.spmm_csr: forward and backward, by keyword and under gather_precision (the backward outside the block)
    for how in ("keyword", "context"):
        x = X.clone().requires_grad_(True)
        if how == "keyword":
            y = ops.spmm_csr(G, x, ss, ds, gather_dtype=BF16)
        else:
            with ops.gather_precision(BF16):
                y = ops.spmm_csr(G, x, ss, ds)
                assert torch.equal(G.spmm(X, ss, ds), y_ref) and torch.equal(G.spmm(X, ss, ds, gather_dtype=torch.float32), y_f32)
        y.backward(dY)
        assert torch.equal(y.detach(), y_ref) and torch.equal(x.grad, dx_ref), how
    x = X.clone().requires_grad_(True)
    y = ops.spmm_csr(G, x, ss, ds)
    with ops.gather_precision(BF16):  # a float32 product keeps float32 in a backward that runs inside a block
        y.backward(dY)
    assert torch.equal(y.detach(), y_f32) and torch.equal(x.grad, dx_f32)
    # the fused epilogue and its backward
    mask = (torch.rand(g["n_dst"], F, device=dev) < 0.7).float()
    x = X.clone().requires_grad_(True)
    with ops.gather_precision(BF16):
        y = ops.spmm_csr_act_dropout(G, x, ss, ds, 1, 0.1, mask, 1.25)
    y.backward(dY)
    y_epi = _explicit(g, X, ss, ds, epi=(1, 0.1, mask, 1.25))
    g_pre = ops.epilogue_backward(dY, y_epi, mask, 1, 0.1, 1.25)
    assert torch.equal(y.detach(), y_epi)
    assert torch.equal(x.grad, _explicit(g, g_pre, ds, ss, "sl_t") if both else G.spmm_t(g_pre, ss, ds))
    # a value view (random values: no scale x multiplicity form, the value stream)
    Gv = G.with_values(g["vals"])
    assert torch.equal(Gv.spmm(X, ss, ds, gather_dtype=BF16), _explicit(g, X, ss, ds, vals=g["vals"][g["sl"].eid.long()].contiguous()))
    # dropped views: compacted (the default) and on the fly
    E = int(g["dst"].shape[0])
    desc = ops.random_subset_select(E, int(0.8 * E), 9, dev)
    view = G.dropped(desc)
    want = g["sl"].compacted(desc).spmm(ops.rows_to_bf16(X, ss), None, ds)
    assert torch.equal(view.spmm(X, ss, ds, gather_dtype=BF16), want) and "sliced" in view._c
    if both:
        assert torch.equal(view.spmm_t(dY, ss, ds, gather_dtype=BF16),
                           g["sl_t"].compacted(desc).spmm(ops.rows_to_bf16(dY, ds), None, ss))


@pytest.mark.skipif(bool(os.environ.get("DGMI_FORCE_KERNEL")), reason="kernel choice is forced")
def test_requests_that_fall_back(dev):
    """A 300-row graph and an F = 12 product do not take the XCD-local form: a float32 ``X`` gets today's float32 result,
    bit for bit, a bfloat16 ``X`` is refused with the reason."""
    from dream_gnn_amd import ops

    d = C.split_graph("heavy")
    G = ops.CSRGraph(_t(d.dst, dev), _t(d.src, dev), d.n_dst, d.n_src)
    X = torch.randn(d.n_src, 128, device=dev)
    assert not G.takes_bf16_gather(128) and not G.takes_bf16_gather(128, transposed=True)
    y = G.spmm(X, _t(d.ss, dev), _t(d.ds, dev))
    assert torch.equal(G.spmm(X, _t(d.ss, dev), _t(d.ds, dev), gather_dtype=BF16), y)
    with ops.gather_precision(BF16):
        assert torch.equal(G.spmm(X, _t(d.ss, dev), _t(d.ds, dev)), y)
        x = X.clone().requires_grad_(True)
        ops.spmm_csr(G, x, _t(d.ss, dev), _t(d.ds, dev)).backward(torch.ones(d.n_dst, 128, device=dev))
    assert torch.equal(x.grad, G.spmm_t(torch.ones(d.n_dst, 128, device=dev), _t(d.ss, dev), _t(d.ds, dev)))
    with pytest.raises(RuntimeError, match="does not take the plain XCD-local form"):
        G.spmm(X.to(BF16))
    g = _graph(dev, "wide")
    X12 = torch.randn(g["n_src"], 12, device=dev)
    y12 = g["G"].spmm(X12, g["ss"], g["ds"])
    assert torch.equal(g["G"].spmm(X12, g["ss"], g["ds"], gather_dtype=BF16), y12)
    with pytest.raises(RuntimeError, match="not a multiple of 8"):
        g["G"].spmm(X12.to(BF16))


# ---------------------------------------------------------------------------------------------
# (7) module level
# ---------------------------------------------------------------------------------------------
@pytest.mark.skipif(bool(os.environ.get("DGMI_FORCE_KERNEL")), reason="kernel choice is forced")
def test_modules_under_gather_precision(dev):
    """``GraphConvolution`` and ``GCMCGraphConv`` on the square graph: under ``gather_precision(bfloat16)`` output and
    input gradient equal the same computation written out with the ops-level calls; outside it they are what they are
    without the feature (the float32 product), bit for bit."""
    import dream_gnn_amd
    from dream_gnn_amd import graph as GR, layers, ops

    g = _graph(dev, "square")
    G, dY, F = g["G"], g["dY"], g["F"]
    torch.manual_seed(3)
    inp = torch.randn(g["n_src"], 64, device=dev)

    def run(fn, ctx):
        x = inp.clone().requires_grad_(True)
        if ctx:
            with dream_gnn_amd.gather_precision(BF16):
                y = fn(x)
        else:
            y = fn(x)
        y.backward(dY)
        return y.detach(), x.grad

    gc = layers.GraphConvolution(64, F).to(dev)
    written = lambda dt: (lambda x: ops.spmm_csr(G, torch.mm(x, gc.weight), gather_dtype=dt) + gc.bias)
    rel = GR.RelationGraph(("drug", "1", "disease"), g["src"], g["dst"], g["n_src"], g["n_dst"],
                           {"cj": g["ss"].view(-1, 1)}, {"ci": g["ds"].view(-1, 1)})
    conv = layers.GCMCGraphConv(64, F, dropout_rate=0.0).to(dev)
    written_c = lambda dt: (lambda x: ops.spmm_csr(rel.csr, layers.dot_or_identity(x, conv.weight, None),
                                                   src_scale=g["ss"].view(-1, 1), dst_scale=g["ds"].view(-1, 1), gather_dtype=dt))
    for module, wr in ((lambda x: gc(x, G), written), (lambda x: conv(rel, x), written_c)):
        y_b, gx_b = run(module, True)
        y_w, gx_w = run(wr(BF16), False)
        assert torch.equal(y_b, y_w) and torch.equal(gx_b, gx_w)
        y_0, gx_0 = run(module, False)
        y_p, gx_p = run(wr(torch.float32), False)
        assert torch.equal(y_0, y_p) and torch.equal(gx_0, gx_p)
        assert not torch.equal(y_b, y_0) and not torch.equal(gx_b, gx_0)
    # ... and the float32 product is the parent's: the layout's fp32 kernel, no conversion pass
    s = torch.mm(inp, gc.weight)
    assert torch.equal(gc(inp, G), g["sl"].spmm(s) + gc.bias)


# ---------------------------------------------------------------------------------------------
# (8) recordable
# ---------------------------------------------------------------------------------------------
@pytest.mark.skipif(bool(os.environ.get("DGMI_FORCE_KERNEL")), reason="kernel choice is forced")
def test_forward_and_backward_record_into_a_hip_graph(dev):
    """Forward and backward under the context, captured on one stream after an eager warm-up on a side stream (as
    ``CapturedTrainStep`` does) and replayed twice on new inputs: bitwise the eager results.  Nothing on the path
    synchronises or allocates outside the caching allocator."""
    from dream_gnn_amd import ops

    g = _graph(dev, "square")
    G, ss, ds = g["G"], g["ss"], g["ds"]
    x = g["X"].clone().requires_grad_(True)
    dy = g["dY"].clone()

    def step():
        x.grad = None
        with ops.gather_precision(BF16):
            y = ops.spmm_csr(G, x, ss, ds)
        y.backward(dy)
        return y.detach(), x.grad

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(2):
            step()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        y_c, gx_c = step()
    for seed in (1, 2):
        gen = torch.Generator(device="cpu").manual_seed(seed)
        with torch.no_grad():
            x.copy_(torch.randn(x.shape, generator=gen))
            dy.copy_(torch.randn(dy.shape, generator=gen))
        graph.replay()
        torch.cuda.synchronize()
        got_y, got_gx = y_c.clone(), gx_c.clone()
        want_y = _explicit(g, x.detach(), ss, ds)
        want_gx = _explicit(g, dy, ds, ss, "sl_t")
        assert torch.equal(got_y, want_y) and torch.equal(got_gx, want_gx), seed
