"""The workgroup-owned form of the XCD-local SpMM gathering from a bf16 table (csrc/dgmi_owned.hip: rows summed in
LDS, 8 columns per lane, no partial planes), forced with ``sliced_owned = 1`` through ``dgmi_spmm_sliced_bf16``, so that
``Y`` may be strided.  On the designed integer operands of _spmm_cases.py (exact in bf16, sums exact in fp32) it is held
to ZERO tolerance (``torch.equal``) under every knob that shapes its plan; on ``randn`` tables rounded by
``dgmi_rows_to_bf16`` to the bits of the bf16 pair (``sliced_owned = 0``) and of the fp32 owned kernel on the upcast
table; on layouts of 3, 16 and 64 slices to both; what the form does not take must come back as the pair's product; and
the graph level (``CSRGraph.spmm`` / ``spmm_t``, ``ops.spmm_csr`` with autograd, a captured product) gives the same bits
with the knob at 0 and at 1.

The shapes are the smallest at which each index can go wrong: 307 rows (prime) over 8 slices; F = 344 has a column
round > 0 at every width and a partly filled last column tile, F = 8 leaves every lane group but lane 0 past F; grid 19
leaves workgroups without rows and a short last one; LDS caps give 2 and 4 row rounds with a short last round;
``sliced_no_off32`` takes the 64-bit row addresses."""
import itertools

import numpy as np
import pytest
import torch

import _owned_window_cases as D
import _spmm_cases as C

pytestmark = pytest.mark.gpu
BF16 = torch.bfloat16
WIDTHS = (8, 16, 32)

KNOBS = dict(sliced_owned=-1, sliced_owned_slices=0, sliced_owned_grid=0, sliced_owned_rows=0, sliced_owned_lds_rows=0,
             sliced_owned_lag=-2, sliced_owned_spin_ticks=0, sliced_owned_wgs=0, sliced_owned_workers=0, sliced_lpr=0,
             sliced_no_off32=0, sliced_chunk_rows=0)


@pytest.fixture(autouse=True)
def _knobs_back_to_default():
    from dream_gnn_amd import _lib

    try:
        yield
    finally:
        for name, value in KNOBS.items():
            _lib.set_tuning(name, value)


def _set(**knobs):
    from dream_gnn_amd import _lib

    for name, value in dict(KNOBS, **knobs).items():
        _lib.set_tuning(name, value)


def _t(a, dev):
    return None if a is None else torch.from_numpy(np.array(a)).to(dev)


_staged = {}


def _design(n_slices):
    if n_slices == 16:  # _spmm_cases has no 16-slice design: the one of the fp32 slice-count tests
        import test_gpu_spmm_owned_slices as S

        return S.design16()
    return C.sliced_design(n_slices)


def _stage(dev, n_slices=8):
    from dream_gnn_amd import ops

    if n_slices not in _staged:
        d = _design(n_slices)
        sl = ops.SlicedCSR(_t(d.dst, dev), _t(d.src, dev), d.n_dst, d.n_src, n_slices=n_slices)
        assert int(sl.range_flag) == 0 and sl.n_slices == n_slices
        ids = (sl.indices | ((_t(d.mult, dev) - 1)[sl.eid.long()] << ops.MULT_SHIFT)).contiguous()
        _staged[n_slices] = dict(d=d, sl=sl, ds=_t(d.ds, dev), ids=ids)
    return _staged[n_slices]


def _call(name, sl, ids, id_mult, X, ds, epi_mask, ld_y):
    from dream_gnn_amd import _lib

    n_dst, F = sl.n_dst, X.shape[1]
    ld = F if ld_y is None else ld_y
    buf = torch.full((n_dst, ld), float("nan"), device=X.device)
    nbytes = _lib.lib.dgmi_spmm_sliced_planes_bytes(n_dst, sl.n_slices, F)
    planes = torch.empty(max(nbytes // 4, 4), dtype=torch.float32, device=X.device)
    epi = (1, C.SLOPE, epi_mask.data_ptr(), epi_mask.stride(0), C.MASK_SCALE) if epi_mask is not None else (0, 0.0, None, 0, 1.0)
    table = (X.data_ptr(), X.stride(0)) + ((None,) if name == "dgmi_spmm_sliced_f32" else ())  # fp32: a null src_scale
    _lib.check(getattr(_lib.lib, name)(
        sl.segptr.data_ptr(), ids.data_ptr(), None, None, None, 0, *table, None if ds is None else ds.data_ptr(),
        buf.data_ptr(), ld, n_dst, sl.n_src, F, sl.n_slices, 0, int(id_mult), planes.data_ptr(), nbytes, *epi,
        torch.cuda.current_stream().cuda_stream), name)
    if ld > F:
        assert bool(torch.isnan(buf[:, F:]).all()), "the product wrote outside its F columns"
    return buf[:, :F]


def _product(sl, ids, id_mult, Xb, ds=None, epi_mask=None, ld_y=None):
    """``dgmi_spmm_sliced_bf16`` on the layout ``sl`` with the id words ``ids`` and the bf16 table ``Xb``; ``ld_y``:
    leading dimension of ``Y`` (a view of a wider NaN-filled buffer, whose other columns must stay NaN)."""
    assert Xb.dtype == BF16
    return _call("dgmi_spmm_sliced_bf16", sl, ids, id_mult, Xb, ds, epi_mask, ld_y)


def _product_f32(sl, ids, id_mult, X, ds=None, epi_mask=None):
    assert X.dtype == torch.float32
    return _call("dgmi_spmm_sliced_f32", sl, ids, id_mult, X, ds, epi_mask, None)


def _cap(n_dst, grid, rounds):
    """The LDS-row cap that gives ``rounds`` row rounds of a workgroup's B = ceil(n_dst / grid) rows."""
    B = -(-n_dst // grid)
    return 0 if rounds == 1 else -(-B // rounds)


def _settings(n_dst):
    """Each knob alone, then lane-group width x R x row rounds on 3 workgroups."""
    out = [dict()]
    out += [dict(sliced_lpr=w) for w in WIDTHS]
    out += [dict(sliced_owned_grid=g) for g in (1, 3, 8, 19)]
    out += [dict(sliced_owned_rows=r) for r in (1, 2, 5)]
    out += [dict(sliced_owned_grid=8, sliced_owned_lds_rows=_cap(n_dst, 8, k)) for k in (2, 4)]
    out += [dict(sliced_no_off32=1), dict(sliced_no_off32=1, sliced_owned_grid=3, sliced_owned_rows=2)]
    out += [dict(sliced_owned_workers=1), dict(sliced_owned_workers=1, sliced_owned_grid=19, sliced_owned_rows=2)]
    out += [dict(sliced_lpr=w, sliced_owned_rows=r, sliced_owned_grid=3, sliced_owned_lds_rows=_cap(n_dst, 3, k))
            for w, r, k in itertools.product(WIDTHS, (1, 2, 5), (1, 2, 4))]
    return out


def _kernels_of(run):
    with torch.profiler.profile(activities=[torch.profiler.ProfilerActivity.CUDA]) as prof:
        run()
        torch.cuda.synchronize()
    return " ".join(e.key for e in prof.key_averages())


# ---------------------------------------------------------------------------------------------
# (1) the knob selects the kernel
# ---------------------------------------------------------------------------------------------
def test_forced_form_launches_the_owned_bf16_kernel(dev):
    """A profiled call on a bf16 table: ``sliced_owned = 1`` shows ``spmm_owned_bf16_kernel`` and no plane reduce,
    ``sliced_owned = 0`` the bf16 pair — and the built-in rule (-1) runs the pair on this small product."""
    st = _stage(dev)
    Xb = _t(C.features(st["d"].n_src, 128, 5), dev).to(BF16)
    names = {}
    for flag in (1, 0, -1):
        _set(sliced_owned=flag)
        names[flag] = _kernels_of(lambda: _product(st["sl"], st["sl"].indices, False, Xb))
    assert "spmm_owned_bf16_kernel" in names[1] and "reduce_planes_kernel" not in names[1], names[1]
    assert "spmm_sliced_bf16_kernel" not in names[1], names[1]
    for flag in (0, -1):
        assert "spmm_sliced_bf16_kernel" in names[flag] and "reduce_planes_kernel" in names[flag], names[flag]
        assert "spmm_owned_bf16_kernel" not in names[flag], names[flag]


def test_built_in_rule_takes_a_measured_bf16_class_and_nothing_else(dev):
    """``sliced_owned = -1`` on a product of a measured class (profiles/owned_bf16/README.md: 8 slices, one column round,
    one row round, unit values, a 24.4 MiB bf16 table: 100 000 sources -> 50 000 rows at F = 128) runs the owned kernel;
    the same graph at F = 64 (a 12.2 MiB table: no class of unit values in one row round) runs the pair.  Either way
    the bits are the pair's.  Three edges per row keep the launches short."""
    from dream_gnn_amd import ops

    n_dst, n_src = 50000, 100000
    rng = np.random.default_rng(50)
    dst = np.repeat(np.arange(n_dst, dtype=np.int32), 3)
    src = rng.integers(0, n_src, dst.size).astype(np.int32)
    sl = ops.SlicedCSR(_t(dst, dev), _t(src, dev), n_dst, n_src, n_slices=8)
    gen = torch.Generator(device="cpu").manual_seed(50)
    X = torch.randn(n_src, 128, generator=gen).to(dev).to(BF16)
    for F, owned in ((128, True), (64, False)):
        Xb = X[:, :F].contiguous()
        _set(sliced_owned=0)
        pair = _product(sl, sl.indices, False, Xb)
        _set(sliced_owned=-1)
        names = _kernels_of(lambda: _product(sl, sl.indices, False, Xb))
        assert ("spmm_owned_bf16_kernel" in names) == owned and ("reduce_planes_kernel" in names) != owned, (F, names)
        assert torch.equal(_product(sl, sl.indices, False, Xb), pair), F


# ---------------------------------------------------------------------------------------------
# (2) zero tolerance on the designed operands, every knob
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("F", [8, 128, 344])
@pytest.mark.parametrize("kind", ["unit", "mult"])
def test_owned_bf16_exact_on_designed_operands(dev, kind, F):
    """Every lane-group width, grids 1 / 3 / 8 / 19, R 1 / 2 / 5, 1 / 2 / 4 row rounds, 64-bit row addresses, one wave
    running every task; unit values and id multiplicities; ``dst_scale`` on and off, the activation + mask epilogue on
    and off, a strided ``Y`` whose padding stays NaN."""
    st = _stage(dev)
    d, sl = st["d"], st["sl"]
    seed = 13 * F + 5
    X = C.features(d.n_src, F, seed)
    mask = C.out_mask(d.n_dst, F, seed + 1)
    w = d.mult if kind == "mult" else None
    ids = st["ids"] if kind == "mult" else sl.indices
    combos = list(itertools.product((False, True), (False, True)))
    want = {(has_ds, epi): _t(C.reference(d.dst, d.src, d.n_dst, X, w, None, d.ds if has_ds else None, None,
                                          mask if epi else None, epi), dev) for has_ds, epi in combos}
    Xd, mask_d = _t(X, dev), _t(mask, dev)
    Xb = Xd.to(BF16)
    assert torch.equal(Xb.float(), Xd)  # the designed features are exact in bf16
    for i, knobs in enumerate(_settings(d.n_dst)):
        _set(sliced_owned=1, **knobs)
        for has_ds, epi in combos:
            y = _product(sl, ids, kind == "mult", Xb, st["ds"] if has_ds else None, mask_d if epi else None,
                         ld_y=F + 8 if i % 2 else None)
            assert torch.equal(y, want[has_ds, epi]), "%s dst_scale=%s epilogue=%s: %d elements differ, first row %d" % (
                knobs, has_ds, epi, int((y != want[has_ds, epi]).sum()), int((y != want[has_ds, epi]).any(1).nonzero()[0]))


def _stage_window(dev):
    from dream_gnn_amd import ops

    if "window" not in _staged:
        d = D.design()
        sl = ops.SlicedCSR(_t(d.dst, dev), _t(d.src, dev), d.n_dst, d.n_src, n_slices=D.N_SLICES)
        assert np.array_equal(sl.segptr.cpu().numpy(), d.segptr) and np.array_equal(sl.indices.cpu().numpy(), d.indices)
        ids = (sl.indices | ((_t(d.mult, dev) - 1)[sl.eid.long()] << ops.MULT_SHIFT)).contiguous()
        _staged["window"] = dict(d=d, sl=sl, ids=ids)
    return _staged["window"]


@pytest.mark.parametrize("F", [8, 128, 344])
@pytest.mark.parametrize("kind", ["unit", "mult"])
def test_owned_bf16_window_exact_on_the_designed_graph(dev, kind, F):
    """The graph designed for the rolling window (_owned_window_cases.py: every segment length around the window and
    the lane-group widths as first, middle and last row of a run, empty tasks, a last id of ``n_src - 1``), which
    test_gpu_spmm_owned_window.py runs through the fp32 kernel: the group, last-group and drain paths are those of the
    one kernel body, here under the bf16 row policy.  Its settings at the widths a bf16 table has."""
    st = _stage_window(dev)
    d, sl = st["d"], st["sl"]
    X = np.random.default_rng(7 * F + 1).integers(-8, 9, (d.n_src, F)).astype(np.float32)
    want = _t(D.reference(d, X, d.mult if kind == "mult" else None), dev)
    ids = st["ids"] if kind == "mult" else sl.indices
    Xb = _t(X, dev).to(BF16)
    assert torch.equal(Xb.float(), _t(X, dev))  # integers in [-8, 8] are exact in bf16
    settings = [knobs for knobs in D.settings() if knobs["sliced_lpr"] in WIDTHS]
    assert len(settings) == len(D.settings()) * 3 // 4
    for i, knobs in enumerate(settings):
        _set(sliced_owned=1, **knobs)
        y = _product(sl, ids, kind == "mult", Xb, ld_y=F + 8 if i % 2 == 0 else None)  # (_product checks the NaN frame)
        assert torch.equal(y, want), "%s: %d elements differ, first row %d" % (
            knobs, int((y != want).sum()), int((y != want).any(1).nonzero()[0]))


# ---------------------------------------------------------------------------------------------
# (3) bit for bit against the bf16 pair and the fp32 owned kernel
# ---------------------------------------------------------------------------------------------
def _knn_like(dev):
    """2 500 nodes, 64 neighbours each with repeats, multiplicities 1 .. 8 in the id words."""
    from dream_gnn_amd import ops

    if "knn" not in _staged:
        rng = np.random.default_rng(64)
        n, k = 2500, 64
        dst = np.repeat(np.arange(n, dtype=np.int32), k)
        src = rng.integers(0, n, n * k).astype(np.int32)
        sl = ops.SlicedCSR(_t(dst, dev), _t(src, dev), n, n, n_slices=8)
        mult = _t(rng.integers(0, 8, n * k).astype(np.int32), dev)
        _staged["knn"] = (sl, (sl.indices | (mult[sl.eid.long()] << ops.MULT_SHIFT)).contiguous())
    return _staged["knn"]


@pytest.mark.parametrize("graph", ["designed", "knn"])
def test_owned_bf16_is_bitwise_the_pair_and_the_fp32_owned_kernel_on_randn(dev, graph):
    """The same call with ``sliced_owned`` 0 and 1 on ``randn`` tables rounded by ``dgmi_rows_to_bf16`` (every sum
    rounds): identical bits, with and without multiplicities, ``dst_scale`` and the epilogue, at F = 128 and 344 — and
    identical to ``spmm_owned_kernel`` on the upcast table: same segment sums, same order, another lane-group width."""
    from dream_gnn_amd import ops

    if graph == "designed":
        st = _stage(dev)
        sl, ids = st["sl"], st["ids"]
    else:
        sl, ids = _knn_like(dev)
    gen = torch.Generator(device="cpu").manual_seed(19)
    for F in (128, 344):
        Xb = ops.rows_to_bf16(torch.randn(sl.n_src, F, generator=gen).to(dev))
        Xf = Xb.float()
        ds = (torch.rand(sl.n_dst, generator=gen) + 0.5).to(dev)
        mask = _t(C.out_mask(sl.n_dst, F, 2), dev)
        for id_mult, has_ds, epi in itertools.product((False, True), (False, True), (False, True)):
            form = (sl, ids if id_mult else sl.indices, id_mult)
            rest = (ds if has_ds else None, mask if epi else None)
            _set(sliced_owned=0)
            pair = _product(*form, Xb, *rest)
            assert float(pair.abs().max()) > 1.0
            _set(sliced_owned=1)
            assert torch.equal(_product_f32(*form, Xf, *rest), pair), (F, id_mult, has_ds, epi, "fp32 owned kernel")
            for knobs in (dict(), dict(sliced_owned_grid=19, sliced_owned_rows=2), dict(sliced_lpr=8, sliced_owned_grid=3),
                          dict(sliced_lpr=32, sliced_owned_grid=8, sliced_owned_lds_rows=40), dict(sliced_no_off32=1),
                          dict(sliced_owned_lag=0, sliced_owned_spin_ticks=1, sliced_owned_wgs=2)):  # ignored for bf16
                _set(sliced_owned=1, **knobs)
                assert torch.equal(_product(*form, Xb, *rest), pair), (F, id_mult, has_ds, epi, knobs)


# ---------------------------------------------------------------------------------------------
# (4) other slice counts
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_slices", [3, 16, 64])
def test_owned_bf16_on_other_slice_counts(dev, n_slices):
    """Layouts of 3, 16 and 64 slices (64 over 40 sources: empty trailing slices): exact against the design's reference
    and equal to the pair on that layout.  (64 slices x 3 column rounds is beyond 128 phases: the pair's product.)"""
    st = _stage(dev, n_slices)
    d, sl = st["d"], st["sl"]
    some = [dict(), dict(sliced_lpr=8, sliced_owned_grid=3, sliced_owned_rows=2), dict(sliced_lpr=32, sliced_owned_grid=19),
            dict(sliced_lpr=16, sliced_owned_grid=8, sliced_owned_lds_rows=_cap(d.n_dst, 8, 2))]
    for F, kind in itertools.product((8, 128, 344), ("unit", "mult")):
        X = C.features(d.n_src, F, 7 * F + n_slices)
        mask = C.out_mask(d.n_dst, F, F + 1)
        Xb, mask_d = _t(X, dev).to(BF16), _t(mask, dev)
        ids = st["ids"] if kind == "mult" else sl.indices
        want = _t(C.reference(d.dst, d.src, d.n_dst, X, d.mult if kind == "mult" else None, None, d.ds, None, mask, True), dev)
        _set(sliced_owned=0)
        assert torch.equal(_product(sl, ids, kind == "mult", Xb, st["ds"], mask_d), want), (F, kind, "pair")
        for knobs in some:
            _set(sliced_owned=1, **knobs)
            assert torch.equal(_product(sl, ids, kind == "mult", Xb, st["ds"], mask_d, ld_y=F + 4), want), (F, kind, knobs)
    # randn: every sum rounds
    gen = torch.Generator(device="cpu").manual_seed(n_slices)
    Xb = torch.randn(d.n_src, 128, generator=gen).to(dev).to(BF16)
    for id_mult in (False, True):
        form = (sl, st["ids"] if id_mult else sl.indices, id_mult, Xb, st["ds"])
        _set(sliced_owned=0)
        pair = _product(*form)
        _set(sliced_owned=1)
        assert torch.equal(_product(*form), pair), id_mult
    _set(sliced_owned=1)
    names = _kernels_of(lambda: _product(sl, sl.indices, False, Xb))
    assert "spmm_owned_bf16_kernel" in names and "reduce_planes_kernel" not in names, names


# ---------------------------------------------------------------------------------------------
# (5) what the form does not take
# ---------------------------------------------------------------------------------------------
def test_forms_the_owned_bf16_kernel_does_not_take_fall_back_to_the_pair(dev):
    """A value stream, dropout on the fly, forced chunking, a plan beyond 128 phases (one workgroup, two LDS rows:
    154 row rounds) and a forced ``sliced_owned_slices`` with ``sliced_owned = 1``: the pair's kernels and the pair's
    bits."""
    from dream_gnn_amd import ops

    st = _stage(dev)
    d, sl = st["d"], st["sl"]
    gen = torch.Generator(device="cpu").manual_seed(4)
    Xb = torch.randn(d.n_src, 128, generator=gen).to(dev).to(BF16)
    vals = torch.randn(d.dst.size, generator=gen).to(dev)
    desc = ops.random_subset_select(d.dst.size, int(d.dst.size * C.DROP_KEEP), C.DROP_SEED, dev)
    forms = {"value stream": (lambda: sl.spmm(Xb, vals=vals), {}),
             "dropout on the fly": (lambda: sl.spmm(Xb, keep=desc), {}),
             "forced chunking": (lambda: sl.spmm(Xb), dict(sliced_chunk_rows=37)),
             "beyond 128 phases": (lambda: sl.spmm(Xb), dict(sliced_owned_grid=1, sliced_owned_lds_rows=2)),
             # the knob of the fp32 layout experiment: no layout is made for the owned form on behalf of a bf16 product
             "forced layout slice count, 8": (lambda: sl.spmm(Xb), dict(sliced_owned_slices=8)),
             "forced layout slice count, 16": (lambda: sl.spmm(Xb), dict(sliced_owned_slices=16, sliced_owned_grid=3))}
    for what, (run, knobs) in forms.items():
        _set(sliced_owned=0, **knobs)
        pair = run()
        _set(sliced_owned=1, **knobs)
        assert torch.equal(run(), pair), what
        names = _kernels_of(run)
        assert "spmm_owned_bf16_kernel" not in names and "reduce_planes_kernel" in names, (what, names)


# ---------------------------------------------------------------------------------------------
# (6) through the graph
# ---------------------------------------------------------------------------------------------
def _square(dev):
    """12 288 x 12 288, 48 edges per row: both directions take the XCD-local form, hence the bf16 gather, at F = 128."""
    from dream_gnn_amd import ops

    if "square" not in _staged:
        rng = np.random.default_rng(6)
        n, deg, F = 12288, 48, 128
        dst = np.repeat(np.arange(n), deg).astype(np.int32)
        src = rng.integers(0, n, dst.size).astype(np.int32)
        _staged["square"] = dict(G=ops.CSRGraph(_t(dst, dev), _t(src, dev), n, n), F=F,
                                 X=_t(rng.standard_normal((n, F)).astype(np.float32), dev),
                                 dY=_t(rng.standard_normal((n, F)).astype(np.float32), dev),
                                 ss=_t(rng.uniform(0.5, 1.5, n).astype(np.float32), dev),
                                 ds=_t(rng.uniform(0.5, 1.5, n).astype(np.float32), dev))
    return _staged["square"]


def test_graph_level_products_are_bitwise_equal_under_both_forms(dev):
    """``CSRGraph.spmm`` / ``spmm_t(gather_dtype=bfloat16)`` and ``ops.spmm_csr`` with autograd under ``sliced_owned``
    0 and 1: the same bits, from the owned kernel under 1."""
    from dream_gnn_amd import ops

    g = _square(dev)
    G, X, dY, ss, ds, F = g["G"], g["X"], g["dY"], g["ss"], g["ds"], g["F"]
    assert G.takes_bf16_gather(F) and G.takes_bf16_gather(F, transposed=True)
    got = {}
    for flag in (0, 1):
        _set(sliced_owned=flag)
        x = X.clone().requires_grad_(True)
        y = ops.spmm_csr(G, x, ss, ds, gather_dtype=BF16)
        y.backward(dY)
        got[flag] = (G.spmm(X, ss, ds, gather_dtype=BF16), G.spmm_t(dY, ss, ds, gather_dtype=BF16), y.detach(), x.grad)
    for a, b in zip(got[0], got[1]):
        assert torch.equal(a, b)
    assert torch.equal(got[1][0], got[1][2]) and torch.equal(got[1][1], got[1][3])
    assert not torch.equal(got[1][0], G.spmm(X, ss, ds))  # it is the bf16 product
    _set(sliced_owned=1)
    for run in (lambda: G.spmm(X, ss, ds, gather_dtype=BF16), lambda: G.spmm_t(dY, ss, ds, gather_dtype=BF16)):
        names = _kernels_of(run)
        assert "spmm_owned_bf16_kernel" in names and "reduce_planes_kernel" not in names, names


def test_owned_bf16_product_records_into_a_hip_graph(dev):
    """One product with ``sliced_owned = 1`` captured after a warm-up call and replayed twice on a refreshed table: the
    bits of the eager pair."""
    g = _square(dev)
    G, ss, ds = g["G"], g["ss"], g["ds"]
    x = g["X"].clone()
    _set(sliced_owned=1)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        G.spmm(x, ss, ds, gather_dtype=BF16)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        y_c = G.spmm(x, ss, ds, gather_dtype=BF16)
    for seed in (1, 2):
        x.copy_(torch.randn(x.shape, generator=torch.Generator(device="cpu").manual_seed(seed)))
        _set(sliced_owned=1)
        graph.replay()
        torch.cuda.synchronize()
        got = y_c.clone()
        _set(sliced_owned=0)
        assert torch.equal(got, G.spmm(x, ss, ds, gather_dtype=BF16)), seed
