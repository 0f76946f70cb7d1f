"""The owned form's SCALED product (csrc/dgmi_owned_kernel.h ``SCALED``, include/dgmi_scale.h): the scale of the gathered
rows as a code in the id words, read from a table in LDS, instead of the pass that scales ``X`` beforehand.

Its contract is BIT EQUALITY with ``scale_rows`` + the plain owned product on the same layout — the gathered row is
multiplied by its scale, rounded once, before it joins the same sum — so every comparison here is of ``int32`` views
(NaN payloads and signed zeros included).  The owned form is forced through ``set_tuning`` as in
test_gpu_spmm_owned_slices.py, on that file's 301 x 330 graph of 16 slices and on ``_spmm_cases.sliced_design(8)``: designed
(row, slice) segments of length 0, 1, W - 1, W, W + 1, 2 W + 1 in the first, a middle and the last slice — the path edges
of the rolling gather window and of its hand-over — at F = 128 and at F = 100 (seven idle lanes of a 32-lane group).

Then ``ops.CSRGraph``: which products take the route, that every declined one is today's product, the cache of coded id
words, and a stream capture."""
import itertools

import numpy as np
import pytest
import torch

import _spmm_cases as C
from test_gpu_spmm_owned_slices import KNOBS as _SLICE_KNOBS, _cap, _t, design16

pytestmark = pytest.mark.gpu

KNOBS = dict(_SLICE_KNOBS, sliced_owned_scaled=-1)
SHIFT, BITS = 17, 11


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


def _bits(t):
    return t.contiguous().view(torch.int32)


def _same(a, b):
    return torch.equal(_bits(a), _bits(b))


_staged = {}


def _stage(dev, n_slices):
    from dream_gnn_amd import ops

    if n_slices not in _staged:
        d = design16() if n_slices == 16 else C.sliced_design(8)
        sl = ops.SlicedCSR(_t(d.dst, dev), _t(d.src, dev), d.n_dst, d.n_src, n_slices=n_slices)
        assert int(sl.range_flag) == 0
        ids = (sl.indices | ((_t(d.mult, dev) - 1)[sl.eid.long()] << ops.MULT_SHIFT)).contiguous()
        _staged[n_slices] = dict(d=d, sl=sl, ds=_t(d.ds, dev), ids=ids)
    return _staged[n_slices]


def _plain(sl, ids, id_mult, X, ds=None, mask=None):
    """``dgmi_spmm_sliced_f32`` (the plain owned kernel under ``sliced_owned = 1``) on plain id words."""
    from dream_gnn_amd import _lib

    n_dst, F = sl.n_dst, X.shape[1]
    y = torch.full((n_dst, F), float("nan"), device=X.device)
    nbytes = _lib.lib.dgmi_spmm_sliced_planes_bytes(n_dst, sl.n_slices, F)
    planes = torch.empty(max(nbytes // 4, 4), dtype=torch.float32, device=X.device)
    epi = (1, C.SLOPE, mask.data_ptr(), mask.stride(0), C.MASK_SCALE) if mask is not None else (0, 0.0, None, 0, 1.0)
    _lib.check(_lib.lib.dgmi_spmm_sliced_f32(
        sl.segptr.data_ptr(), ids.data_ptr(), None, None, None, 0, X.data_ptr(), X.stride(0), None,
        None if ds is None else ds.data_ptr(), y.data_ptr(), F, n_dst, sl.n_src, F, sl.n_slices, 0, int(id_mult),
        planes.data_ptr(), nbytes, *epi, torch.cuda.current_stream().cuda_stream), "dgmi_spmm_sliced_f32")
    return y


def _scaled(sl, words, table, id_mult, X, ds=None, mask=None):
    """``dgmi_spmm_owned_scaled_f32``; None when it declines (``Y`` then untouched)."""
    from dream_gnn_amd import _lib

    y = torch.full((sl.n_dst, X.shape[1]), float("nan"), device=X.device)
    epi = (1, C.SLOPE, mask, C.MASK_SCALE) if mask is not None else (0, 0.0, None, 1.0)
    took = _lib.spmm_owned_scaled(sl.segptr, words, X, table, ds, y, sl.n_src, sl.n_slices, id_mult, epi)
    if not took:
        assert bool(torch.isnan(y).all()), "a declined product wrote Y"
        return None
    return y


def _kernels(run):
    with torch.profiler.profile(activities=[torch.profiler.ProfilerActivity.CUDA]) as prof:
        run()
        torch.cuda.synchronize()
    return " ".join(e.key for e in prof.key_averages())


def _scales(n, kind, seed):
    """A scale vector of ``n`` entries with 1, 2, 37 or ``n`` distinct values, or one of the two with special values:
    ``"nan"`` holds +-0 and a NaN of the payload 0x7fc00123, ``"inf"`` holds +-0 and +-inf.

    Two vectors, so that a row's sum never meets two DIFFERENT NaNs: under ``"nan"`` every NaN is the table's own (a
    mangled payload or sign shows), under ``"inf"`` every NaN is the one ``inf - inf`` generates.  A row that summed one
    of each would hand on whichever stood first in a commutative add, an order the compiler picks per unrolled site in
    either kernel (with both in one vector, 0xffc00000 met 0x7fc00000 in row 103 of the 8-slice design).  That every
    payload keeps a code of its own is a property of the table (test_scale_codes_host.py)."""
    rng = np.random.default_rng(seed)
    if kind in ("nan", "inf"):
        special = np.array([0x7FC00123], np.uint32).view(np.float32) if kind == "nan" else np.array([np.inf, -np.inf], np.float32)
        pool = np.concatenate([np.array([0.0, -0.0, 1.5, -3.0, 0.75], np.float32), special])
        s = pool[rng.integers(0, pool.size, n)]
        s[:pool.size] = pool
        return s
    k = n if kind == "all" else int(kind)
    values = (0.25 + rng.permutation(4096)[:k] / 1024.0).astype(np.float32)
    s = values[rng.integers(0, k, n)]
    s[:k] = values
    return s


SETTINGS = (dict(sliced_owned_grid=3), dict(sliced_owned_grid=19, sliced_owned_rows=2), dict(sliced_owned_grid=1, sliced_owned_workers=1),
            dict(sliced_owned_grid=3, sliced_owned_lds_rows=-1))  # -1: two row rounds (_cap)


@pytest.mark.parametrize("F", [128, 100])
@pytest.mark.parametrize("kind", ["unit", "mult"])
@pytest.mark.parametrize("n_slices", [16, 8])
def test_scaled_is_bitwise_the_prescaled_plain_product(dev, n_slices, kind, F):
    """Scales of 1, 2, 37 and ``n_src`` distinct values, one of +-0 and a NaN with a payload, one of +-0 and +-inf (``_scales``),
    with and without ``dst_scale`` and the epilogue, on randn rows, over grids, row rounds and worker counts: the bits of
    ``scale_rows`` + the plain owned product, for every element — the designed segments of every window path edge among
    them, every NaN with its sign and payload."""
    from dream_gnn_amd import ops

    st = _stage(dev, n_slices)
    d, sl = st["d"], st["sl"]
    id_mult = kind == "mult"
    ids = st["ids"] if id_mult else sl.indices
    gen = torch.Generator(device="cpu").manual_seed(7 * F + n_slices)
    X = torch.randn(d.n_src, F, generator=gen).to(dev)
    mask = _t(C.out_mask(d.n_dst, F, 3), dev)
    for which, s_kind in enumerate(("1", "2", "37", "all", "nan", "inf")):
        s = _t(_scales(d.n_src, s_kind, 50 + which), dev)
        table, words = ops.CSRGraph.scale_codes(s, ids)
        assert table.numel() == (d.n_src if s_kind == "all" else torch.unique(_bits(s)).numel())
        if s_kind in ("nan", "inf"):
            assert table.numel() == (6 if s_kind == "nan" else 7)  # +-0, the NaN / +-inf and the finite values: all told apart
        Xs = ops._T.scale_rows(X, s)
        for knobs in SETTINGS:
            if knobs.get("sliced_owned_lds_rows") == -1:
                knobs = dict(knobs, sliced_owned_lds_rows=_cap(d.n_dst, 3, 2))
            _set(sliced_owned=1, sliced_lpr=32, **knobs)
            for has_ds, epi in itertools.product((False, True), (False, True)):
                args = (st["ds"] if has_ds else None, mask if epi else None)
                want = _plain(sl, ids, id_mult, Xs, *args)
                got = _scaled(sl, words, table, id_mult, X, *args)
                assert got is not None, "declined: %s" % (knobs,)
                if s_kind in ("nan", "inf") and not (has_ds or epi):
                    assert bool(torch.isnan(want).any()), "the design has no NaN to compare"
                diff = (_bits(got) != _bits(want)).any(1).nonzero().flatten().tolist()
                where = (_bits(got) != _bits(want)).nonzero()[:1].tolist()
                assert not diff, "%d slices %s F=%d scale %s %s ds=%s epi=%s: rows %s differ (designed: %s); first %s: %s" % (
                    n_slices, kind, F, s_kind, knobs, has_ds, epi, diff[:8], sorted(r for r, _ in d.designed if r in diff), where,
                    [hex(int(_bits(t)[r, c]) & 0xFFFFFFFF) for t in (got, want) for r, c in where])


@pytest.mark.parametrize("kind", ["unit", "mult"])
def test_scaled_matches_the_integer_reference_with_power_of_two_scales(dev, kind):
    """Integer rows, integer multiplicities and scales of 0.5 / 1 / 2 (``sliced_design(8)``'s ``ss``): the integer
    reference at zero tolerance, with ``dst_scale`` and the epilogue."""
    from dream_gnn_amd import ops

    st = _stage(dev, 8)
    d, sl = st["d"], st["sl"]
    id_mult = kind == "mult"
    ids = st["ids"] if id_mult else sl.indices
    table, words = ops.CSRGraph.scale_codes(_t(d.ss, dev), ids)
    assert table.numel() == 3
    for F in (128, 100):
        Xn, mask = C.features(d.n_src, F, 21 + F), C.out_mask(d.n_dst, F, 4)
        _set(sliced_owned=1, sliced_lpr=32, sliced_owned_grid=3)
        for has_ds, epi in itertools.product((False, True), (False, True)):
            want = _t(C.reference(d.dst, d.src, d.n_dst, Xn, d.mult if id_mult else None, d.ss, d.ds if has_ds else None, None,
                                  mask if epi else None, epi), dev)
            got = _scaled(sl, words, table, id_mult, _t(Xn, dev), st["ds"] if has_ds else None, _t(mask, dev) if epi else None)
            assert got is not None and torch.equal(got, want), (kind, F, has_ds, epi)


def _field_graph(dev, n_src):
    """40 rows over ``n_src`` sources: every row reads id 0 once and the last id eight-fold, plus a few random ids; the scale
    has exactly 2048 distinct values, the smallest at id 0 (code 0), the largest at id 2047 mod 2048 (code 2047)."""
    from dream_gnn_amd import ops

    rng = np.random.default_rng(77)
    n_dst = 40
    rows = np.repeat(np.arange(n_dst), 12)
    cols = rng.integers(0, n_src, rows.size)
    mult = rng.integers(1, 9, rows.size)
    cols[0::12], mult[0::12] = 0, 1
    cols[1::12], mult[1::12] = n_src - 1, 8
    sl = ops.SlicedCSR(_t(rows.astype(np.int32), dev), _t(cols.astype(np.int32), dev), n_dst, n_src, n_slices=8)
    ids = (sl.indices | ((_t(mult.astype(np.int32), dev) - 1)[sl.eid.long()] << ops.MULT_SHIFT)).contiguous()
    s = (1.0 + (np.arange(n_src) % 2048) / 4096.0).astype(np.float32)
    return sl, ids, _t(s, dev)


def test_field_edges_of_the_id_word(dev):
    """``n_src = 131072`` at F = 8: the word ``0x7fffffff`` (id 131071, code 2047, multiplicity 8) and the word 0 (id 0,
    code 0, multiplicity 1) are among the edges, and the product is the pre-scaled one bit for bit."""
    from dream_gnn_amd import ops

    n_src = 1 << SHIFT
    sl, ids, s = _field_graph(dev, n_src)
    table, words = ops.CSRGraph.scale_codes(s, ids)
    assert table.numel() == 1 << BITS
    assert int((words == 0x7FFFFFFF).sum()) == 40 and int((words == 0).sum()) == 40
    assert torch.equal(words & (n_src - 1), ids & (n_src - 1)) and torch.equal(words >> ops.MULT_SHIFT, ids >> ops.MULT_SHIFT)
    X = torch.randn(n_src, 8, generator=torch.Generator(device="cpu").manual_seed(5)).to(dev)
    _set(sliced_owned=1, sliced_lpr=32, sliced_owned_grid=3)
    got = _scaled(sl, words, table, True, X)
    assert got is not None and _same(got, _plain(sl, ids, True, ops._T.scale_rows(X, s)))


def test_entry_point_declines_what_the_kernel_is_not_built_for(dev):
    """A width the kernel is not built at, 64-bit offsets, a forced gate or two-workgroup form, ``sliced_owned = 0``,
    ``sliced_owned_scaled = 0``, the built-in rule on a small product, ``n_src`` above 2^17 and a table above 2048 entries:
    ``taken = 0`` and ``Y`` untouched, and the host query says the same."""
    from dream_gnn_amd import _lib, ops

    st = _stage(dev, 16)
    d, sl = st["d"], st["sl"]
    X = torch.randn(d.n_src, 128, generator=torch.Generator(device="cpu").manual_seed(6)).to(dev)
    table, words = ops.CSRGraph.scale_codes(_t(_scales(d.n_src, "37", 1), dev), sl.indices)
    query = lambda n_src=d.n_src, n=37: _lib.owned_scaled_takes(d.n_dst, n_src, 128, 128, 16, False, n)
    _set(sliced_owned=1, sliced_owned_grid=3)
    assert query() and _scaled(sl, words, table, False, X) is not None
    for knobs in (dict(sliced_lpr=8), dict(sliced_lpr=64), dict(sliced_no_off32=1), dict(sliced_owned_lag=0), dict(sliced_owned_wgs=2),
                  dict(sliced_owned=0), dict(sliced_owned_scaled=0), dict(sliced_owned=-1)):
        _set(**dict(dict(sliced_owned=1, sliced_owned_grid=3), **knobs))
        assert not query() and _scaled(sl, words, table, False, X) is None, knobs
    _set(sliced_owned=1, sliced_owned_grid=3)
    assert not query(n_src=(1 << SHIFT) + 1) and not query(n=(1 << BITS) + 1) and not query(n=0)
    assert query(n_src=1 << SHIFT, n=1 << BITS)


# ---------------------------------------------------------------------------------------------
# ops.CSRGraph
# ---------------------------------------------------------------------------------------------
@pytest.fixture
def routed(monkeypatch):
    """Small graphs take the XCD-local form and its pre-scale pass, as large ones do by rule."""
    from dream_gnn_amd import ops

    monkeypatch.setattr(ops, "FORCE_KERNEL", "sliced")
    monkeypatch.setattr(ops.SlicedCSR, "_prescale_rule", staticmethod(lambda *a: True))
    _set(sliced_owned=1, sliced_owned_slices=16, sliced_owned_grid=3, sliced_lpr=32)
    return monkeypatch


def _graph(dev, weighted=False):
    from dream_gnn_amd import ops

    d = design16()
    g = ops.CSRGraph(_t(d.dst, dev), _t(d.src, dev), d.n_dst, d.n_src)
    if weighted:  # D^-1 M: a row scale times a multiplicity — its transposed product gathers the scaled rows
        row_scale = _t((0.25 + np.arange(d.n_dst) % 7 / 8.0).astype(np.float32), dev)
        g = g.with_values(row_scale[_t(d.dst, dev).long()] * _t(d.mult, dev).float())
    return d, g


def _today(monkeypatch, run):
    """``run()`` with the route switched off in ``ops``: the pre-scale pass and the plain product."""
    from dream_gnn_amd import ops

    monkeypatch.setattr(ops, "SCALE_CODES", False)
    try:
        return run()
    finally:
        monkeypatch.setattr(ops, "SCALE_CODES", True)


def test_csrgraph_takes_the_route_and_gives_todays_bits(dev, routed):
    """A unit-value product with ``src_scale`` and the transposed product of a ``scale x multiplicity`` graph launch the
    scaled kernel and no ``scale_rows_kernel``; both are bit for bit the products of the pre-scale pass."""
    d, g = _graph(dev)
    gen = torch.Generator(device="cpu").manual_seed(31)
    X, dY = torch.randn(d.n_src, 128, generator=gen).to(dev), torch.randn(d.n_dst, 128, generator=gen).to(dev)
    s, ds = _t(_scales(d.n_src, "37", 2), dev), _t(d.ds, dev)
    names = _kernels(lambda: g.spmm(X, s, ds))
    assert "spmm_owned_scaled_kernel" in names and "scale_rows_kernel" not in names, names
    assert _same(g.spmm(X, s, ds), _today(routed, lambda: g.spmm(X, s, ds)))
    assert g._S.scale_builds == 1
    _, gw = _graph(dev, weighted=True)
    names = _kernels(lambda: gw.spmm_t(dY))
    assert "spmm_owned_scaled_kernel" in names and "scale_rows_kernel" not in names, names
    assert _same(gw.spmm_t(dY), _today(routed, lambda: gw.spmm_t(dY))) and gw._S.scale_builds == 1
    want = torch.zeros(d.n_src, 128, dtype=torch.float64, device=dev).index_add_(
        0, _t(d.src, dev).long(), dY.double()[_t(d.dst, dev).long()] * gw._coo_vals.double()[:, None])
    assert torch.allclose(gw.spmm_t(dY).double(), want, rtol=1e-5, atol=1e-4)  # 13 terms of at most 8.2 x 5 at 6e-8: 3e-5


def test_csrgraph_declined_products_are_todays(dev, routed):
    """2049 distinct values, ``n_src = 131073``, ``sliced_owned = 0``, a dropped view, a bf16 gather and a folded scale: no
    scaled kernel, and the bits of the product with the route switched off."""
    from dream_gnn_amd import ops

    def check(g, run, builds=None):
        before = g._S.scale_builds
        names = _kernels(lambda: run())
        assert "spmm_owned_scaled_kernel" not in names, names
        assert _same(run(), _today(routed, run))
        if builds is not None:
            assert g._S.scale_builds - before == builds

    d, g = _graph(dev)
    gen = torch.Generator(device="cpu").manual_seed(32)
    X, dY = torch.randn(d.n_src, 128, generator=gen).to(dev), torch.randn(d.n_dst, 128, generator=gen).to(dev)
    s = _t(_scales(d.n_src, "37", 3), dev)
    _set(sliced_owned=0, sliced_owned_slices=16, sliced_owned_grid=3, sliced_lpr=32)
    check(g, lambda: g.spmm(X, s), builds=0)
    _set(sliced_owned=1, sliced_owned_slices=16, sliced_owned_grid=3, sliced_lpr=32)
    desc = ops.random_subset_select(d.dst.size, int(d.dst.size * C.DROP_KEEP), C.DROP_SEED, dev)
    view = g.dropped(desc)
    check(view, lambda: view.spmm(X, s), builds=0)
    check(g, lambda: g.spmm(X, s, gather_dtype=torch.bfloat16), builds=0)
    _, gw = _graph(dev, weighted=True)
    extra = _t(_scales(d.n_dst, "2", 4), dev)
    check(gw, lambda: gw.spmm_t(dY, None, extra), builds=0)  # the graph's own scale folded with the caller's
    for n_src, n_values in ((2500, 2049), ((1 << SHIFT) + 1, 16)):
        rng = np.random.default_rng(n_src)
        rows, cols = np.repeat(np.arange(48), 40).astype(np.int32), rng.integers(0, n_src, 48 * 40).astype(np.int32)
        cols[:2] = (0, n_src - 1)
        big = ops.CSRGraph(_t(rows, dev), _t(cols, dev), 48, n_src)
        sv = (1.0 + (np.arange(n_src) % n_values) / 4096.0).astype(np.float32)
        Xb, sd = torch.randn(n_src, 8, generator=gen).to(dev), _t(sv, dev)
        check(big, lambda: big.spmm(Xb, sd))
    # and exactly 2048 values on the same shape are taken
    big = ops.CSRGraph(_t(rows, dev), _t(cols % 2500, dev), 48, 2500)
    sv, Xb = _t((1.0 + (np.arange(2500) % 2048) / 4096.0).astype(np.float32), dev), torch.randn(2500, 8, generator=gen).to(dev)
    assert "spmm_owned_scaled_kernel" in _kernels(lambda: big.spmm(Xb, sv))
    assert _same(big.spmm(Xb, sv), _today(routed, lambda: big.spmm(Xb, sv)))


def test_csrgraph_cache_of_coded_words(dev, routed):
    """One build per scale tensor; ``reshape`` and slice views of its storage hit; an in-place update rebuilds and gives the
    new product; an equal-valued other tensor gives the right product; two misses in a row switch the route off."""
    d, g = _graph(dev)
    X = torch.randn(d.n_src, 128, generator=torch.Generator(device="cpu").manual_seed(33)).to(dev)
    store = torch.zeros(d.n_src + 6, device=dev)
    s = store[:d.n_src]
    s.copy_(_t(_scales(d.n_src, "37", 5), dev))
    today = lambda sc: _today(routed, lambda: g.spmm(X, sc))
    builds = lambda: g._S.scale_builds
    y = g.spmm(X, s)
    assert builds() == 1 and _same(y, today(s))
    for view in (s, s.reshape(-1), s.reshape(-1, 1), store[:d.n_src], s.view(d.n_src)):
        assert _same(g.spmm(X, view), y) and builds() == 1
    s.mul_(2)
    y2 = g.spmm(X, s)
    assert builds() == 2 and _same(y2, today(s)) and not _same(y2, y)
    assert _same(g.spmm(X, s), y2) and builds() == 2  # a hit: the miss counter starts over
    other = s.clone()
    assert _same(g.spmm(X, other), y2) and builds() == 3  # another storage: one rebuild
    assert _same(g.spmm(X, other), y2) and builds() == 3
    # two misses in a row: the route goes off for this view and layout, the products stay right
    a, b = other.clone(), (other * 0.5)
    assert _same(g.spmm(X, a), y2) and builds() == 4
    names = _kernels(lambda: g.spmm(X, b))
    assert builds() == 4 and "spmm_owned_scaled_kernel" not in names and "scale_rows_kernel" in names, names
    assert _same(g.spmm(X, b), today(b)) and _same(g.spmm(X, s), y2) and builds() == 4


def test_captured_product_takes_the_prescale_pass(dev, routed):
    """Recorded under ``torch.cuda.graph`` the product is the pre-scale pass and the plain kernel, so a replay after
    ``s.copy_(new)`` gives the product of the new values."""
    d, g = _graph(dev)
    gen = torch.Generator(device="cpu").manual_seed(34)
    X = torch.randn(d.n_src, 128, generator=gen).to(dev)
    s = _t(_scales(d.n_src, "37", 6), dev)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        g.spmm(X, s)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    built = g._S.scale_builds
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        y_c = g.spmm(X, s)
    assert g._S.scale_builds == built
    for seed in (7, 8):
        new = _t(_scales(d.n_src, "all", seed), dev)
        s.copy_(new)
        graph.replay()
        torch.cuda.synchronize()
        assert _same(y_c, g.spmm(X, new.clone())), seed
