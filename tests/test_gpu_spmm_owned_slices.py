"""The workgroup-owned form of the XCD-local SpMM (csrc/dgmi_owned.hip) on layouts of 3, 16 and 64 source slices: the
slice count is a field of its plan.  Forced with ``sliced_owned = 1`` through the C ABI, as in test_gpu_spmm_owned.py, on
designed integer operands at ZERO tolerance (``torch.equal`` with the integer reference AND with the pair of launches on the
same layout) and bit for bit against the pair on ``randn`` operands: a row's sum joins its segment sums in slice order
from +0 in both forms, whatever the slice count.

The 16-slice graph is designed here (``_spmm_cases.sliced_design`` has none): 301 rows over 330 sources — 16 slices of
21 columns, the last one of 15 — with one (row, slice) segment of every length 0, 1, W - 1, W, W + 1, 2 W + 1
(W = ``kOwnedWindow`` = 4: the lengths at which the rolling gather window changes its path) in slice 0, in two middle
slices and in slice 15, each in a row that has no other edge (so there are rows whose only edges lie in the LAST slice,
the phase that writes ``Y``), a background of 0 .. 12 edges per row over all slices, and empty rows in the middle and at
the end.

A setting whose plan would exceed 128 phases (64 slices x 2 column rounds x 2 row rounds, ...) is not taken by the form
and must come back as the pair's product; both are held to the same reference.

The last tests are about ``ops.CSRGraph``: which layout a product runs on (``dgmi_sliced_layout_slices``) depends on the
product alone, products the owned form cannot take run on the 8-slice layout exactly as before, and that layout is only
built when such a product arrives."""
import itertools
from collections import namedtuple

import numpy as np
import pytest
import torch

import _spmm_cases as C

pytestmark = pytest.mark.gpu

W = 4  # kOwnedWindow (csrc/dgmi_owned_common.h; test_owned_window_host.py pins it)
N_DST, N_SRC, N_SLICES = 301, 330, 16
LENGTHS = (0, 1, W - 1, W, W + 1, 2 * W + 1)
DESIGNED_SLICES = (0, 5, 10, 15)
EMPTY_ROWS = (110, 111, 112, 298, 299, 300)

KNOBS = dict(sliced_owned=-1, sliced_owned_slices=0, sliced_owned_grid=0, sliced_owned_rows=0, sliced_owned_lds_rows=0,
             sliced_owned_lag=-2, sliced_owned_spin_ticks=0, sliced_owned_wgs=0, sliced_owned_workers=0, sliced_lpr=0,
             sliced_no_off32=0, sliced_chunk_rows=0)

Design = namedtuple("Design", "n_dst n_src n_slices dst src mult ds designed seglen")


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


_designs = {}


def design16():
    if 16 in _designs:
        return _designs[16]
    rng = np.random.default_rng(1016)
    slice_of = C.col_slices(N_SRC, N_SLICES)
    assert np.array_equal(np.unique(slice_of), np.arange(N_SLICES)), "every slice holds columns"
    designed, dst, src = {}, [], []
    for k, (s, length) in enumerate(itertools.product(DESIGNED_SLICES, LENGTHS)):
        row = 3 + 11 * k
        designed[(row, s)] = length
        dst.append(np.full(length, row))
        src.append(rng.choice(np.flatnonzero(slice_of == s), length))
    free = np.setdiff1d(np.arange(N_DST), list(EMPTY_ROWS) + [r for r, _ in designed])
    deg = rng.integers(0, 13, free.size)
    dst.append(np.repeat(free, deg))
    src.append(rng.integers(0, N_SRC, int(deg.sum())))
    dst, src = np.concatenate(dst), np.concatenate(src)
    order = rng.permutation(dst.size)
    dst, src = dst[order].astype(np.int32), src[order].astype(np.int32)
    seglen = C.segment_lengths(dst, src, N_DST, N_SRC, N_SLICES)
    for (row, s), length in designed.items():
        assert seglen[s, row] == length and seglen[:, row].sum() == length
    assert len(designed) == len(LENGTHS) * len(DESIGNED_SLICES) and np.all(seglen[:, list(EMPTY_ROWS)] == 0)
    only_last = [r for r in range(N_DST) if seglen[15, r] > 0 and seglen[:15, r].sum() == 0]
    assert len(only_last) >= len(LENGTHS) - 1  # rows whose only edges lie in the last slice
    assert set(LENGTHS) <= set(seglen[0].tolist()) and set(LENGTHS) <= set(seglen[15].tolist())
    d = Design(N_DST, N_SRC, N_SLICES, dst, src, rng.integers(1, 9, dst.size).astype(np.int32),
               rng.choice([0.25, 0.5, 1.0, 2.0], N_DST).astype(np.float32), designed, seglen)
    for a in d:
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    _designs[16] = d
    return d


def _design(n_slices):
    return design16() if n_slices == 16 else C.sliced_design(n_slices)


_staged = {}


def _stage(dev, n_slices):
    from dream_gnn_amd import ops

    if n_slices not in _staged:
        d = _design(n_slices)
        sl = ops.SlicedCSR(_t(d.dst, dev), _t(d.src, dev), d.n_dst, d.n_src, n_slices=n_slices)
        assert int(sl.range_flag) == 0 and sl.n_slices == n_slices
        ids = (sl.indices | ((_t(d.mult, dev) - 1)[sl.eid.long()] << ops.MULT_SHIFT)).contiguous()
        _staged[n_slices] = dict(d=d, sl=sl, ds=_t(d.ds, dev), ids=ids)
    return _staged[n_slices]


def _product(sl, ids, id_mult, X, ds=None, epi_mask=None, ld_y=None):
    """``dgmi_spmm_sliced_f32`` on the layout ``sl`` with the id words ``ids``; ``ld_y``: leading dimension of ``Y`` (a
    view of a wider NaN-filled buffer, whose other columns must stay NaN)."""
    from dream_gnn_amd import _lib

    n_dst, F = sl.n_dst, X.shape[1]
    ld = F if ld_y is None else ld_y
    buf = torch.full((n_dst, ld), float("nan"), device=X.device)
    nbytes = _lib.lib.dgmi_spmm_sliced_planes_bytes(n_dst, sl.n_slices, F)
    planes = torch.empty(max(nbytes // 4, 4), dtype=torch.float32, device=X.device)
    epi = (1, C.SLOPE, epi_mask.data_ptr(), epi_mask.stride(0), C.MASK_SCALE) if epi_mask is not None else (0, 0.0, None, 0, 1.0)
    _lib.check(_lib.lib.dgmi_spmm_sliced_f32(
        sl.segptr.data_ptr(), ids.data_ptr(), None, None, None, 0, X.data_ptr(), X.stride(0), None,
        None if ds is None else ds.data_ptr(), buf.data_ptr(), ld, n_dst, sl.n_src, F, sl.n_slices, 0, int(id_mult),
        planes.data_ptr(), nbytes, *epi, torch.cuda.current_stream().cuda_stream), "dgmi_spmm_sliced_f32")
    if ld > F:
        assert bool(torch.isnan(buf[:, F:]).all()), "the product wrote outside its F columns"
    return buf[:, :F]


def _cap(n_dst, grid, rounds):
    """An LDS cap of ceil(B / k) rows gives k row rounds of a workgroup's B = ceil(n_dst / grid) rows."""
    B = -(-n_dst // grid)
    return 0 if rounds == 1 else -(-B // rounds)


def _settings(n_dst):
    """Grids 1 / 3 / 19 x 1 / 2 / 4 row rounds x one worker wave / all of them, then each lane-group width and R."""
    out = [dict(sliced_owned_grid=g, sliced_owned_lds_rows=_cap(n_dst, g, k), sliced_owned_workers=w)
           for g, k, w in itertools.product((1, 3, 19), (1, 2, 4), (1, 0))]
    out += [dict(sliced_owned_grid=3, sliced_lpr=w, sliced_owned_rows=r) for w, r in ((8, 1), (16, 5), (32, 2), (64, 0))]
    out += [dict(), dict(sliced_no_off32=1, sliced_owned_grid=19)]
    return out


def _phases(n_slices, F, knobs, n_dst):
    """Phases of the plan a setting gives (the launcher's arithmetic, for the settings of this file: the built-in width)."""
    lpr = knobs.get("sliced_lpr") or C.pick_lpr(F)
    grid = knobs.get("sliced_owned_grid") or 256
    B = -(-n_dst // grid)
    fit = (144 << 10) // (16 * lpr)
    cap = knobs.get("sliced_owned_lds_rows", 0)
    fit = min(fit, cap) if cap > 0 else fit
    return -(-B // fit) * -(-F // (4 * lpr)) * n_slices


def _kernels(run):
    with torch.profiler.profile(activities=[torch.profiler.ProfilerActivity.CUDA]) as prof:
        run()
        torch.cuda.synchronize()
    return " ".join(e.key for e in prof.key_averages())


@pytest.mark.parametrize("n_slices", [3, 16, 64])
def test_forced_form_launches_the_owned_kernel_at_any_slice_count(dev, n_slices):
    """A profiled call with ``sliced_owned = 1`` shows ``spmm_owned_kernel`` and no plane reduce on a layout of 3, 16
    and 64 slices; one whose plan exceeds 128 phases (64 slices, four row rounds) shows the pair, as does
    ``sliced_owned = 0``."""
    st = _stage(dev, n_slices)
    d = st["d"]
    X = _t(C.features(d.n_src, 128, 5), dev)
    run = lambda: _product(st["sl"], st["sl"].indices, False, X)
    _set(sliced_owned=1, sliced_owned_grid=3)
    assert _phases(n_slices, 128, dict(sliced_owned_grid=3), d.n_dst) == n_slices
    names = _kernels(run)
    assert "spmm_owned_kernel" in names and "reduce_planes_kernel" not in names, names
    _set(sliced_owned=0)
    names = _kernels(run)
    assert "spmm_owned_kernel" not in names and "reduce_planes_kernel" in names, names
    if n_slices == 64:
        knobs = dict(sliced_owned_grid=3, sliced_owned_lds_rows=_cap(d.n_dst, 3, 4))
        assert _phases(64, 128, knobs, d.n_dst) == 256
        _set(sliced_owned=1, **knobs)
        names = _kernels(run)
        assert "spmm_owned_kernel" not in names and "reduce_planes_kernel" in names, names


@pytest.mark.parametrize("F", [4, 128, 344])
@pytest.mark.parametrize("kind", ["unit", "mult"])
@pytest.mark.parametrize("n_slices", [3, 16, 64])
def test_owned_exact_on_designed_operands_at_any_slice_count(dev, n_slices, kind, F):
    """Unit ids and ids with multiplicities, ``dst_scale`` and the epilogue on and off, grids 1 / 3 / 19, 1 / 2 / 4 row
    rounds, one worker wave and all, every width, a strided ``Y``: the integer reference, and the pair on the same layout."""
    st = _stage(dev, n_slices)
    d, sl = st["d"], st["sl"]
    seed = 13 * F + n_slices
    X = C.features(d.n_src, F, seed)
    mask = C.out_mask(d.n_dst, F, seed + 1)
    w = d.mult if kind == "mult" else None
    ids = st["ids"] if kind == "mult" else sl.indices
    combos = list(itertools.product((False, True), (False, True)))
    want = {(has_ds, epi): _t(C.reference(d.dst, d.src, d.n_dst, X, w, None, d.ds if has_ds else None, None,
                                          mask if epi else None, epi), dev) for has_ds, epi in combos}
    Xd, mask_d = _t(X, dev), _t(mask, dev)
    _set(sliced_owned=0)
    for has_ds, epi in combos:
        pair = _product(sl, ids, kind == "mult", Xd, st["ds"] if has_ds else None, mask_d if epi else None)
        assert torch.equal(pair, want[has_ds, epi]), "the pair on %d slices, dst_scale=%s epilogue=%s" % (n_slices, has_ds, epi)
    taken = 0
    for i, knobs in enumerate(_settings(d.n_dst)):
        _set(sliced_owned=1, **knobs)
        taken += _phases(n_slices, F, knobs, d.n_dst) <= 128
        for has_ds, epi in combos:
            y = _product(sl, ids, kind == "mult", Xd, st["ds"] if has_ds else None, mask_d if epi else None,
                         ld_y=F + 8 if i % 2 else None)
            assert torch.equal(y, want[has_ds, epi]), "%d slices %s dst_scale=%s epilogue=%s: %d elements differ, first row %d" % (
                n_slices, knobs, has_ds, epi, int((y != want[has_ds, epi]).sum()), int((y != want[has_ds, epi]).any(1).nonzero()[0]))
    # most settings stay within 128 phases (at 64 slices and three column rounds only the 64-lane one does); the others
    # are not taken and are the pair's
    assert taken >= (1 if (n_slices, F) == (64, 344) else 16), taken


@pytest.mark.parametrize("n_slices", [3, 16, 64])
def test_owned_is_bitwise_the_pair_on_randn_at_any_slice_count(dev, n_slices):
    """The same call with ``sliced_owned`` 0 and 1 on ``randn`` operands: identical bits — sixteen (three, sixty-four)
    segment sums joined in slice order by both forms."""
    st = _stage(dev, n_slices)
    sl, d = st["sl"], st["d"]
    gen = torch.Generator(device="cpu").manual_seed(90 + n_slices)
    for F in (128, 344):
        X = torch.randn(sl.n_src, F, generator=gen).to(dev)
        ds = (torch.rand(sl.n_dst, generator=gen) + 0.5).to(dev)
        mask = _t(C.out_mask(sl.n_dst, F, 2), dev)
        for id_mult, has_ds, epi in itertools.product((False, True), (False, True), (False, True)):
            args = (sl, st["ids"] if id_mult else sl.indices, id_mult, X, ds if has_ds else None, mask if epi else None)
            _set(sliced_owned=0)
            pair = _product(*args)
            for knobs in (dict(), dict(sliced_owned_grid=19, sliced_owned_rows=2), dict(sliced_owned_grid=1, sliced_owned_workers=1),
                          dict(sliced_owned_grid=3, sliced_owned_lds_rows=_cap(d.n_dst, 3, 2)),
                          dict(sliced_owned_grid=3, sliced_owned_lds_rows=_cap(d.n_dst, 3, 4), sliced_owned_lag=1, sliced_owned_spin_ticks=1),
                          dict(sliced_owned_lag=0)):
                _set(sliced_owned=1, **knobs)
                assert torch.equal(_product(*args), pair), (n_slices, F, id_mult, has_ds, epi, knobs)


# ---------------------------------------------------------------------------------------------
# ops.CSRGraph: which layout a product runs on
# ---------------------------------------------------------------------------------------------
def _graph(dev):
    from dream_gnn_amd import ops

    d = design16()
    return d, ops.CSRGraph(_t(d.dst, dev), _t(d.src, dev), d.n_dst, d.n_src)


def _count_builds(monkeypatch):
    from dream_gnn_amd import ops

    built = []
    real = ops.SlicedCSR.from_csr.__func__

    def counting(cls, indptr, indices, eid, n_dst, n_src, n_slices=ops.SlicedCSR.N_SLICES):
        built.append(int(n_slices))
        return real(cls, indptr, indices, eid, n_dst, n_src, n_slices)

    monkeypatch.setattr(ops.SlicedCSR, "from_csr", classmethod(counting))
    return built


def test_csrgraph_builds_the_wide_layout_and_the_8_slice_one_only_on_demand(dev, monkeypatch):
    """With the knob forcing 16 slices a plain product of a small graph runs the owned kernel on a 16-slice layout and
    builds nothing else.  A ``keep``-on-the-fly product and a bf16-gather product of the same graph — which the owned
    form does not take — return exactly what they return with the knob at 8, on the 8-slice layout, which is built when
    the first of them arrives; the plain product is the integer reference either way."""
    from dream_gnn_amd import ops

    monkeypatch.setattr(ops, "FORCE_KERNEL", "sliced")
    d = design16()
    F = 128
    Xn = C.features(d.n_src, F, 7)
    X, ds = _t(Xn, dev), _t(d.ds, dev)
    want = _t(C.reference(d.dst, d.src, d.n_dst, Xn, None, None, d.ds), dev)
    desc = ops.random_subset_select(d.dst.size, int(d.dst.size * C.DROP_KEEP), C.DROP_SEED, dev)
    results = {}
    for slices in (8, 16):
        _set(sliced_owned=1, sliced_owned_slices=slices, sliced_owned_grid=3)
        built = _count_builds(monkeypatch)
        _, g = _graph(dev)
        names = _kernels(lambda: results.setdefault(("plain", slices), g.spmm(X, None, ds)))
        assert "spmm_owned_kernel" in names and "reduce_planes_kernel" not in names, names
        assert built == [slices] and g._sliced is not None and g._sliced.n_slices == slices and not g._S.wide
        assert torch.equal(results["plain", slices], want)
        g.spmm(X, None, ds)
        assert built == [slices]  # kept
        # edge dropout evaluated inside the kernel: the pair, on the 8-slice layout
        monkeypatch.setattr(ops, "COMPACT_DROPPED", False)
        view = g.dropped(desc)
        names = _kernels(lambda: results.setdefault(("keep", slices), view.spmm(X, None, ds)))
        assert "spmm_owned_kernel" not in names and "reduce_planes_kernel" in names, names
        assert built == ([8] if slices == 8 else [16, 8])
        # a bf16 gather: the pair, on the same 8-slice layout
        names = _kernels(lambda: results.setdefault(("bf16", slices), g.spmm(X, None, ds, gather_dtype=torch.bfloat16)))
        assert "spmm_owned_kernel" not in names and "reduce_planes_kernel" in names, names
        assert built == ([8] if slices == 8 else [16, 8])
        # a value stream: the pair, on the 8-slice layout
        rng = np.random.default_rng(3)  # (signed: no `scale x multiplicity` form, a real value stream)
        vals = _t((rng.integers(1, 5, d.dst.size) * rng.choice([-1, 1], d.dst.size)).astype(np.float32), dev)
        results["vals", slices] = g.with_values(vals).spmm(X, None, ds)
        assert built == ([8] if slices == 8 else [16, 8])
        # the compacted view of the wide layout runs the plain kernels: the owned form takes it
        monkeypatch.setattr(ops, "COMPACT_DROPPED", True)
        view = g.dropped(desc)
        names = _kernels(lambda: results.setdefault(("compacted", slices), view.spmm(X, None, ds)))
        assert "spmm_owned_kernel" in names, names
        assert built == ([8] if slices == 8 else [16, 8])
        # the transposed product has layouts of its own
        results["t", slices] = g.spmm_t(_t(C.features(d.n_dst, F, 8), dev))
        assert built == ([8, 8] if slices == 8 else [16, 8, 16])
        monkeypatch.undo()
        monkeypatch.setattr(ops, "FORCE_KERNEL", "sliced")
    for what in ("keep", "bf16", "vals", "compacted", "t"):
        assert torch.equal(results[what, 16], results[what, 8]), what
    kept = C.drop_mask(d.dst.size)
    want_kept = _t(C.reference(d.dst, d.src, d.n_dst, Xn, None, None, d.ds, kept), dev)
    assert torch.equal(results["keep", 16], want_kept) and torch.equal(results["compacted", 16], want_kept)


def test_csrgraph_layout_does_not_depend_on_the_order_of_products(dev, monkeypatch):
    """The 8-slice product first, the plain one second: the 8-slice layout sits in ``sliced``, the 16-slice one beside
    it, and every product returns the bits it returns in the other order."""
    from dream_gnn_amd import ops

    monkeypatch.setattr(ops, "FORCE_KERNEL", "sliced")
    d = design16()
    gen = torch.Generator(device="cpu").manual_seed(12)
    X = torch.randn(d.n_src, 128, generator=gen).to(dev)
    _set(sliced_owned=1, sliced_owned_slices=16, sliced_owned_grid=3)
    built = _count_builds(monkeypatch)
    _, a = _graph(dev)
    _, b = _graph(dev)
    ya = (a.spmm(X), a.spmm(X, gather_dtype=torch.bfloat16))
    assert built == [16, 8] and a._sliced.n_slices == 16 and a._S.wide[(False, 8)].n_slices == 8
    yb = (b.spmm(X, gather_dtype=torch.bfloat16), b.spmm(X))[::-1]
    assert built == [16, 8, 8, 16] and b._sliced.n_slices == 8 and b._S.wide[(False, 16)].n_slices == 16
    assert torch.equal(ya[0], yb[0]) and torch.equal(ya[1], yb[1])
    # and the plain product on 16 slices is the pair's on that layout
    _set(sliced_owned=0)
    assert torch.equal(a._sliced.spmm(X), ya[0])
