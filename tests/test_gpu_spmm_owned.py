"""The workgroup-owned form of the XCD-local SpMM (csrc/dgmi_owned.hip: rows summed in LDS, no partial planes), forced
with ``sliced_owned = 1``, on the designed integer operands of _spmm_cases.py at ZERO tolerance (``torch.equal``), and
bit for bit against the sliced pair (``sliced_owned = 0``) on ``randn`` operands.  Through the C ABI, so that ``Y`` may be
strided.  The products the form does not take must come back as the pair's with the knob set."""
import itertools

import numpy as np
import pytest
import torch

import _spmm_cases as C

pytestmark = pytest.mark.gpu

OWNED_DEFAULTS = dict(sliced_owned=-1, sliced_owned_grid=0, sliced_owned_rows=0, sliced_owned_lds_rows=0, sliced_owned_lag=-2,
                      sliced_owned_spin_ticks=0, sliced_lpr=0, sliced_no_off32=0, sliced_chunk_rows=0)


@pytest.fixture(autouse=True)
def _knobs_back_to_default():
    from dream_gnn_amd import _lib

    try:
        yield
    finally:
        for name, value in OWNED_DEFAULTS.items():
            _lib.set_tuning(name, value)


def _set(**knobs):
    from dream_gnn_amd import _lib

    for name, value in dict(OWNED_DEFAULTS, **knobs).items():
        _lib.set_tuning(name, value)


def _t(a, dev):
    return None if a is None else torch.from_numpy(np.array(a)).to(dev)


_staged = {}


def _stage(dev):
    from dream_gnn_amd import ops

    if "d" not in _staged:
        d = C.sliced_design(8)
        sl = ops.SlicedCSR(_t(d.dst, dev), _t(d.src, dev), d.n_dst, d.n_src, n_slices=8)
        order = sl.eid.long()
        _staged.update(d=d, sl=sl, ds=_t(d.ds, dev),
                       ids=(sl.indices | ((_t(d.mult, dev) - 1)[order] << ops.MULT_SHIFT)).contiguous())
    return _staged


def _product(sl, ids, id_mult, X, ds=None, epi_mask=None, ld_y=None):
    """``dgmi_spmm_sliced_f32`` on the layout ``sl`` with the id words ``ids``; ``ld_y``: leading dimension of ``Y`` (a
    view of a wider NaN-filled buffer, whose other columns must stay NaN)."""
    from dream_gnn_amd import _lib

    n_dst, F = sl.n_dst, X.shape[1]
    ld = F if ld_y is None else ld_y
    buf = torch.full((n_dst, ld), float("nan"), device=X.device)
    nbytes = _lib.lib.dgmi_spmm_sliced_planes_bytes(n_dst, 8, F)
    planes = torch.empty(max(nbytes // 4, 4), dtype=torch.float32, device=X.device)
    epi = (1, C.SLOPE, epi_mask.data_ptr(), epi_mask.stride(0), C.MASK_SCALE) if epi_mask is not None else (0, 0.0, None, 0, 1.0)
    _lib.check(_lib.lib.dgmi_spmm_sliced_f32(
        sl.segptr.data_ptr(), ids.data_ptr(), None, None, None, 0, X.data_ptr(), X.stride(0), None,
        None if ds is None else ds.data_ptr(), buf.data_ptr(), ld, n_dst, sl.n_src, F, 8, 0, int(id_mult), planes.data_ptr(),
        nbytes, *epi, torch.cuda.current_stream().cuda_stream), "dgmi_spmm_sliced_f32")
    if ld > F:
        assert bool(torch.isnan(buf[:, F:]).all()), "the product wrote outside its F columns"
    return buf[:, :F]


def _settings(n_dst):
    """Knob settings of the forced form: each knob alone, then lane-group width x R x row rounds on 3 workgroups and
    grid x row rounds.  An LDS cap of ceil(B / k) rows gives k row rounds of a workgroup's B = ceil(n_dst / grid) rows."""
    def cap(grid, rounds):
        B = -(-n_dst // grid)
        return 0 if rounds == 1 else -(-B // rounds)

    out = [dict()]
    out += [dict(sliced_lpr=w) for w in (8, 16, 32, 64)]
    out += [dict(sliced_owned_grid=g) for g in (1, 3, 8, 19)]
    out += [dict(sliced_owned_rows=r) for r in (1, 2, 5)]
    out += [dict(sliced_owned_grid=8, sliced_owned_lds_rows=cap(8, k)) for k in (2, 4)]
    out += [dict(sliced_no_off32=1), dict(sliced_no_off32=1, sliced_owned_grid=3, sliced_owned_rows=2)]
    out += [dict(sliced_lpr=w, sliced_owned_rows=r, sliced_owned_grid=3, sliced_owned_lds_rows=cap(3, k))
            for w, r, k in itertools.product((8, 16, 32, 64), (1, 2, 5), (1, 2, 4))]
    out += [dict(sliced_owned_grid=g, sliced_owned_lds_rows=cap(g, k), sliced_owned_rows=r)
            for g, k, r in itertools.product((1, 3, 8, 19), (1, 2, 4), (1, 5))]
    return out


def test_forced_form_launches_the_owned_kernel(dev):
    """The knob really selects the LDS kernel: a profiled call with ``sliced_owned = 1`` shows ``spmm_owned_kernel`` and
    no plane reduce, one with ``sliced_owned = 0`` the pair."""
    st = _stage(dev)
    X = _t(C.features(st["d"].n_src, 128, 5), dev)
    names = {}
    for flag in (1, 0):
        _set(sliced_owned=flag)
        with torch.profiler.profile(activities=[torch.profiler.ProfilerActivity.CUDA]) as prof:
            _product(st["sl"], st["sl"].indices, False, X)
            torch.cuda.synchronize()
        names[flag] = " ".join(e.key for e in prof.key_averages())
    assert "spmm_owned_kernel" in names[1] and "reduce_planes_kernel" not in names[1], names[1]
    assert "spmm_owned_kernel" not in names[0] and "reduce_planes_kernel" in names[0], names[0]


@pytest.mark.parametrize("F", [4, 128, 344])
@pytest.mark.parametrize("kind", ["unit", "mult"])
def test_owned_exact_on_designed_operands(dev, kind, F):
    """(a) every lane-group width, grids 1 / 3 / 8 / 19, R 1 / 2 / 5, 1 / 2 / 4 row rounds, 64-bit row addresses; unit
    values and id multiplicities; ``dst_scale`` on and off, the activation + mask epilogue, a strided ``Y``."""
    st = _stage(dev)
    d, sl = st["d"], st["sl"]
    seed = 11 * F + 3
    X = C.features(d.n_src, F, seed)
    mask = C.out_mask(d.n_dst, F, seed + 1)
    w = d.mult if kind == "mult" else None
    ids = st["ids"] if kind == "mult" else sl.indices
    combos = list(itertools.product((False, True), (False, True)))
    want = {(has_ds, epi): _t(C.reference(d.dst, d.src, d.n_dst, X, w, None, d.ds if has_ds else None, None,
                                          mask if epi else None, epi), dev) for has_ds, epi in combos}
    Xd, mask_d = _t(X, dev), _t(mask, dev)
    for i, knobs in enumerate(_settings(d.n_dst)):
        _set(sliced_owned=1, **knobs)
        for has_ds, epi in combos:
            y = _product(sl, ids, kind == "mult", Xd, st["ds"] if has_ds else None, mask_d if epi else None,
                         ld_y=F + 8 if i % 2 else None)
            assert torch.equal(y, want[has_ds, epi]), "%s dst_scale=%s epilogue=%s: %d elements differ, first row %d" % (
                knobs, has_ds, epi, int((y != want[has_ds, epi]).sum()), int((y != want[has_ds, epi]).any(1).nonzero()[0]))


def _knn_like(dev):
    """2 500 nodes, 64 neighbours each with repeats, multiplicities 1 .. 8 in the id words."""
    from dream_gnn_amd import ops

    rng = np.random.default_rng(64)
    n, k = 2500, 64
    dst = np.repeat(np.arange(n, dtype=np.int32), k)
    src = rng.integers(0, n, n * k).astype(np.int32)
    sl = ops.SlicedCSR(_t(dst, dev), _t(src, dev), n, n, n_slices=8)
    mult = _t(rng.integers(0, 8, n * k).astype(np.int32), dev)
    return sl, (sl.indices | (mult[sl.eid.long()] << ops.MULT_SHIFT)).contiguous()


@pytest.mark.parametrize("graph", ["designed", "knn"])
def test_owned_is_bitwise_the_pair_on_randn(dev, graph):
    """(b) the same call with ``sliced_owned`` 0 and 1 on ``randn`` operands: identical bits, with and without
    multiplicities, ``dst_scale`` and the epilogue, at two widths — and (c) whatever the gate does: lag -1 / 0 / 1 and a
    spin bound of one tick."""
    if graph == "designed":
        st = _stage(dev)
        sl, ids = st["sl"], st["ids"]
    else:
        sl, ids = _knn_like(dev)
    gen = torch.Generator(device="cpu").manual_seed(9)
    for F in (128, 344):
        X = torch.randn(sl.n_src, F, generator=gen).to(dev)
        ds = (torch.rand(sl.n_dst, generator=gen) + 0.5).to(dev)
        mask = _t(C.out_mask(sl.n_dst, F, 2), dev)
        for id_mult, has_ds, epi in itertools.product((False, True), (False, True), (False, True)):
            args = (sl, ids if id_mult else sl.indices, id_mult, X, ds if has_ds else None, mask if epi else None)
            _set(sliced_owned=0)
            pair = _product(*args)
            for knobs in (dict(), dict(sliced_owned_grid=19, sliced_owned_rows=2), dict(sliced_owned_lag=-1), dict(sliced_owned_lag=0),
                          dict(sliced_owned_lag=1, sliced_owned_spin_ticks=1), dict(sliced_owned_lag=0, sliced_owned_spin_ticks=1),
                          dict(sliced_owned_grid=8, sliced_owned_lds_rows=40, sliced_owned_lag=1)):
                _set(sliced_owned=1, **knobs)
                assert torch.equal(_product(*args), pair), (F, id_mult, has_ds, epi, knobs)


def test_forms_the_owned_kernel_does_not_take_fall_back_to_the_pair(dev):
    """(d) a value stream, ``src_scale``, dropout on the fly, a bf16 table, 3 slices and forced chunking with
    ``sliced_owned = 1``: the pair's result."""
    from dream_gnn_amd import ops

    st = _stage(dev)
    d, sl = st["d"], st["sl"]
    gen = torch.Generator(device="cpu").manual_seed(4)
    X = torch.randn(d.n_src, 128, generator=gen).to(dev)
    vals = torch.randn(d.dst.size, generator=gen).to(dev)
    ss = (torch.rand(d.n_src, generator=gen) + 0.5).to(dev)
    desc = ops.random_subset_select(d.dst.size, int(d.dst.size * C.DROP_KEEP), C.DROP_SEED, dev)
    sl3 = ops.SlicedCSR(_t(d.dst, dev), _t(d.src, dev), d.n_dst, d.n_src, n_slices=3)
    forms = {"value stream": lambda: sl.spmm(X, vals=vals), "src_scale": lambda: sl.spmm(X, ss),
             "dropout on the fly": lambda: sl.spmm(X, keep=desc), "bf16 table": lambda: sl.spmm(X, gather_dtype=torch.bfloat16),
             "3 slices": lambda: sl3.spmm(X), "forced chunking": lambda: sl.spmm(X)}
    for what, run in forms.items():
        chunk = 37 if what == "forced chunking" else 0
        _set(sliced_owned=0, sliced_chunk_rows=chunk)
        pair = run()
        _set(sliced_owned=1, sliced_chunk_rows=chunk)
        assert torch.equal(run(), pair), what
