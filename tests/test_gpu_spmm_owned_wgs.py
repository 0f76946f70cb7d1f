"""The workgroup-owned form of the XCD-local SpMM with TWO co-resident 12-wave workgroups per CU
(``sliced_owned = 1, sliced_owned_wgs = 2``; csrc/dgmi_owned.hip), through the C ABI as test_gpu_spmm_owned.py does:
(a) ``torch.equal`` against the integer reference on the designed operands of _spmm_cases.py, (b) identical bits to the
sliced pair and to the one-workgroup form on ``randn``, whatever the gate does, (c) the knob really selects the kernel
instantiation, (d) a gate-free launch issues no fill kernel for the arrive counters."""
import itertools
import re

import numpy as np
import pytest
import torch

import _spmm_cases as C

pytestmark = pytest.mark.gpu

OWNED_DEFAULTS = dict(sliced_owned=-1, sliced_owned_wgs=0, sliced_owned_grid=0, sliced_owned_rows=0, sliced_owned_lds_rows=0,
                      sliced_owned_lag=-2, sliced_owned_spin_ticks=0, sliced_lpr=0, sliced_no_off32=0, sliced_chunk_rows=0)


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


def _buffers(sl, F, dev, ld_y=None):
    """(Y buffer of leading dimension ``ld_y`` filled with NaN, plane workspace, its bytes)."""
    from dream_gnn_amd import _lib

    nbytes = _lib.lib.dgmi_spmm_sliced_planes_bytes(sl.n_dst, 8, F)
    return (torch.full((sl.n_dst, F if ld_y is None else ld_y), float("nan"), device=dev),
            torch.empty(max(nbytes // 4, 4), dtype=torch.float32, device=dev), nbytes)


def _call(sl, ids, id_mult, X, ds, epi_mask, buf, planes, nbytes):
    """``dgmi_spmm_sliced_f32`` alone: nothing else is put on the stream."""
    from dream_gnn_amd import _lib

    epi = (1, C.SLOPE, epi_mask.data_ptr(), epi_mask.stride(0), C.MASK_SCALE) if epi_mask is not None else (0, 0.0, None, 0, 1.0)
    _lib.check(_lib.lib.dgmi_spmm_sliced_f32(
        sl.segptr.data_ptr(), ids.data_ptr(), None, None, None, 0, X.data_ptr(), X.stride(0), None,
        None if ds is None else ds.data_ptr(), buf.data_ptr(), buf.stride(0), sl.n_dst, sl.n_src, X.shape[1], 8, 0, int(id_mult),
        planes.data_ptr(), nbytes, *epi, torch.cuda.current_stream().cuda_stream), "dgmi_spmm_sliced_f32")


def _product(sl, ids, id_mult, X, ds=None, epi_mask=None, ld_y=None):
    """The product into a view of a NaN-filled buffer of leading dimension ``ld_y``, whose other columns must stay NaN."""
    F = X.shape[1]
    buf, planes, nbytes = _buffers(sl, F, X.device, ld_y)
    _call(sl, ids, id_mult, X, ds, epi_mask, buf, planes, nbytes)
    if buf.shape[1] > F:
        assert bool(torch.isnan(buf[:, F:]).all()), "the product wrote outside its F columns"
    return buf[:, :F]


def _settings(n_dst):
    """Knob settings of the two-workgroup form: each knob alone, 64-bit row addresses, then lane-group width x R x row
    rounds x grid.  An LDS cap of ceil(B / k) rows gives k row rounds of a workgroup's B = ceil(n_dst / grid) rows; an odd
    grid leaves one workgroup alone on a CU."""
    def cap(grid, rounds):
        B = -(-n_dst // grid)
        return 0 if rounds == 1 else -(-B // rounds)

    out = [dict()]
    out += [dict(sliced_lpr=w) for w in (8, 16, 32, 64)]
    out += [dict(sliced_owned_grid=g) for g in (2, 3, 8, 19)]
    out += [dict(sliced_owned_rows=r) for r in (1, 2, 5)]
    out += [dict(sliced_no_off32=1), dict(sliced_no_off32=1, sliced_owned_grid=3, sliced_owned_rows=2)]
    out += [dict(sliced_lpr=w, sliced_owned_rows=r, sliced_owned_grid=g, sliced_owned_lds_rows=cap(g, k))
            for w, r, k, g in itertools.product((8, 16, 32, 64), (1, 2, 5), (1, 2, 4), (2, 3, 8, 19))]
    return out


@pytest.mark.parametrize("F", [4, 128, 344])
@pytest.mark.parametrize("kind", ["unit", "mult"])
def test_two_workgroups_exact_on_designed_operands(dev, kind, F):
    """(a) every lane-group width x R 1 / 2 / 5 x 1 / 2 / 4 row rounds at grids 2 / 3 / 8 / 19, 64-bit row addresses; unit
    values and id multiplicities; ``dst_scale`` on and off, the activation + mask epilogue, a strided ``Y`` whose guard
    columns stay NaN."""
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
    for i, knobs in enumerate(_settings(d.n_dst)):
        _set(sliced_owned=1, sliced_owned_wgs=2, **knobs)
        for has_ds, epi in combos:
            y = _product(sl, ids, kind == "mult", Xd, st["ds"] if has_ds else None, mask_d if epi else None,
                         ld_y=F + 8 if i % 2 else None)
            assert torch.equal(y, want[has_ds, epi]), "%s dst_scale=%s epilogue=%s: %d elements differ, first row %d" % (
                knobs, has_ds, epi, int((y != want[has_ds, epi]).sum()), int((y != want[has_ds, epi]).any(1).nonzero()[0]))


def _knn_like(dev):
    """2 500 nodes, 64 neighbours each with repeats, multiplicities 1 .. 8 in the id words."""
    from dream_gnn_amd import ops

    rng = np.random.default_rng(65)
    n, k = 2500, 64
    dst = np.repeat(np.arange(n, dtype=np.int32), k)
    src = rng.integers(0, n, n * k).astype(np.int32)
    sl = ops.SlicedCSR(_t(dst, dev), _t(src, dev), n, n, n_slices=8)
    mult = _t(rng.integers(0, 8, n * k).astype(np.int32), dev)
    return sl, (sl.indices | (mult[sl.eid.long()] << ops.MULT_SHIFT)).contiguous()


@pytest.mark.parametrize("graph", ["designed", "knn"])
def test_two_workgroups_are_bitwise_the_pair_and_the_one_workgroup_form_on_randn(dev, graph):
    """(b) the same call with the pair (``sliced_owned = 0``), with ``sliced_owned_wgs = 1`` and with ``= 2`` on ``randn``
    operands: identical bits, with and without multiplicities, ``dst_scale`` and the epilogue, at two widths, with lag
    -1 / 0 / 1 and a spin bound of one tick."""
    if graph == "designed":
        st = _stage(dev)
        sl, ids = st["sl"], st["ids"]
    else:
        sl, ids = _knn_like(dev)
    gen = torch.Generator(device="cpu").manual_seed(10)
    for F in (128, 344):
        X = torch.randn(sl.n_src, F, generator=gen).to(dev)
        ds = (torch.rand(sl.n_dst, generator=gen) + 0.5).to(dev)
        mask = _t(C.out_mask(sl.n_dst, F, 3), dev)
        for id_mult, has_ds, epi in itertools.product((False, True), (False, True), (False, True)):
            args = (sl, ids if id_mult else sl.indices, id_mult, X, ds if has_ds else None, mask if epi else None)
            _set(sliced_owned=0)
            pair = _product(*args)
            for knobs in (dict(), dict(sliced_owned_grid=19, sliced_owned_rows=2), dict(sliced_owned_lag=-1), dict(sliced_owned_lag=0),
                          dict(sliced_owned_lag=1), dict(sliced_owned_lag=1, sliced_owned_spin_ticks=1),
                          dict(sliced_owned_lag=0, sliced_owned_spin_ticks=1),
                          dict(sliced_owned_grid=8, sliced_owned_lds_rows=40, sliced_owned_lag=1)):
                for wgs in (1, 2):
                    _set(sliced_owned=1, sliced_owned_wgs=wgs, **knobs)
                    assert torch.equal(_product(*args), pair), (F, id_mult, has_ds, epi, wgs, knobs)


def _kernels_of_one_call(st, dev, ids, id_mult, **knobs):
    """(names of what ran on the device, names of everything the profiler recorded: runtime calls too) during ONE product
    call; the buffers are made beforehand."""
    X = _t(C.features(st["d"].n_src, 128, 6), dev)
    buf, planes, nbytes = _buffers(st["sl"], 128, dev)
    _set(**knobs)
    torch.cuda.synchronize()
    with torch.profiler.profile(activities=[torch.profiler.ProfilerActivity.CUDA]) as prof:
        _call(st["sl"], ids, id_mult, X, None, None, buf, planes, nbytes)
        torch.cuda.synchronize()
    events = prof.key_averages()
    return [e.key for e in events if e.device_type == torch.autograd.DeviceType.CUDA], [e.key for e in events]


def _owned_waves(names):
    """The WAVES argument (the last one) of every ``spmm_owned_kernel`` instantiation among ``names``."""
    return [int(re.search(r"spmm_owned_kernel<([^>]*)>", n).group(1).split(",")[-1]) for n in names[0] if "spmm_owned_kernel<" in n]


def test_the_knob_selects_the_instantiation(dev):
    """(c) ``sliced_owned_wgs = 2`` launches the 12-wave instantiation and ``= 1`` the 16-wave one; the 8-lane groups with
    multiplicities exist in the 16-wave form only and take it under either setting."""
    st = _stage(dev)
    unit = (st["sl"].indices, False)
    assert _owned_waves(_kernels_of_one_call(st, dev, *unit, sliced_owned=1, sliced_owned_wgs=2)) == [12]
    assert _owned_waves(_kernels_of_one_call(st, dev, *unit, sliced_owned=1, sliced_owned_wgs=1)) == [16]
    assert _owned_waves(_kernels_of_one_call(st, dev, *unit, sliced_owned=1, sliced_owned_wgs=2, sliced_owned_grid=3)) == [12]
    assert _owned_waves(_kernels_of_one_call(st, dev, st["ids"], True, sliced_owned=1, sliced_owned_wgs=2, sliced_lpr=16)) == [12]
    assert _owned_waves(_kernels_of_one_call(st, dev, st["ids"], True, sliced_owned=1, sliced_owned_wgs=2, sliced_lpr=8)) == [16]
    assert _owned_waves(_kernels_of_one_call(st, dev, *unit, sliced_owned=0)) == []


@pytest.mark.parametrize("wgs", [1, 2])
def test_a_gate_free_launch_is_one_kernel(dev, wgs):
    """(d) with lag -1 the product call is the owned kernel and nothing else: no fill kernel (or memset) of the arrive
    counters.  With a gate (lag 0) the same call does show one — the trace can see it."""
    st = _stage(dev)
    fill = re.compile(r"(?i)fill|memset")
    for lag in (dict(sliced_owned_lag=-1), dict()):  # asked for, and the built-in choice
        on_device, recorded = _kernels_of_one_call(st, dev, st["sl"].indices, False, sliced_owned=1, sliced_owned_wgs=wgs, **lag)
        assert len(on_device) == 1 and "spmm_owned_kernel" in on_device[0], on_device
        assert not any(fill.search(n) for n in recorded), recorded
    on_device, recorded = _kernels_of_one_call(st, dev, st["sl"].indices, False, sliced_owned=1, sliced_owned_wgs=wgs, sliced_owned_lag=0)
    assert any(fill.search(n) for n in recorded), recorded
    assert sum("spmm_owned_kernel" in n for n in on_device) == 1, on_device
