"""The hand-over of the gather window from task to task in the workgroup-owned SpMM (csrc/dgmi_owned_kernel.h) on the designed
graph of _owned_window_cases.py, whose consecutive pairs of runs _owned_carry_cases.py restates
(test_owned_carry_host.py shows which kinds of pair occur under the settings used here).

The form is forced with ``sliced_owned = 1`` through the C ABI, as in test_gpu_spmm_owned.py.  ``sliced_owned_workers``
makes the order reproducible: with 1 a single wave runs every task of a workgroup in order, so every consecutive pair
of tasks hands over; with 2 the pairs interleave; 0 is the launch as shipped.  Crossed with 1 and 2 workgroups, every
lane-group width, 1 / 2 / 5 rows per lane group, 1 and 2 row rounds, both address widths, unit values and multiplicities
1 .. 8, F = 4 / 128 / 344 (11 column rounds at 8-lane groups) and a strided ``Y`` inside a NaN-filled buffer.  Integer
operands at ZERO tolerance (``torch.equal``) against the int64 numpy reference, which asserts exactness; on ``randn``
bit for bit the pair, with ``dst_scale`` and the epilogue on and off.

Which value-only mutations of the hand-over fail which of these cases: profiles/owned_carry/README.md."""
import numpy as np
import pytest
import torch

import _owned_carry_cases as C
import _owned_window_cases as D
from test_gpu_spmm_owned import OWNED_DEFAULTS, _product, _t

pytestmark = pytest.mark.gpu

DEFAULTS = dict(OWNED_DEFAULTS, sliced_owned_wgs=0, sliced_owned_workers=0)


@pytest.fixture(autouse=True)
def _knobs_back_to_default():
    from dream_gnn_amd import _lib

    try:
        yield
    finally:
        for name, value in DEFAULTS.items():
            _lib.set_tuning(name, value)


def _set(**knobs):
    from dream_gnn_amd import _lib

    for name, value in dict(DEFAULTS, **knobs).items():
        _lib.set_tuning(name, value)


_staged = {}


def _stage(dev):
    from dream_gnn_amd import ops

    if "d" not in _staged:
        d = D.design()
        sl = ops.SlicedCSR(_t(d.dst, dev), _t(d.src, dev), d.n_dst, d.n_src, n_slices=D.N_SLICES)
        assert np.array_equal(sl.segptr.cpu().numpy(), d.segptr) and np.array_equal(sl.indices.cpu().numpy(), d.indices)
        ids = (sl.indices | ((_t(d.mult, dev) - 1)[sl.eid.long()] << ops.MULT_SHIFT)).contiguous()
        _staged.update(d=d, sl=sl, ids=ids)
    return _staged


def test_the_settings_launch_the_owned_kernel(dev):
    """Settings of the sweep, the single worker among them, really run the LDS kernel (the knob would otherwise fall
    back to the pair silently)."""
    st = _stage(dev)
    X = torch.ones(st["d"].n_src, 128, device=dev)
    for knobs in (C.settings()[0], C.settings()[-1]):
        _set(sliced_owned=1, **knobs)
        with torch.profiler.profile(activities=[torch.profiler.ProfilerActivity.CUDA]) as prof:
            _product(st["sl"], st["sl"].indices, False, X)
            torch.cuda.synchronize()
        names = " ".join(e.key for e in prof.key_averages())
        assert "spmm_owned_kernel" in names and "reduce_planes_kernel" not in names, names


@pytest.mark.parametrize("F", C.FS)
@pytest.mark.parametrize("kind", ["unit", "mult"])
def test_hand_over_exact_on_the_designed_graph(dev, kind, F):
    st = _stage(dev)
    d, sl = st["d"], st["sl"]
    X = np.random.default_rng(11 * F + 3).integers(-8, 9, (d.n_src, F)).astype(np.float32)
    want = _t(D.reference(d, X, d.mult if kind == "mult" else None), dev)
    ids = st["ids"] if kind == "mult" else sl.indices
    Xd = _t(X, dev)
    for i, knobs in enumerate(C.settings()):
        _set(sliced_owned=1, **knobs)
        y = _product(sl, ids, kind == "mult", Xd, ld_y=F + 8 if i % 3 == 0 else None)  # (_product checks the NaN frame)
        assert torch.equal(y, want), "%s: %d elements differ, first row %d" % (
            knobs, int((y != want).sum()), int((y != want).any(1).nonzero()[0]))


@pytest.mark.parametrize("F", [128, 344])
def test_hand_over_is_bitwise_the_pair_on_randn(dev, F):
    """Against the pair, with and without multiplicities, ``dst_scale`` and the epilogue; both address widths."""
    st = _stage(dev)
    sl = st["sl"]
    gen = torch.Generator(device="cpu").manual_seed(17 + F)
    X = torch.randn(sl.n_src, F, generator=gen).to(dev)
    ds = (torch.rand(sl.n_dst, generator=gen) + 0.5).to(dev)
    mask = _t((np.random.default_rng(5).random((sl.n_dst, F)) < 0.6).astype(np.float32), dev)
    for id_mult in (False, True):
        for has_ds, epi in ((False, False), (True, True), (True, False)):
            args = (sl, st["ids"] if id_mult else sl.indices, id_mult, X, ds if has_ds else None, mask if epi else None)
            _set(sliced_owned=0)
            pair = _product(*args)
            for knobs in C.settings()[::5]:  # (a stride coprime to the six inner combinations: every worker count x address width)
                _set(sliced_owned=1, **knobs)
                assert torch.equal(_product(*args), pair), (F, id_mult, has_ds, epi, knobs)


def test_the_number_of_workers_changes_no_bit(dev):
    """Two calls that differ in ``sliced_owned_workers`` alone: which tasks a wave runs back to back — which windows
    are handed over and which start cold — must not show in the result."""
    st = _stage(dev)
    sl = st["sl"]
    gen = torch.Generator(device="cpu").manual_seed(29)
    X = torch.randn(sl.n_src, 128, generator=gen).to(dev)
    ds = (torch.rand(sl.n_dst, generator=gen) + 0.5).to(dev)
    for id_mult in (False, True):
        ids = st["ids"] if id_mult else sl.indices
        for lpr in C.WIDTHS:
            for R in C.ROWS:
                base = dict(sliced_owned=1, sliced_lpr=lpr, sliced_owned_rows=R, sliced_owned_grid=2)
                outs = []
                for n in (0, 1, 2, 7):
                    _set(sliced_owned_workers=n, **base)
                    outs.append(_product(sl, ids, id_mult, X, ds).clone())
                for y in outs[1:]:
                    assert torch.equal(y, outs[0]), (id_mult, lpr, R)


@pytest.mark.parametrize("grid", C.GRIDS)
@pytest.mark.parametrize("lpr", C.WIDTHS)
def test_hand_over_exact_on_the_graph_made_for_the_setting(dev, lpr, grid):
    """``made_design``: under its own setting every run hands over in every kind the geometry allows
    (test_owned_carry_host.py), the step into the next column round with the next task's column offset among them.
    Zero tolerance, unit values and multiplicities, F = 4 / 128 / 344, 1 / 2 / all workers, both address widths."""
    from dream_gnn_amd import ops

    for R in C.ROWS:
        for rounds in C.ROUNDS:
            d = C.made_design(lpr, R, rounds, grid)
            sl = ops.SlicedCSR(_t(d.dst, dev), _t(d.src, dev), d.n_dst, d.n_src, n_slices=D.N_SLICES)
            assert np.array_equal(sl.segptr.cpu().numpy(), d.segptr) and np.array_equal(sl.indices.cpu().numpy(), d.indices)
            ids = (sl.indices | ((_t(d.mult, dev) - 1)[sl.eid.long()] << ops.MULT_SHIFT)).contiguous()
            for F in C.FS:
                X = np.random.default_rng(13 * F + R).integers(-8, 9, (d.n_src, F)).astype(np.float32)
                Xd = _t(X, dev)
                for kind in ("unit", "mult"):
                    want = _t(D.reference(d, X, d.mult if kind == "mult" else None), dev)
                    for i, (workers, o) in enumerate((n, o) for n in C.WORKERS for o in (0, 1)):
                        _set(sliced_owned=1, sliced_lpr=lpr, sliced_owned_rows=R, sliced_owned_grid=grid,
                             sliced_owned_lds_rows=C.lds_cap(rounds, grid), sliced_owned_workers=workers, sliced_no_off32=o)
                        y = _product(sl, ids if kind == "mult" else sl.indices, kind == "mult", Xd, ld_y=F + 8 if i % 2 else None)
                        assert torch.equal(y, want), (R, rounds, F, kind, workers, o, int((y != want).sum()))
