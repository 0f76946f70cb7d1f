"""The rolling gather window of the workgroup-owned SpMM (csrc/dgmi_owned_kernel.h) on the graph designed for it
(_owned_window_cases.py: every segment length around the window and the lane-group widths, in every slice, as first,
middle and last row of a run; runs shorter than the window, exact multiples, runs ending in empty rows, empty tasks, a
last source id of ``n_src - 1``; test_owned_window_host.py checks that it covers all that under every setting used here).

The form is forced with ``sliced_owned = 1`` through the C ABI, as in test_gpu_spmm_owned.py.  Integer operands at ZERO
tolerance (``torch.equal``) against a numpy integer reference, and bit for bit against the sliced pair on ``randn``;
crossed with every lane-group width, 1 / 2 / 5 rows per lane group, 1 and 2 row rounds, 64-bit row addresses, unit values
and multiplicities 1 .. 8, F = 4 / 128 / 344, and a strided ``Y`` inside a NaN-filled buffer."""
import numpy as np
import pytest
import torch

import _owned_window_cases as D
from test_gpu_spmm_owned import OWNED_DEFAULTS, _product, _t

pytestmark = pytest.mark.gpu

DEFAULTS = dict(OWNED_DEFAULTS, sliced_owned_wgs=0)


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
    """A setting of the sweep really runs the LDS kernel (the knob would otherwise fall back to the pair silently)."""
    st = _stage(dev)
    X = torch.ones(st["d"].n_src, 128, device=dev)
    _set(sliced_owned=1, **D.settings()[0])
    with torch.profiler.profile(activities=[torch.profiler.ProfilerActivity.CUDA]) as prof:
        _product(st["sl"], st["sl"].indices, False, X)
        torch.cuda.synchronize()
    names = " ".join(e.key for e in prof.key_averages())
    assert "spmm_owned_kernel" in names and "reduce_planes_kernel" not in names, names


@pytest.mark.parametrize("F", [4, 128, 344])
@pytest.mark.parametrize("kind", ["unit", "mult"])
def test_window_exact_on_the_designed_graph(dev, kind, F):
    st = _stage(dev)
    d, sl = st["d"], st["sl"]
    X = np.random.default_rng(7 * F + 1).integers(-8, 9, (d.n_src, F)).astype(np.float32)
    want = _t(D.reference(d, X, d.mult if kind == "mult" else None), dev)
    ids = st["ids"] if kind == "mult" else sl.indices
    Xd = _t(X, dev)
    for i, knobs in enumerate(D.settings()):
        _set(sliced_owned=1, **knobs)
        y = _product(sl, ids, kind == "mult", Xd, ld_y=F + 8 if i % 2 == 0 else None)  # (_product checks the NaN frame)
        assert torch.equal(y, want), "%s: %d elements differ, first row %d" % (
            knobs, int((y != want).sum()), int((y != want).any(1).nonzero()[0]))


@pytest.mark.parametrize("wgs", [1, 2])
def test_window_is_bitwise_the_pair_on_randn(dev, wgs):
    """Both forms of the kernel (one 16-wave workgroup per CU, two 12-wave ones) against the pair, with and
    without multiplicities, ``dst_scale`` and the epilogue."""
    st = _stage(dev)
    sl = st["sl"]
    gen = torch.Generator(device="cpu").manual_seed(13)
    mask_rng = np.random.default_rng(3)
    for F in (128, 344):
        X = torch.randn(sl.n_src, F, generator=gen).to(dev)
        ds = (torch.rand(sl.n_dst, generator=gen) + 0.5).to(dev)
        mask = _t((mask_rng.random((sl.n_dst, F)) < 0.6).astype(np.float32), dev)
        for id_mult in (False, True):
            for has_ds, epi in ((False, False), (True, True)):
                args = (sl, st["ids"] if id_mult else sl.indices, id_mult, X, ds if has_ds else None, mask if epi else None)
                _set(sliced_owned=0)
                pair = _product(*args)
                for knobs in D.settings()[::2]:  # (the 32-bit offsets)
                    _set(sliced_owned=1, sliced_owned_wgs=wgs, **knobs)
                    assert torch.equal(_product(*args), pair), (F, id_mult, has_ds, epi, knobs)
