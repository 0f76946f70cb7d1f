"""The two directions of ``ops.CSRGraph`` are one path: the transposed product of a graph is, bit for bit and kernel
for kernel, the forward product of its mirror.  For ``G = CSRGraph(dst, src, n_dst, n_src, vals)`` and
``Gt = CSRGraph(src, dst, n_src, n_dst, vals)``, carrying the same views (``with_values``, ``dropped``, ``dropped``
twice, ``masked``):

    G.spmm_t(W, ss, ds) == Gt.spmm(W, ds, ss)        G.spmm(X, ss, ds) == Gt.spmm_t(X, ds, ss)

with ``torch.equal`` on ``randn`` operands (the summation order matters), and the device kernels the two calls launch
have the same names in the same order (``torch.profiler``).  Every route is forced on the small designed graphs of the
exact files: wave per row, planned, plain XCD-local (float32 and bf16 gather, dropped edges compacted or evaluated on the
fly), ``scale x multiplicity`` values (``G`` finds the ``"row"`` form, ``Gt`` the ``"col"`` form) and the split form.
What is correct is settled by the exact files against the reference; this file only says that forward and backward do
not drift apart."""
import os

import numpy as np
import pytest
import torch

import _binding_cases as B
import _spmm_cases as C

pytestmark = [pytest.mark.gpu,
              pytest.mark.skipif(bool(os.environ.get("DGMI_FORCE_KERNEL")), reason="kernel choice is forced")]


def _t(a, dev):
    return None if a is None else torch.from_numpy(np.array(a)).to(dev)


def _views(ops, G, E, dev, other_vals):
    """The views both graphs are given, from draws that depend on the edge count alone."""
    desc = ops.random_subset_select(E, int(E * C.DROP_KEEP), C.DROP_SEED, dev)
    desc2 = ops.random_subset_select(E, E // 2, 5, dev)
    keep = (torch.rand(E, generator=torch.Generator().manual_seed(11)) < 0.8).float().to(dev)
    return [("base", G), ("with_values", G.with_values(other_vals)), ("dropped", G.dropped(desc)),
            ("dropped twice", G.dropped(desc).dropped(desc2)), ("masked", G.masked(keep))]


def _kernel_names(calls):
    """Run ``calls`` under the profiler: the device kernel names in launch order."""
    with torch.profiler.profile(activities=[torch.profiler.ProfilerActivity.CUDA]) as prof:
        for call in calls:
            call()
        torch.cuda.synchronize()
    events = [e for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA]
    return [e.name for e in sorted(events, key=lambda e: e.time_range.start)]


def _check_mirror(ops, dev, dst, src, n_dst, n_src, vals, F, gather_dtype=None, route=None, **graph_kw):
    """Build ``G``, its mirror and their views; compare both products of every view bitwise, then (everything built, so
    that only the products themselves launch) their kernel names.  ``route(G, Gt)`` asserts the route that was taken."""
    E = int(dst.shape[0])
    rng = torch.Generator().manual_seed(3)
    X, W = torch.randn(n_src, F, generator=rng).to(dev), torch.randn(n_dst, F, generator=rng).to(dev)
    ss, ds = (torch.rand(n_src, generator=rng) + 0.5).to(dev), (torch.rand(n_dst, generator=rng) + 0.5).to(dev)
    other = (torch.rand(E, generator=rng) + 0.5).to(dev)
    G = ops.CSRGraph(_t(dst, dev), _t(src, dev), n_dst, n_src, vals=_t(vals, dev), **graph_kw)
    Gt = ops.CSRGraph(_t(src, dev), _t(dst, dev), n_src, n_dst, vals=_t(vals, dev), **graph_kw)
    kw = dict(gather_dtype=gather_dtype)
    own, mirror = [], []
    for (what, v), (_, vt) in zip(_views(ops, G, E, dev, other), _views(ops, Gt, E, dev, other)):
        for s, d in ((None, None), (ss, ds)):
            assert torch.equal(v.spmm_t(W, s, d, **kw), vt.spmm(W, d, s, **kw)), (what, "spmm_t", s is not None)
            assert torch.equal(v.spmm(X, s, d, **kw), vt.spmm_t(X, d, s, **kw)), (what, "spmm", s is not None)
            own += [lambda v=v, s=s, d=d: v.spmm_t(W, s, d, **kw), lambda v=v, s=s, d=d: v.spmm(X, s, d, **kw)]
            mirror += [lambda vt=vt, s=s, d=d: vt.spmm(W, d, s, **kw), lambda vt=vt, s=s, d=d: vt.spmm_t(X, d, s, **kw)]
    if route is not None:
        route(G, Gt)
    names, names_t = _kernel_names(own), _kernel_names(mirror)
    assert len(names) >= len(own) and names == names_t, (names, names_t)
    return G, Gt


def _plain(G, Gt):
    for g in (G, Gt):
        S = g._S
        assert S.sliced is None and S.sliced_t is None and S.split is None and S.split_t is None


def _xcd_local(G, Gt):
    for g in (G, Gt):
        S = g._S
        assert S.sliced is not None and S.sliced_t is not None and S.split is None and S.split_t is None


def _split(G, Gt):
    for g in (G, Gt):
        S = g._S
        assert S.sliced is None and S.sliced_t is None and S.split is not None and S.split_t is not None


@pytest.mark.parametrize("planned", [False, True], ids=["wave-per-row", "planned"])
@pytest.mark.parametrize("weighted", [False, True], ids=["unit", "vals"])
def test_plain_csr_routes(dev, planned, weighted):
    """The 331-row design with its 3 000-edge row (longer than the plan's chunk): without a plan a wave per row, with it
    the planned kernel in the direction that holds the long row."""
    from dream_gnn_amd import ops

    g = B.graph()
    G, Gt = _check_mirror(ops, dev, g.dst, g.src, g.n_dst, g.n_src, g.vals if weighted else None, 64, route=_plain,
                          planned=planned)
    assert (G.plan is not None) == planned and (not planned or G._S.max_deg == 3000 > G.plan.chunk)


@pytest.mark.parametrize("compact", [True, False], ids=["compacted", "on-the-fly"])
@pytest.mark.parametrize("gather", [None, torch.bfloat16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("weighted", [False, True], ids=["unit", "vals"])
def test_plain_xcd_local_route(dev, monkeypatch, weighted, gather, compact):
    from dream_gnn_amd import ops

    monkeypatch.setattr(ops, "FORCE_KERNEL", "sliced")
    monkeypatch.setattr(ops, "COMPACT_DROPPED", compact)
    d = C.sliced_design(8)
    _check_mirror(ops, dev, d.dst, d.src, d.n_dst, d.n_src, d.vals if weighted else None, 128, gather, route=_xcd_local)


def _normalized_adjacency(n, k, seed):
    """``D^-1 (A + A^T + I)`` of a random ``k``-neighbour list as COO triplets (duplicates merged: multiplicities 1 .. 3)."""
    rng = np.random.default_rng(seed)
    r = np.repeat(np.arange(n), k)
    c = rng.integers(0, n, r.size)
    M = np.zeros((n, n), np.float64)
    np.add.at(M, (r, c), 1.0)
    M = np.minimum(M, 1.0)
    M = M + M.T + np.eye(n)
    rows, cols = np.nonzero(M)
    vals = (M[rows, cols] / M.sum(1)[rows]).astype(np.float32)
    order = rng.permutation(rows.size)
    return rows[order].astype(np.int32), cols[order].astype(np.int32), vals[order]


@pytest.mark.parametrize("compact", [True, False], ids=["compacted", "on-the-fly"])
@pytest.mark.parametrize("gather", [None, torch.bfloat16], ids=["fp32", "bf16"])
def test_scale_times_multiplicity_values(dev, monkeypatch, gather, compact):
    """The reference's normalised adjacency on 311 nodes: ``G`` carries the row scale on its destinations, its mirror on
    its sources, and both run without a value stream."""
    from dream_gnn_amd import ops

    monkeypatch.setattr(ops, "FORCE_KERNEL", "sliced")
    monkeypatch.setattr(ops, "COMPACT_DROPPED", compact)
    monkeypatch.setattr(ops, "MULT_FORM", True)
    n = 311
    rows, cols, vals = _normalized_adjacency(n, 6, 7)
    G, Gt = _check_mirror(ops, dev, rows, cols, n, n, vals, 128, gather, route=_xcd_local)
    assert G._mult_form()[0] == "row" and Gt._mult_form()[0] == "col"
    assert torch.equal(G._mult_form()[1], Gt._mult_form()[1]) and torch.equal(G._mult_form()[2], Gt._mult_form()[2])


@pytest.mark.parametrize("compact", [True, False], ids=["compacted", "on-the-fly"])
@pytest.mark.parametrize("kind", ["light", "heavy"])
def test_split_route(dev, monkeypatch, kind, compact):
    """The 300-row graphs with a 3 000-edge row and a 2 500-edge column under the 16 / 4 layout: both directions of both
    graphs take the split form."""
    from dream_gnn_amd import ops

    monkeypatch.setattr(ops, "SPLIT_MIN_TABLE_BYTES", 0)
    monkeypatch.setattr(ops, "SPLIT_ROW_EDGES", 16)
    monkeypatch.setattr(ops, "SPLIT_LIGHT_ROW_EDGES", 4)
    monkeypatch.setattr(ops, "COMPACT_DROPPED", compact)
    g = C.split_graph(kind)
    G, Gt = _check_mirror(ops, dev, g.dst, g.src, g.n_dst, g.n_src, g.vals, 128, route=_split)
    assert G._S.split.has_light == Gt._S.split_t.has_light and G._S.split_t.n_virtual == Gt._S.split.n_virtual
