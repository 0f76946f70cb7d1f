"""Designed graphs, plain references and the checks of the row-shard layer (``dream_gnn_amd/shard.py``): which rows, which
values and which slice of ``dst_scale`` every rank's kernels see, and how the blocks come back together.  Plain module
(like ``_module_cases.py``), shared by test_shard_cases_host.py (CPU backend, gloo) and test_gpu_shard_exact.py.

Operands are those of ``_spmm_cases.py`` — ``X`` / ``dY`` integers in [-8, 8], edge values +-1 .. +-4 (the adjacency:
``2^-k * m`` with m in 1..3), ``src_scale`` in {0.5, 1, 2}, ``dst_scale`` in {0.25, 0.5, 1, 2} — so every sharded product
is an integer computation in units of its granularity: exact in fp32 under any kernel, any split into ranks and any
exchange, and every comparison is ``torch.equal``.  ``_spmm_cases.reference`` asserts the condition (``sum |terms| /
granularity < 2^23`` per row) for every product referenced here.

Nothing here calls ``torch.distributed`` except ``check_gather``: ``RowShard.__init__``, ``spmm_local`` and
``ShardedRelation(..., rank=r, world=W)`` need no process group, so one process builds every rank."""
from collections import namedtuple

import numpy as np
import torch

import _module_cases as MC
import _spmm_cases as C

ShardDesign = namedtuple("ShardDesign", "name dst src vals n_dst n_src gran")  # vals: float32 or None; gran: their granularity
Local = namedtuple("Local", "dst src vals")
WORLDS_HOST = (1, 2, 3, 5, 8, 16)
WORLDS_GPU = (1, 2, 3, 5, 8)
TOL = 0.01                      # choose_row_bounds' default
DROP_KEEP, DROP_SEED = 0.7, 77
NAN = float("nan")


def _finish(name, dst, src, n_dst, n_src, seed, vals="ints", gran=1.0):
    """Shuffle the COO order (so that ``vals[mine]`` is a real gather) and draw the integer edge values."""
    rng = np.random.default_rng(seed)
    order = rng.permutation(dst.size)
    dst, src = dst[order].astype(np.int64), src[order].astype(np.int64)
    if isinstance(vals, str):
        vals = (rng.integers(1, 5, dst.size) * rng.choice([-1, 1], dst.size)).astype(np.float32)
    else:
        vals = vals[order].astype(np.float32)
    for a in (dst, src, vals):
        a.setflags(write=False)
    return ShardDesign(name, dst, src, vals, int(n_dst), int(n_src), float(gran))


# ---------------------------------------------------------------------------------------------
# designs
# ---------------------------------------------------------------------------------------------
HUB_ROW, HUB_ROW_EDGES, HUB_COL, HUB_COL_EDGES = 5, 400, 2, 380


def hub():
    """41 destination rows x 23 sources (rectangular: a forward / backward mix-up changes shapes).  Row 5 holds 400
    edges, 380 of them from source 2 (duplicate (row, col) pairs; the transposed side's hub), rows 6 .. 19 hold 0 .. 3
    each, row 30 holds 7, rows 0 .. 4, 20 .. 29 and 31 .. 40 are empty."""
    rng = np.random.default_rng(41)
    n_dst, n_src = 41, 23
    deg = np.zeros(n_dst, np.int64)
    deg[HUB_ROW] = HUB_ROW_EDGES
    deg[6:20] = np.array([0, 3, 1, 2, 0, 3, 2, 1, 0, 2, 3, 1, 2, 3])
    deg[30] = 7
    dst = np.repeat(np.arange(n_dst), deg)
    src = rng.integers(0, n_src, dst.size)
    src[np.flatnonzero(dst == HUB_ROW)[:HUB_COL_EDGES]] = HUB_COL
    return _finish("hub", dst, src, n_dst, n_src, 42)


EVEN_N, EVEN_DEG, EVEN_ROW = 64, 32, 63


def even(extra=0):
    """64 x 64, every row and every column of degree 32 (64 % world == 0 for world 2, 4, 8).  ``extra``: that many more
    edges in the LAST row (2: still inside ``tol`` = 1 % at every world, and outside half of it at world 8; 24: outside
    at every world).  In the last row, so that the nnz-balanced cut differs from equal rows once the rule falls back to
    it: the targets move up past the row ends (one extra edge moves none of them: ``i * 2049 // 8 == 256 i``)."""
    n = EVEN_N
    dst = np.repeat(np.arange(n), EVEN_DEG)
    src = (dst * 7 + np.tile(np.arange(EVEN_DEG), n) * 5) % n
    dst = np.concatenate([dst, np.full(extra, EVEN_ROW)])
    src = np.concatenate([src, (np.arange(extra) * 11 + 3) % n])
    return _finish({0: "even", 2: "even_plus2", 24: "even_plus24"}[extra], dst, src, n, n, 43 + extra)


STAIRS_N, STAIRS_SRC = 20, 17


def stairs(kind="hit"):
    """Row r holds r + 1 edges (20 rows, 210 edges, 17 sources): the running sum is 1, 3, 6, ... and reaches 105 = 210 // 2
    exactly at the end of row 13 (``hit``: the cut of world 2 is 14, and ``right=True`` would say 15).  ``short``: one
    edge moved from row 13 to row 14 — the sum stands at 104 there, one edge short, and the cut is 15.  ``inside``: 19
    rows (190 edges): no target of world 2, 3, 5 or 8 is a running sum."""
    n = {"hit": 20, "short": 20, "inside": 19}[kind]
    deg = np.arange(1, n + 1)
    if kind == "short":
        deg[13] -= 1
        deg[14] += 1
    dst = np.repeat(np.arange(n), deg)
    src = (dst * 3 + np.arange(dst.size) * 5) % STAIRS_SRC
    return _finish("stairs_" + kind, dst, src, n, STAIRS_SRC, 50 + len(kind))


def adjacency(transposed=False):
    """The 96-node ``D^-1 (A + A^T + I)`` of ``_module_cases.adjacency_edges``: values ``scale[row] * m``, m in 1..3, every
    scale a power of two (1/4 .. 1/128).  ``transposed``: the same entries handed in as the graph ``make(c, r, n, n, v)``
    of bench.py's backward products — values ``scale[source] * m``."""
    _, _, M = MC.adjacency_edges(0)
    rows, cols = np.nonzero(M)
    rs = M.sum(1)
    vals = (M[rows, cols] / rs[rows]).astype(np.float32)
    assert np.array_equal(vals.astype(np.float64) * rs[rows], M[rows, cols])
    if transposed:
        rows, cols = cols, rows
    return _finish("adjacency_t" if transposed else "adjacency", rows, cols, MC.ADJ_N, MC.ADJ_N, 60, vals, 1.0 / rs.max())


def no_edges():
    z = np.zeros(0, np.int64)
    return _finish("no_edges", z, z, 9, 5, 70)


def one_row():
    return _finish("one_row", np.zeros(12, np.int64), np.arange(12) % 7, 1, 7, 71)


DESIGNS = {"hub": hub, "even": even, "even_plus2": lambda: even(2), "even_plus24": lambda: even(24),
           "stairs_hit": stairs, "stairs_short": lambda: stairs("short"), "stairs_inside": lambda: stairs("inside"),
           "adjacency": adjacency, "adjacency_t": lambda: adjacency(True), "no_edges": no_edges, "one_row": one_row}
_made = {}


def design(name):
    if name not in _made:
        _made[name] = DESIGNS[name]()
    return _made[name]


def degrees(d):
    """(in-degree of every destination, out-degree of every source)."""
    return np.bincount(d.dst, minlength=d.n_dst), np.bincount(d.src, minlength=d.n_src)


# ---------------------------------------------------------------------------------------------
# the cut rule, restated
# ---------------------------------------------------------------------------------------------
def expected_bounds(deg, parts):
    """``balanced_row_bounds`` as a plain loop: cut i (0 < i < parts) is one past the first row at which the running
    degree sum reaches ``i * total // parts`` (n + 1 when no row does), clamped to [0, n], the whole list made monotone
    between 0 and n."""
    deg = [int(x) for x in deg]
    n, total = len(deg), sum(int(x) for x in deg)
    cuts = []
    for i in range(1, parts):
        target = i * total // parts
        if n == 0:
            cut = target
        else:
            run, cut = 0, n + 1
            for r in range(n):
                run += deg[r]
                if run >= target:
                    cut = r + 1
                    break
        cuts.append(min(max(cut, 0), n))
    bounds, top = [], 0
    for b in [0] + cuts + [n]:
        top = max(top, b)
        bounds.append(top)
    return bounds


def equal_rows_condition(deg, parts, tol=TOL):
    """Whether ``choose_row_bounds`` takes equal row counts: n > 0 a multiple of ``parts``, and the heaviest block of
    n / parts consecutive rows holds at most ``(1 + tol) * total / parts`` edges (of a non-empty graph)."""
    deg = [int(x) for x in deg]
    n = len(deg)
    if n == 0 or n % parts:
        return False
    per = [sum(deg[i * (n // parts):(i + 1) * (n // parts)]) for i in range(parts)]
    mean = float(sum(per)) / parts
    return mean > 0 and float(max(per)) <= (1.0 + tol) * mean


def expected_choice(deg, parts, tol=TOL):
    if equal_rows_condition(deg, parts, tol):
        return [i * (len(deg) // parts) for i in range(parts + 1)]
    return expected_bounds(deg, parts)


def expected_shard(d, bounds, rank, transposed=False):
    """The rank's local edge list in PARENT order, rows shifted by ``lo``, with its values (``transposed``: the shard of
    the reversed edges — rows are sources)."""
    rows, cols = (d.src, d.dst) if transposed else (d.dst, d.src)
    lo, hi = bounds[rank], bounds[rank + 1]
    mine = [e for e in range(rows.size) if lo <= rows[e] < hi]
    mine = np.asarray(mine, np.int64)
    return Local(rows[mine] - lo, cols[mine], None if d.vals is None else d.vals[mine])


# ---------------------------------------------------------------------------------------------
# operands and references
# ---------------------------------------------------------------------------------------------
Operands = namedtuple("Operands", "X dY ss ds")
_operands, _refs = {}, {}


def operands(d, F):
    key = (d.name, F)
    if key not in _operands:
        rng = np.random.default_rng(1000 + 7 * F + len(d.name))
        ops_ = Operands(C.features(d.n_src, F, 11 * F + d.n_src), C.features(d.n_dst, F, 13 * F + d.n_dst),
                        rng.choice([0.5, 1.0, 2.0], d.n_src).astype(np.float32),
                        rng.choice([0.25, 0.5, 1.0, 2.0], d.n_dst).astype(np.float32))
        for a in ops_:
            a.setflags(write=False)
        _operands[key] = ops_
    return _operands[key]


def product(rows, cols, n_rows, X, w, gather_scale, out_scale, kept=None, gran=1.0):
    """``diag(out_scale) A diag(gather_scale) X`` over the COO list ``(rows, cols)`` by ``_spmm_cases.reference`` (float64,
    the exactness condition asserted); an empty scale (a shard without rows on that side) is no scale."""
    gs = None if gather_scale is None or np.size(gather_scale) == 0 else gather_scale
    os_ = None if out_scale is None or np.size(out_scale) == 0 else out_scale
    return C.reference(rows, cols, n_rows, X, w, gs, os_, kept, x_gran=gran if w is not None else 1.0)


def reference_forward(d, F, with_vals=True, has_ss=True, has_ds=True):
    """``diag(ds) A diag(ss) X`` of the whole graph, computed once per variant and shared (read-only)."""
    key = (d.name, F, "fwd", with_vals, has_ss, has_ds)
    if key not in _refs:
        o = operands(d, F)
        _refs[key] = product(d.dst, d.src, d.n_dst, o.X, d.vals if with_vals else None, o.ss if has_ss else None,
                             o.ds if has_ds else None, gran=d.gran)
        _refs[key].setflags(write=False)
    return _refs[key]


def reference_transposed(d, F, with_vals=True, has_ss=True, has_ds=True):
    """``diag(ss) A^T diag(ds) dY``: rows are sources, ``dst_scale`` applies to the gathered side, ``src_scale`` to the output."""
    key = (d.name, F, "bwd", with_vals, has_ss, has_ds)
    if key not in _refs:
        o = operands(d, F)
        _refs[key] = product(d.src, d.dst, d.n_src, o.dY, d.vals if with_vals else None, o.ds if has_ds else None,
                             o.ss if has_ss else None, gran=d.gran)
        _refs[key].setflags(write=False)
    return _refs[key]


def _h(a):
    """A host tensor holding a copy (the designs and references are read-only arrays)."""
    return torch.from_numpy(np.array(a))


def _t(a, device):
    return None if a is None else _h(a).to(device)


def _coo(d, device, with_vals=True):
    return _t(d.dst, device), _t(d.src, device), (_t(d.vals, device) if with_vals else None)


# (vals, ss, ds) given or None; the last one — unit values, no source scale — is what the workgroup-owned form takes
VARIANTS = ((True, True, True), (True, False, True), (True, True, False), (True, False, False), (False, True, True), (False, False, True))


def _into_nan_rows(rows, F, device, run):
    """Run ``run(out)`` on the middle rows of a larger NaN-filled buffer; the result, and that the rows around it still
    hold NaN (4 above — the slice starts on a 16-byte boundary at every width — and 2 below), as bench.py's ``y_local``."""
    buf = torch.full((rows + 6, F), NAN, dtype=torch.float32, device=device)
    out = buf[4:4 + rows]
    got = run(out)
    assert got.data_ptr() == out.data_ptr() and got.shape == out.shape
    assert bool(torch.isnan(buf[:4]).all()) and bool(torch.isnan(buf[4 + rows:]).all()), "rows around `out` were written"
    return got


# ---------------------------------------------------------------------------------------------
# checks without a process group
# ---------------------------------------------------------------------------------------------
def check_forward(device, d, world, F=8, variants=VARIANTS, hook=None):
    """Every rank's ``RowShard`` under ``choose_row_bounds`` (what bench.py cuts by): local structure, values and
    products.  Returns the bounds."""
    from dream_gnn_amd import shard

    deg_in, _ = degrees(d)
    bounds = shard.choose_row_bounds(_t(deg_in, device), world)
    assert bounds.dtype == torch.int64 and bounds.tolist() == expected_choice(deg_in, world), (d.name, world, bounds.tolist())
    blist = bounds.tolist()
    o = operands(d, F)
    X, ss, ds = _t(o.X, device), _t(o.ss, device), _t(o.ds, device)
    for with_vals in sorted({v[0] for v in variants}, reverse=True):
        dst, src, vals = _coo(d, device, with_vals)
        shards = [shard.RowShard(dst, src, d.n_dst, d.n_src, bounds, r, vals) for r in range(world)]
        assert sum(sh.nnz for sh in shards) == d.dst.size
        for r, sh in enumerate(shards):
            lo, hi = blist[r], blist[r + 1]
            exp = expected_shard(d, blist, r)
            assert (sh.lo, sh.hi, sh.rank, sh.world, sh.nnz) == (lo, hi, r, world, exp.dst.size)
            assert sh.max_rows == max(blist[i + 1] - blist[i] for i in range(world))
            assert sh.local.n_dst == hi - lo and sh.local.n_src == d.n_src
            indptr = sh.local.indptr.cpu().numpy().astype(np.int64)
            assert indptr.shape == (hi - lo + 1,) and indptr[0] == 0 and np.array_equal(np.diff(indptr), deg_in[lo:hi])
            order = np.argsort(exp.dst, kind="stable")  # the stable CSR of the local list: parent order inside a row
            assert np.array_equal(sh.local.indices.cpu().numpy(), exp.src[order])
            assert np.array_equal(sh.local.eid.cpu().numpy(), order)
            if with_vals:
                assert torch.equal(sh.local._coo_vals.cpu(), _h(exp.vals))
            for (_, has_ss, has_ds) in (v for v in variants if v[0] == with_vals):
                want = _h(reference_forward(d, F, with_vals, has_ss, has_ds)[lo:hi])
                a, b = ss if has_ss else None, ds if has_ds else None
                y = sh.spmm_local(X, a, b)
                y2 = _into_nan_rows(hi - lo, F, device, lambda out: sh.spmm_local(X, a, b, out=out))
                for got in (y, y2):
                    assert got.shape == (hi - lo, F) and got.dtype == torch.float32
                    assert torch.equal(got.cpu(), want), (d.name, world, r, with_vals, has_ss, has_ds)
                if exp.dst.size == 0:
                    assert not bool(y.any())  # rows but no edges: exact zeros (no rows: shape (0, F))
            if hook is not None:
                hook("forward", sh.local, F)
    return blist


def check_backward(device, d, world, F=8, hook=None):
    """``ShardedRelation(..., rank=r, world=W)`` for every r: both bounds by the restated rule, ``fwd`` / ``bwd`` local
    products concatenated equal the forward / transposed references."""
    from dream_gnn_amd import shard

    deg_in, deg_out = degrees(d)
    o = operands(d, F)
    X, dY, ss, ds = _t(o.X, device), _t(o.dY, device), _t(o.ss, device), _t(o.ds, device)
    dst, src, vals = _coo(d, device)
    fwd, bwd = [], []
    for r in range(world):
        rel = shard.ShardedRelation(dst, src, d.n_dst, d.n_src, vals=vals, rank=r, world=world)
        assert rel.fwd.bounds == expected_bounds(deg_in, world) and rel.bwd.bounds == expected_bounds(deg_out, world)
        assert (rel.fwd.n_dst, rel.fwd.n_src, rel.bwd.n_dst, rel.bwd.n_src) == (d.n_dst, d.n_src, d.n_src, d.n_dst)
        exp = expected_shard(d, rel.bwd.bounds, r, transposed=True)
        assert rel.bwd.nnz == exp.dst.size and torch.equal(rel.bwd.local._coo_vals.cpu(), _h(exp.vals))
        fwd.append(rel.fwd.spmm_local(X, ss, ds))
        part = rel.bwd.spmm_local(dY, ds, ss)
        assert part.shape == (rel.bwd.hi - rel.bwd.lo, F)
        bwd.append(_into_nan_rows(part.shape[0], F, device, lambda out: rel.bwd.spmm_local(dY, ds, ss, out=out)))
        assert torch.equal(part, bwd[-1])
        if hook is not None:
            hook("forward", rel.fwd.local, F)
            hook("forward", rel.bwd.local, F)
    assert torch.equal(torch.cat(fwd).cpu(), _h(reference_forward(d, F)))
    assert torch.equal(torch.cat(bwd).cpu(), _h(reference_transposed(d, F))), (d.name, world)


def check_dropped(device, oracle, d, world, F=8, hook=None):
    """bench.py's dropout step on every rank: ``sh.local.dropped(desc)`` with a description over the SHARD's own edges
    (``oracle.random_subset_select``, a fixed seed per rank); the reference keeps ``oracle.keep_mask`` of that description
    over ``expected_shard``'s local edge order.  Forward and ``spmm_t``."""
    from dream_gnn_amd import shard

    deg_in, _ = degrees(d)
    blist = expected_choice(deg_in, world)
    bounds = torch.tensor(blist, dtype=torch.int64)
    o = operands(d, F)
    X, dY, ss, ds = _t(o.X, device), _t(o.dY, device), _t(o.ss, device), _t(o.ds, device)
    dst, src, vals = _coo(d, device)
    for r in range(world):
        lo, hi = blist[r], blist[r + 1]
        sh = shard.RowShard(dst, src, d.n_dst, d.n_src, bounds, r, vals)
        exp = expected_shard(d, blist, r)
        E = exp.dst.size
        assert sh.nnz == E
        desc = oracle.random_subset_select(E, int(E * DROP_KEEP), DROP_SEED + r)
        kept = np.asarray(oracle.keep_mask(desc, E)).astype(bool)
        assert kept.sum() == int(E * DROP_KEEP)
        view = sh.local.dropped(_t(np.ascontiguousarray(desc).reshape(1, 8), device))
        ds_local = ds[lo:hi].contiguous()
        want = product(exp.dst, exp.src, hi - lo, o.X, exp.vals, o.ss, o.ds[lo:hi], kept, d.gran)
        got = view.spmm(X, ss, ds_local)
        assert got.shape == (hi - lo, F) and torch.equal(got.cpu(), _h(want)), (d.name, world, r, "dropped")
        want_t = product(exp.src, exp.dst, d.n_src, o.dY[lo:hi], exp.vals, o.ds[lo:hi], o.ss, kept, d.gran)
        dY_local = dY[lo:hi].contiguous()
        got_t = view.spmm_t(dY_local, ss, ds_local)
        got_t2 = _into_nan_rows(d.n_src, F, device, lambda out: view.spmm_t(dY_local, ss, ds_local, out=out))
        for g in (got_t, got_t2):
            assert g.shape == (d.n_src, F) and torch.equal(g.cpu(), _h(want_t)), (d.name, world, r, "dropped_t")
        if hook is not None:
            hook("dropped", view, F)


def check_unsharded(device, d, world, F=8):
    """The concatenated ranks against the unsharded library: ``CSRGraph(dst, src, ...).spmm`` of the whole graph."""
    from dream_gnn_amd import ops, shard

    deg_in, _ = degrees(d)
    bounds = shard.choose_row_bounds(_t(deg_in, device), world)
    o = operands(d, F)
    X, ss, ds = _t(o.X, device), _t(o.ss, device), _t(o.ds, device)
    dst, src, vals = _coo(d, device)
    whole = ops.CSRGraph(dst.to(torch.int32), src.to(torch.int32), d.n_dst, d.n_src, vals=vals).spmm(X, ss, ds)
    parts = [shard.RowShard(dst, src, d.n_dst, d.n_src, bounds, r, vals).spmm_local(X, ss, ds) for r in range(world)]
    assert torch.equal(torch.cat(parts), whole) and torch.equal(whole.cpu(), _h(reference_forward(d, F)))


# ---------------------------------------------------------------------------------------------
# the exchange, inside a process group
# ---------------------------------------------------------------------------------------------
def check_gather(device, d, F=8, edge_shard=True):
    """This rank's part of the exchange, every result held to the full references: ``gather_rows`` in both forms,
    allocating and into a NaN-filled ``out`` (which must come back fully written); ``rel(X, ss, ds)`` and its
    ``backward`` under both class-level exchange settings; ``EdgeShard.spmm`` on the strided partition
    ``e % world == rank`` (``edge_shard=False``: a backend whose all-reduce does not take this device's tensors).
    Returns True, or the list of what differed."""
    import torch.distributed as dist

    from dream_gnn_amd import shard

    rank, world = dist.get_rank(), dist.get_world_size()
    deg_in, deg_out = degrees(d)
    o = operands(d, F)
    X, dY, ss, ds = _t(o.X, device), _t(o.dY, device), _t(o.ss, device), _t(o.ds, device)
    dst, src, vals = _coo(d, device)
    want, want_t = _h(reference_forward(d, F)), _h(reference_transposed(d, F))
    bad = []

    def hold(what, got, ref):
        if got.shape != ref.shape or not torch.equal(got.detach().cpu(), ref):
            bad.append(what)

    bounds = shard.choose_row_bounds(_t(deg_in, device), world)
    if bounds.tolist() != expected_choice(deg_in, world):
        bad.append("bounds")
    sh = shard.RowShard(dst, src, d.n_dst, d.n_src, bounds, rank, vals)
    y_local = sh.spmm_local(X, ss, ds)
    for form in ("allgather", "direct"):
        hold("gather_rows/" + form, sh.gather_rows(y_local, exchange=form), want)
        out = torch.full((d.n_dst, F), NAN, dtype=torch.float32, device=device)
        res = sh.gather_rows(y_local, out=out, exchange=form)
        if res.data_ptr() != out.data_ptr():
            bad.append("gather_rows/%s/out is not returned" % form)
        hold("gather_rows/%s/out" % form, out, want)
    rel = shard.ShardedRelation(dst, src, d.n_dst, d.n_src, vals=vals)  # rank / world from the process group
    if rel.fwd.bounds != expected_bounds(deg_in, world) or rel.bwd.bounds != expected_bounds(deg_out, world):
        bad.append("relation bounds")
    saved = shard.RowShard.exchange
    try:
        for form in ("allgather", "direct"):
            shard.RowShard.exchange = form
            x = X.clone().requires_grad_(True)
            y = rel(x, ss, ds)
            y.backward(dY)
            hold("relation/%s/forward" % form, y, want)
            hold("relation/%s/backward" % form, x.grad, want_t)
    finally:
        shard.RowShard.exchange = saved
    if edge_shard:
        mine = np.arange(d.dst.size) % world == rank
        es = shard.EdgeShard(_t(d.dst[mine], device), _t(d.src[mine], device), d.n_dst, d.n_src, vals=_t(d.vals[mine], device))
        hold("edge_shard", es.spmm(X, ss, ds), want)
        hold("edge_shard/no dst_scale", es.spmm(X, ss, None), _h(reference_forward(d, F, True, True, False)))
    return True if not bad else bad
