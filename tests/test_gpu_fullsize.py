"""BASELINE-size checks on the GPU (config 4: 100k x 50k nodes, 10 M edges, kNN-64 graphs,
F = 128): size-independent properties, oracle spot checks on sampled rows, and (r4) EVERY row of every
product of the bench step against the f64 oracle (the OpenMP oracle does a 10 M-edge product in ~0.1-0.5 s on
the box's 16 cores: `test_every_row_of_every_config4_product`)."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ND, NS, E, F = 100_000, 50_000, 10_000_000, 128
# DGMI_FORCE_KERNEL=planned|sliced pins the kernel choice (A/B aid): the numeric checks below still
# run, only the assertions about WHICH kernel was picked are skipped.
FORCED = bool(__import__("os").environ.get("DGMI_FORCE_KERNEL"))


@pytest.fixture(scope="module")
def cfg4(dev):
    from dream_gnn_amd import ops, synth

    drug, dis = synth.bipartite_edges(ND, NS, E, seed=0, device=dev)
    g = ops.CSRGraph(dis, drug, NS, ND)  # drug -> disease
    return drug, dis, g


def _rows_vs_oracle(oracle, g, X, rows, y, vals=None, ss=None, ds=None, rtol=1e-5):
    """Recompute a sample of destination rows with the f64 oracle."""
    indptr = g.indptr.cpu().numpy()
    indices = g.indices.cpu().numpy()
    vv = None if g.vals is None else g.vals.cpu().numpy()
    Xn = X.cpu().numpy()
    for r in rows:
        lo, hi = int(indptr[r]), int(indptr[r + 1])
        sub_ptr = np.array([0, hi - lo], np.int32)
        ref = oracle.spmm_csr(sub_ptr, indices[lo:hi], None if vv is None else vv[lo:hi], Xn,
                              None if ss is None else ss.cpu().numpy(),
                              None if ds is None else ds.cpu().numpy()[r:r + 1], acc="f64")[0]
        got = y[r].cpu().numpy().astype(np.float64)
        scale = max(np.abs(ref).max(), 1e-30)
        assert np.abs(got - ref).max() <= rtol * scale, "row %d (deg %d): rel %.2e" % (r, hi - lo, np.abs(got - ref).max() / scale)


def test_csr_build_is_a_stable_sort_at_full_size(cfg4):
    drug, dis, g = cfg4
    indptr, indices, eid = g.indptr.long(), g.indices, g.eid.long()
    assert int(indptr[0]) == 0 and int(indptr[-1]) == E
    assert bool((indptr[1:] >= indptr[:-1]).all())
    assert torch.equal(torch.bincount(dis.long(), minlength=NS), indptr[1:] - indptr[:-1])
    assert torch.equal(torch.sort(eid)[0], torch.arange(E, device=eid.device))  # a permutation
    assert torch.equal(indices, drug[eid])  # indices[p] = col[eid[p]]
    row_sorted = dis[eid]
    assert bool((row_sorted[1:] >= row_sorted[:-1]).all())  # sorted by destination
    same = row_sorted[1:] == row_sorted[:-1]
    assert bool((eid[1:][same] > eid[:-1][same]).all())  # ties keep input order (stable)
    # idempotence: rebuilding from the CSR-ordered edge list is the identity permutation
    from dream_gnn_amd import ops

    ip2, ix2, eid2 = ops.csr_from_coo(row_sorted.contiguous(), indices, NS)
    assert torch.equal(ip2, g.indptr) and torch.equal(ix2, indices)
    assert torch.equal(eid2.long(), torch.arange(E, device=eid.device))


def test_spmm_full_size_properties(oracle, cfg4, dev):
    from dream_gnn_amd import ops, synth

    drug, dis, g = cfg4
    gen = torch.Generator(device=dev).manual_seed(3)
    X = torch.randn(ND, F, generator=gen, device=dev)
    Z = torch.randn(ND, F, generator=gen, device=dev)
    cj, ci = synth.degree_norm(drug, ND), synth.degree_norm(dis, NS)
    # A @ ones = in-degree, exactly (integers < 2^24 are exact in fp32)
    deg = (g.indptr[1:] - g.indptr[:-1]).float()
    ones = g.spmm(torch.ones(ND, F, device=dev))
    assert torch.equal(ones, deg[:, None].expand(-1, F))
    # planned launch == wave-per-row launch bit for bit when no row exceeds the chunk
    y_rows = ops.spmm_csr_raw(g.indptr, g.indices, None, X, cj, ci)
    y_plan = ops.spmm_csr_raw(g.indptr, g.indices, None, X, cj, ci, plan=g.plan)
    assert int(deg.max()) <= g.plan.chunk and torch.equal(y_plan, y_rows)
    # config 4's 51 MB feature table selects the XCD-local sliced kernel: same product, summed
    # slice by slice
    y = g.spmm(X, cj, ci)
    assert g.regular and (FORCED or g._sliced is not None)
    assert float((y - y_rows).abs().max()) <= 1e-5 * float(y_rows.abs().max())
    assert torch.equal(y, g.spmm(X, cj, ci))  # run-to-run reproducible
    # linearity
    lin = g.spmm(2.0 * X - 0.5 * Z, cj, ci)
    ref = 2.0 * y - 0.5 * g.spmm(Z, cj, ci)
    assert float((lin - ref).abs().max()) <= 1e-5 * float(ref.abs().max())
    # adjoint: <A X, W> == <X, A^T W> with both scalings (the autograd formula)
    W = torch.randn(NS, F, generator=gen, device=dev)
    lhs = (y.double() * W.double()).sum()
    rhs = (X.double() * g.spmm_t(W, cj, ci).double()).sum()
    assert abs(float(lhs - rhs)) <= 1e-6 * float((y.double().abs() * W.double().abs()).sum())
    # checksum of checksums: column sums of Y equal sum_e ci[dst]*cj[src]*X[src]
    w_src = torch.zeros(ND, dtype=torch.float64, device=dev).index_add_(0, drug.long(), ci.double()[dis.long()])
    col_ref = ((w_src * cj.double())[:, None] * X.double()).sum(0)
    assert float((y.double().sum(0) - col_ref).abs().max()) <= 1e-6 * float(col_ref.abs().max() + 1)
    # oracle on sampled rows (first, last, max-degree, random)
    rows = [0, NS - 1, int(deg.argmax())] + np.random.default_rng(0).integers(0, NS, 40).tolist()
    _rows_vs_oracle(oracle, g, X, rows, y, ss=cj, ds=ci)


def test_weighted_knn64_full_size(oracle, dev):
    from dream_gnn_amd import ops, synth

    n = 100_000
    r, c, v = synth.knn_sim_graph(n, 64, seed=2, device=dev)
    g = ops.CSRGraph(r, c, n, n, vals=v)
    assert 128 * n <= g.nnz <= 130 * n
    X = torch.randn(n, F, device=dev)
    y = g.spmm(X)
    # rows of D^-1(A + A^T + I) sum to one: A @ ones = ones (to rounding)
    ones = g.spmm(torch.ones(n, F, device=dev))
    assert float((ones - 1).abs().max()) <= 1e-5
    W = torch.randn(n, F, device=dev)
    lhs = (y.double() * W.double()).sum()
    rhs = (X.double() * g.spmm_t(W).double()).sum()
    assert abs(float(lhs - rhs)) <= 1e-6 * float((y.double().abs() * W.double().abs()).sum())
    deg = g.indptr[1:] - g.indptr[:-1]
    _rows_vs_oracle(oracle, g, X, [0, n - 1, int(deg.argmax()), int(deg.argmin())] + list(range(5000, 5020)), y)


def test_power_law_degrees_full_size(oracle, dev):
    """10 M edges with Zipf(1.2) destination degrees: the longest row holds ~2 M edges.  The
    planned launch must agree with the oracle there too (chunk partials summed in order)."""
    from dream_gnn_amd import ops

    gen = torch.Generator(device=dev).manual_seed(11)
    p = 1.0 / torch.arange(1, NS + 1, device=dev, dtype=torch.float64) ** 1.2
    dst = torch.multinomial(p / p.sum(), E, replacement=True, generator=gen).to(torch.int32)
    src = torch.randint(0, ND, (E,), generator=gen, device=dev, dtype=torch.int32)
    g = ops.CSRGraph(dst, src, NS, ND)
    deg = g.indptr[1:] - g.indptr[:-1]
    n_items, n_long, n_slots, chunk = g.plan.header()[:4]
    assert int(deg.max()) > 1_000_000 and n_long == int((deg > chunk).sum()) and n_long > 0
    assert n_items == int(torch.clamp((deg + chunk - 1) // chunk, min=1).sum())
    X = torch.randn(ND, F, generator=gen, device=dev)
    y = g.spmm(X)
    assert torch.equal(y, g.spmm(X))
    # not regular -> rows cut into virtual rows of <= SPLIT_ROW_EDGES edges, XCD-local kernel on those, ordered re-sum
    assert not g.regular
    if not FORCED:
        assert g._S.split is not None and g._S.sliced is None
        # (r4) the light rows (< 24 edges: most rows of a power law, few of its edges) are gathered by the second stage
        # straight from the source table; only the heavy rows are cut into virtual rows for the XCD-local kernel
        heavy = deg >= ops.SPLIT_LIGHT_ROW_EDGES
        assert g._S.split.has_light and int((~heavy).sum()) * 4 >= NS
        assert g._S.split.n_virtual == int(((deg[heavy] + ops.SPLIT_ROW_EDGES - 1) // ops.SPLIT_ROW_EDGES).sum())
    y_planned = ops.spmm_csr_raw(g.indptr, g.indices, None, X, plan=g.plan)
    assert float((y - y_planned).abs().max()) <= 1e-5 * float(y_planned.abs().max())
    ones = g.spmm(torch.ones(ND, F, device=dev))
    assert torch.equal(ones, deg.float()[:, None].expand(-1, F))  # exact while deg < 2^24
    order = torch.argsort(deg, descending=True)
    rows = order[:3].tolist() + order[-3:].tolist() + order[1000:1010].tolist()
    _rows_vs_oracle(oracle, g, X, rows, y)
    W = torch.randn(NS, F, generator=gen, device=dev)
    lhs = (y.double() * W.double()).sum()
    rhs = (X.double() * g.spmm_t(W).double()).sum()
    assert abs(float(lhs - rhs)) <= 1e-6 * float((y.double().abs() * W.double().abs()).sum())
    assert g.regular_t and (FORCED or g._S.sliced_t is not None)  # source degrees are uniform: plain sliced backward
    # the mirrored case: a graph whose SOURCE degrees are the power law (its transpose takes the split path)
    gt = ops.CSRGraph(src, dst, ND, NS)
    Xs = torch.randn(NS, F, generator=gen, device=dev)
    V = torch.randn(ND, F, generator=gen, device=dev)
    lhs = (gt.spmm(Xs).double() * V.double()).sum()
    dxs = gt.spmm_t(V)
    assert FORCED or gt._S.split_t is not None
    rhs = (Xs.double() * dxs.double()).sum()
    assert abs(float(lhs - rhs)) <= 1e-6 * float((gt.spmm(Xs).double().abs() * V.double().abs()).sum())


def test_edge_dropout_rebuild_full_size(cfg4, dev):
    """augmentation.py:13-89 at config-4 size: a random 90 % prefix per relation, CSR rebuilt
    on the device without a host sync, norms copied (stale), result still a valid SpMM."""
    from dream_gnn_amd import graph as G

    drug, dis, _ = cfg4
    hg = G.HeteroGraph({("drug", "0", "disease"): (drug, dis), ("disease", "rev-0", "drug"): (dis, drug)},
                       {"drug": ND, "disease": NS})
    hg.nodes["drug"].data.update({"ci": torch.ones(ND, 1, device=dev), "cj": torch.ones(ND, 1, device=dev)})
    hg.nodes["disease"].data.update({"ci": torch.ones(NS, 1, device=dev), "cj": torch.ones(NS, 1, device=dev)})
    dropped = G.random_edge_dropout(hg, 0.1)
    for et in ("0", "rev-0"):
        rel = dropped[et]
        assert rel.number_of_edges() == max(1, int(E * 0.9)) and rel.trusted
        csr = rel.csr  # a keep-mask view of the parent's CSR: same structure, no re-sort
        assert csr.indptr is hg[et].csr.indptr and csr.nnz == E
        deg = torch.bincount(rel.dst.long(), minlength=rel.n_dst)  # kept edges, materialised on demand
        ones = csr.spmm(torch.ones(rel.n_src, 8, device=dev))
        assert torch.equal(ones[:, 0], deg.float())
        # same product as a CSR rebuilt from the kept edge list (the reference's construction)
        from dream_gnn_amd import ops

        X = torch.randn(rel.n_src, 128, device=dev)
        rebuilt = ops.CSRGraph(rel.dst, rel.src, rel.n_dst, rel.n_src, check_range=False)
        a, b = csr.spmm(X), rebuilt.spmm(X)
        assert float((a - b).abs().max()) <= 1e-5 * float(b.abs().max())
        W = torch.randn(rel.n_dst, 128, device=dev)
        a, b = csr.spmm_t(W), rebuilt.spmm_t(W)
        assert float((a - b).abs().max()) <= 1e-5 * float(b.abs().max())
    # the two directions were dropped independently: rev-0 is no longer the transpose of 0
    a = torch.sort(dropped["0"].src.long() * NS + dropped["0"].dst.long())[0]
    b = torch.sort(dropped["rev-0"].dst.long() * NS + dropped["rev-0"].src.long())[0]
    assert not torch.equal(a, b)


def test_addresses_beyond_4_gib(oracle, dev):
    """Feature tables and edge outputs larger than 2^32 bytes: every kernel must do its row
    addressing in 64 bits.  9 M x 128 fp32 sources (4.6 GB) with all edges pointing into the top
    of the table; a 5.1 GB gather-concat output."""
    from dream_gnn_amd import ops

    gen = torch.Generator(device=dev).manual_seed(5)
    n_src, n_dst, E, Fw = 9_000_000, 2_000, 200_000, 128
    X = torch.empty(n_src, Fw, device=dev)
    X[-600_000:] = torch.randn(600_000, Fw, generator=gen, device=dev)  # only the part that is read needs data
    src = (n_src - 1 - torch.randint(0, 600_000, (E,), generator=gen, device=dev)).to(torch.int32)
    dst = torch.randint(0, n_dst, (E,), generator=gen, device=dev, dtype=torch.int32)
    vals = torch.rand(E, generator=gen, device=dev)
    g = ops.CSRGraph(dst, src, n_dst, n_src, vals=vals)
    ref = torch.zeros(n_dst, Fw, device=dev, dtype=torch.float64).index_add_(
        0, dst.long(), X.index_select(0, src.long()).double() * vals.double()[:, None])
    sl = ops.SlicedCSR(dst, src, n_dst, n_src, vals=vals)
    for y in (ops.spmm_csr_raw(g.indptr, g.indices, g.vals, X),            # a wave per row
              ops.spmm_csr_raw(g.indptr, g.indices, g.vals, X, plan=g.plan),  # planned
              sl.spmm(X)):                                                    # XCD-sliced
        assert float((y.double() - ref).abs().max()) <= 1e-5 * float(ref.abs().max())
    # the XCD-sliced kernel's 64-bit row addresses in two more template variants: src_scale in the kernel, dropout on the fly
    ss = torch.ones(n_src, device=dev)
    ss[-600_000:] = torch.rand(600_000, generator=gen, device=dev) + 0.5
    kept = ops.keep_mask(ops.random_subset_select(E, int(E * 0.7), 11, dev), E)
    for y, w in ((sl.spmm(X, ss), vals * ss[src.long()]),
                 (sl.spmm(X, keep=ops.random_subset_select(E, int(E * 0.7), 11, dev)), vals * kept)):
        ref_w = torch.zeros(n_dst, Fw, device=dev, dtype=torch.float64).index_add_(
            0, dst.long(), X.index_select(0, src.long()).double() * w.double()[:, None])
        assert float((y.double() - ref_w).abs().max()) <= 1e-5 * float(ref_w.abs().max())
    del sl, ss, ref_w
    # transpose product writes rows beyond the 4 GiB mark of a 9 M-row output
    W = torch.randn(n_dst, Fw, generator=gen, device=dev)
    dx = g.spmm_t(W)
    rows = src[:200].long()
    it, ix, vt, _ = g.transposed()
    for r in rows[:20].tolist():
        lo, hi = int(it[r]), int(it[r + 1])
        want = (W.index_select(0, ix[lo:hi].long()).double() * vt[lo:hi].double()[:, None]).sum(0)
        assert float((dx[r].double() - want).abs().max()) <= 1e-5 * float(want.abs().max() + 1e-30)
    del X, dx, g
    torch.cuda.empty_cache()
    # gather-concat with a > 4 GiB output
    Ea, n_a, n_b = 5_000_000, 1000, 700
    A, B = torch.randn(n_a, 128, device=dev), torch.randn(n_b, 128, device=dev)
    s = torch.randint(0, n_a, (Ea,), generator=gen, device=dev, dtype=torch.int32)
    d = torch.randint(0, n_b, (Ea,), generator=gen, device=dev, dtype=torch.int32)
    out = ops.gather_concat_raw(s, d, A, B)
    assert out.numel() * 4 > 2 ** 32
    for e in (0, 1, Ea // 2, Ea - 2, Ea - 1):
        assert torch.equal(out[e, :128], A[int(s[e])]) and torch.equal(out[e, 128:], B[int(d[e])])
    tail = slice(Ea - 4096, Ea)
    assert torch.equal(out[tail], torch.cat([A[s[tail].long()], B[d[tail].long()]], 1))
    ga = ops.gather_add_raw(s, d, A, B)
    assert torch.equal(ga[tail], A[s[tail].long()] + B[d[tail].long()])


def _every_row(oracle, g_csr, vals_csr, X, ss, ds, y, what, threads):
    """All rows, elementwise forward-error bound 1e-5 * sum |terms| against the f64 oracle (tests/test_gpu_configs.py's
    bar), plus 1e-5 of the output's magnitude."""
    indptr, indices = g_csr
    tn = lambda a: None if a is None else a.cpu().numpy()
    args = (tn(indptr), tn(indices), tn(vals_csr), tn(X), tn(ss), tn(ds))
    ref = oracle.spmm_csr(*args, acc="f64", threads=threads, validate=False)
    bound = oracle.spmm_csr(*args, acc="abs", validate=False)
    err = np.abs(y.cpu().numpy().astype(np.float64) - ref)
    worst = float((err / (1e-5 * bound + 1e-30)).max())
    assert worst <= 1.0, "%s: worst element at %.2f of its bound" % (what, worst)
    assert float(err.max()) <= 1e-5 * float(np.abs(ref).max()), what
    return worst


def test_every_row_of_every_config4_product(oracle, cfg4, dev):
    """the four GCMC products of bench.py's step (copy_u -> sum with cj / ci fused, forward and
    transpose, both directions), the kNN-64 product and its transpose (value = row scale x multiplicity form), and
    one edge-dropped product of each kind — EVERY destination row at 10 M / 12.9 M edges against the f64 oracle
    (layers.py:224-234, :312)."""
    from dream_gnn_amd import ops, synth

    drug, dis, g = cfg4
    threads = oracle.max_threads()
    gen = torch.Generator(device=dev).manual_seed(3)
    x_drug = torch.randn(ND, F, generator=gen, device=dev)
    x_dis = torch.randn(NS, F, generator=gen, device=dev)
    cj, ci = synth.degree_norm(drug, ND), synth.degree_norm(dis, NS)
    gr = ops.CSRGraph(drug, dis, ND, NS)  # disease -> drug
    worst = {}
    for name, gg, X, ss, ds in (("drug->disease", g, x_drug, cj, ci), ("disease->drug", gr, x_dis, ci, cj)):
        worst["fwd " + name] = _every_row(oracle, (gg.indptr, gg.indices), None, X, ss, ds, gg.spmm(X, ss, ds), "fwd " + name, threads)
        it, ix, _, _ = gg.transposed()
        W = x_dis if gg is g else x_drug  # any (n_dst, F) matrix
        worst["bwd " + name] = _every_row(oracle, (it, ix), None, W, ds, ss, gg.spmm_t(W, ss, ds), "bwd " + name, threads)
    assert FORCED or (g._sliced is not None and g._sliced_t is not None)
    # edge-dropped (what every training step runs, train.py:267): 10 % of the edges, through the compacted layout,
    # against the oracle on a CSR of the kept edges only
    keep_n = max(1, int(E * 0.9))
    desc = ops.random_subset_select(E, keep_n, 99, dev)
    view = g.dropped(desc)
    kept = ops.keep_mask(desc, E).bool()
    gk = ops.csr_from_coo(dis[kept].contiguous(), drug[kept].contiguous(), NS, ND)
    worst["dropped fwd drug->disease"] = _every_row(oracle, gk[:2], None, x_drug, cj, ci, view.spmm(x_drug, cj, ci),
                                                    "dropped fwd drug->disease", threads)
    gkt = ops.csr_from_coo(drug[kept].contiguous(), dis[kept].contiguous(), ND, NS)
    worst["dropped bwd drug->disease"] = _every_row(oracle, gkt[:2], None, x_dis, ci, cj, view.spmm_t(x_dis, cj, ci),
                                                    "dropped bwd drug->disease", threads)
    assert FORCED or not ops.COMPACT_DROPPED or ("sliced" in view._c and "sliced_t" in view._c)
    del view, gk, gkt, gr
    # FGCN: th.spmm(adj, support) on the kNN-64 adjacency, forward and transpose, un-dropped and dropped
    n = ND
    r, c, v = synth.knn_sim_graph(n, 64, seed=21, device=dev)
    ga = ops.CSRGraph(r, c, n, n, vals=v)
    y = ga.spmm(x_drug)
    assert FORCED or not ops.MULT_FORM or ga._mult_form() is not None  # the reference's format: no value stream
    worst["fgcn fwd"] = _every_row(oracle, (ga.indptr, ga.indices), ga.vals, x_drug, None, None, y, "fgcn fwd", threads)
    it, ix, vt, _ = ga.transposed()
    worst["fgcn bwd"] = _every_row(oracle, (it, ix), vt, x_drug, None, None, ga.spmm_t(x_drug), "fgcn bwd", threads)
    nnz = ga.nnz
    desc = ops.random_subset_select(nnz, int(nnz * 0.9), 5, dev)
    kept = ops.keep_mask(desc, nnz).bool()
    ik, xk, ek = ops.csr_from_coo(r[kept].contiguous(), c[kept].contiguous(), n, n)
    vk = ops.gather_f32(v[kept].contiguous(), ek)
    worst["fgcn dropped fwd"] = _every_row(oracle, (ik, xk), vk, x_drug, None, None, ga.dropped(desc).spmm(x_drug), "fgcn dropped fwd", threads)
    print("worst element / bound per product:", {k: round(w, 3) for k, w in worst.items()})
