"""The cosine kNN search (csrc/dgmi_knn.hip, csrc/dgmi_knn_screen.hip) on the lattice rows of _knn_cases.py, ZERO
tolerance.  Every similarity of those rows is an integer multiple of 1 / nz that the fp32 MFMA chain, the bf16 screen and
the rescoring's dot product return exactly, whatever the order of their sums, so the reference is an integer matrix
product (evaluated on the device in float64 row blocks) and ties are exact: the k-th boundary cuts a tie class for most
queries, antipodal rows have negative neighbours, zero rows see 0 everywhere, 300 copies of one row form one class.

`dgmi_knn_cosine_topk_f32` is called through ctypes with a workspace the test owns; afterwards the sample's lower bound
`tau0`, the emission thresholds `thr`, the per-region entry counts `cnt` and the take-over `flags` are read out of it at
the offsets `_knn_cases.screen_layout` restates.  For every query of every case:
  (a) contract: k valid distinct ids, similarities non-increasing and equal to the integer top-k multiset, every candidate
      strictly above the k-th value present, similarity exactly 1 first for a non-zero row;
  (b) tau0 is a lattice value <= the true k-th largest similarity (k <= 4: exactly the k-th largest over the sampled
      tiles, `_knn_cases.sampled_tiles`), thr == fp32(tau0 - 2 * 0.008f);
  (c) flags == (some region was offered more than its cap); an unflagged query was offered, over its regions, exactly
      #{c < N: S[q, c] >= thr[q]} entries — no pair twice, none lost at a tile edge; on the `knn_screen_kernel` paths
      (rectangle, triangle, one-chunk 256 x 256, knn_screen_first) every region's count equals `emit_regions`;
  (d) order: the rescoring pass orders by (score desc, id asc) and every candidate at or above tau is in the buffer, so
      an unflagged query's list equals `expected_topk` id for id.  This pins the PRESENT rescoring order: the public
      contract leaves ties free.  The issue assumed this for every unflagged query; for k <= 16 the take-over
      (`knn_cosine_topk_exact_tiles`) recomputes the whole 32-query tile of a flagged query, unflagged members included,
      and its 8-list merge orders ties by list, not by id — so for k <= 16 (d) holds for the queries of 32-query tiles
      without a flagged member, and the others are held to (a).  For k > 16 the take-over (`knn_exact_rows_kernel`) works
      per query and orders through the same `wave_topk_insert`: (d) holds for every query, flagged or not;
  (e) the case is not hollow: at least a quarter of the queries are unflagged AND tie-cut, every antipodal row is
      unflagged; a zero row is offered all N candidates, so it is flagged exactly when one of its regions spans more ids
      than the region's cap (always for k <= 8), and every row of the 300-block is flagged wherever one of its regions
      holds more of the block than the cap: on the full rectangle at k <= 8 always (cap 128, the block falls into at most
      two regions).  Not everywhere, as the issue assumed: at k > 16 a rectangle region has 512 slots — more than the 256
      or 384 ids a region spans at 1 536 / 2 085 rows, so nothing is flagged there and `knn_exact_rows_kernel` is reached
      from 40 997 and 49 452 rows and on the mostly-zero rows instead — and under the triangular sweep the block's last
      rows receive most of it through the column region of 8 x cap slots.
The small-N fp32 kernel + merge is held to (a)."""
import functools

import numpy as np
import pytest
import torch

import _knn_cases as K

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def _knobs_back():
    from dream_gnn_amd import _lib

    yield
    _lib.set_tuning("knn_screen_first", 0)
    _lib.set_tuning("knn_pool_chunks", 0)


_ref = {}


def _reference(dev, d):
    """Once per design: the numerators on the device (float64) and, per query, the keys of its 65 best candidates by
    (similarity desc, id asc): key = (S + nz) * M + (M - 1 - id)."""
    key = id(d)
    if key not in _ref:
        xi = torch.from_numpy(d.num.astype(np.float64)).to(dev)
        N = d.N
        M = 1 << (N - 1).bit_length()
        kk = min(N, 65)
        top = torch.empty((N, kk), dtype=torch.int64, device=dev)
        ids = (M - 1 - torch.arange(N, device=dev))[None, :]
        B = max(1, (1 << 26) // N)
        for lo in range(0, N, B):
            S = (xi[lo:lo + B] @ xi.t()).long()
            top[lo:lo + B] = torch.topk((S + d.nz) * M + ids, kk, dim=1).values
            del S
        _ref[key] = dict(d=d, xi=xi, x=d.x.to(dev), M=M, top=top)
    return _ref[key]


def _raw(x, N, D, k, ld=None):
    """`dgmi_knn_cosine_topk_f32` on rows `x` (leading dimension `ld`) with a workspace of the test's own."""
    from dream_gnn_amd import _lib

    L = _lib.lib
    assert L.dgmi_knn_cosine_supported(N, D, k) == 1
    wb = int(L.dgmi_knn_cosine_workspace_bytes(N, D, k))
    ws = torch.empty(max(wb, 256), dtype=torch.uint8, device=x.device)
    nbr = torch.full((N, k), -7, dtype=torch.int32, device=x.device)
    ld = x.stride(0) if ld is None else ld
    assert x.stride(1) == 1 and ld >= D
    _lib.check(L.dgmi_knn_cosine_topk_f32(x.data_ptr(), ld, N, D, k, nbr.data_ptr(), ws.data_ptr(), ws.numel(),
                                          torch.cuda.current_stream().cuda_stream), "dgmi_knn_cosine_topk_f32")
    torch.cuda.synchronize()
    return nbr, ws, wb


def _readback(ws, L, N):
    f = lambda off, n, dt: ws[off:off + 4 * n].view(dt)
    return (f(L.tau, N, torch.float32), f(L.thr, N, torch.float32),
            f(L.cnt, N * (K.SPLITS + 1), torch.int32).view(N, K.SPLITS + 1).long(), f(L.flags, N, torch.int32))


@functools.lru_cache(maxsize=None)
def _region_tiles(N, k):
    """Per query: first / one-past-last tile of its 8 row regions and the tiles in front of its own (column region)."""
    L = K.screen_layout(N, 64, k)
    n_qt = L.Np // L.tile
    rng = np.array([K.emit_tile_ranges(N, k, t) for t in range(n_qt)])      # (query tiles, 8, 2)
    rng = np.minimum(rng, n_qt)                                             # (an empty split starts past the end)
    per_q = np.repeat(rng, L.tile, axis=0)[:N]
    col = np.repeat(np.arange(n_qt) * (1 if L.sym else 0), L.tile)[:N]
    return per_q[:, :, 0].copy(), per_q[:, :, 1].copy(), col


def _check(dev, d, k, nbr, ws=None, wb=None, dma=False, screen_first=False, pool_chunks=0, hollow=True):
    r = _reference(dev, d)
    N, D, nz, M, xi = d.N, d.D, d.nz, r["M"], r["xi"]
    top = r["top"]
    want_s, want_id = top[:, :k] // M - nz, M - 1 - top[:, :k] % M
    kth = want_s[:, k - 1]
    tie_cut = (top[:, k] // M - nz == kth) if k < N else torch.zeros(N, dtype=torch.bool, device=dev)
    nonzero = torch.ones(N, dtype=torch.bool, device=dev)
    nonzero[list(d.zero)] = False

    # ids first: nothing is gathered with an id that was not checked
    assert nbr.shape == (N, k) and nbr.dtype == torch.int32
    nb = nbr.long()
    assert int(nb.min()) >= 0 and int(nb.max()) < N, "ids out of range: min %d max %d" % (int(nb.min()), int(nb.max()))
    srt = nb.sort(dim=1).values
    assert bool((srt[:, 1:] != srt[:, :-1]).all()), "duplicate ids in %d lists" % int((srt[:, 1:] == srt[:, :-1]).any(1).sum())

    screen = ws is not None
    if screen:
        L = K.screen_layout(N, D, k, pool_chunks)
        assert wb == L.total
        tau, thr, cnt, flags = _readback(ws, L, N)
        caps = torch.from_numpy(K.region_caps(N, k)).to(dev)
        thr_num = thr.double() * nz
        n_tiles = L.Np // L.tile
        t_lo, t_hi, t_col = (torch.from_numpy(a).to(dev) for a in _region_tiles(N, k))
        reg = torch.zeros((N, K.SPLITS + 1), dtype=torch.int64, device=dev)
        samp_kth = torch.zeros(N, dtype=torch.int64, device=dev)
        tiles, T = K.sampled_tiles(N, D, k, screen_first)
        samp_cols = torch.cat([torch.arange(t * T, min((t + 1) * T, N)) for t in tiles]).to(dev)
    got = torch.empty((N, k), dtype=torch.int64, device=dev)
    above = torch.empty(N, dtype=torch.int64, device=dev)
    B = max(1, (1 << 26) // N)
    for lo in range(0, N, B):
        hi = min(N, lo + B)
        S = xi[lo:hi] @ xi.t()                                       # float64, integer-valued, exact
        got[lo:hi] = torch.gather(S, 1, nb[lo:hi]).long()
        above[lo:hi] = (S > kth[lo:hi, None].double()).sum(dim=1)
        if screen:
            hit = torch.cat([S >= thr_num[lo:hi, None], torch.zeros((hi - lo, L.Np - N), dtype=torch.bool, device=dev)], dim=1)
            run = torch.nn.functional.pad(hit.view(hi - lo, n_tiles, L.tile).sum(dim=2).cumsum(dim=1), (1, 0))
            reg[lo:hi, :K.SPLITS] = run.gather(1, t_hi[lo:hi]) - run.gather(1, t_lo[lo:hi])
            reg[lo:hi, K.SPLITS] = run.gather(1, t_col[lo:hi, None])[:, 0]
            if k <= 4:
                samp_kth[lo:hi] = torch.topk(S[:, samp_cols], k, dim=1).values[:, k - 1].long()
            del hit, run
        del S

    # (a)
    bad = (got != want_s).any(dim=1)
    assert not bool(bad.any()), "similarities differ from the integer top-k in %d lists, first query %d: got %s want %s" % (
        int(bad.sum()), int(bad.nonzero()[0]), got[bad][0].tolist(), want_s[bad][0].tolist())
    assert bool((got[:, 1:] <= got[:, :-1]).all())
    assert torch.equal((got > kth[:, None]).sum(dim=1), above)
    assert bool((got[nonzero, 0] == nz).all()) and not bool(got[~nonzero].any())
    if not screen:
        return None

    # (b)
    tau_num = tau.double() * nz
    assert bool((tau_num == tau_num.round()).all()) and bool((tau_num.abs() <= nz).all())
    assert bool((tau_num <= kth.double()).all()), "tau0 above the true k-th value for %d queries" % int((tau_num > kth.double()).sum())
    assert torch.equal(thr, tau - torch.tensor(0.008, dtype=torch.float32, device=dev) * 2)
    if k <= 4:
        wrong = tau_num.long() != samp_kth
        assert not bool(wrong.any()), "tau0 is not the k-th largest of the sampled tiles for %d queries, first %d: %g vs %d" % (
            int(wrong.sum()), int(wrong.nonzero()[0]), float(tau_num[wrong][0]), int(samp_kth[wrong][0]))

    # (c)
    flagged = flags != 0
    assert bool(((flags == 0) | (flags == 1)).all())
    assert torch.equal(flagged, (cnt > caps).any(dim=1))
    un = ~flagged
    assert torch.equal(cnt[un].sum(dim=1), reg[un].sum(dim=1)), "entries offered != candidates at or above the threshold"
    if dma:
        marked = cnt >= K.OVERFLOW_MARK
        assert not bool(marked[un].any())
    else:
        wrong = (cnt != reg).any(dim=1)
        assert not bool(wrong.any()), "region counts differ for %d queries, first %d: %s vs %s" % (
            int(wrong.sum()), int(wrong.nonzero()[0]), cnt[wrong][0].tolist(), reg[wrong][0].tolist())
        assert torch.equal(flagged, (reg > caps).any(dim=1))

    # (d)
    if k > 16:
        ordered = torch.ones(N, dtype=torch.bool, device=dev)
    else:
        pad = torch.cat([flagged, torch.zeros(-N % 32, dtype=torch.bool, device=dev)]).view(-1, 32).any(dim=1)
        ordered = ~pad.repeat_interleave(32)[:N]
    wrong = (nb != want_id).any(dim=1) & ordered
    assert not bool(wrong.any()), "order differs from (score desc, id asc) for %d queries, first %d: %s vs %s" % (
        int(wrong.sum()), int(wrong.nonzero()[0]), nb[wrong][0].tolist(), want_id[wrong][0].tolist())

    # (e)
    shares = dict(flagged=float(flagged.float().mean()), tie_cut=float(tie_cut.float().mean()),
                  unflagged_tie_cut=float((un & tie_cut).float().mean()), ordered_tie_cut=float((ordered & tie_cut).float().mean()),
                  fullest=int(cnt[un].sum(dim=1).max()) if bool(un.any()) else 0)
    print("N=%d D=%d k=%d%s: flagged %.3f, tie-cut %.3f, unflagged and tie-cut %.3f, order-checked and tie-cut %.3f, fullest "
          "unflagged buffer %d" % (N, D, k, " dma" if dma else "", shares["flagged"], shares["tie_cut"], shares["unflagged_tie_cut"],
                                   shares["ordered_tie_cut"], shares["fullest"]))
    if hollow:
        assert shares["unflagged_tie_cut"] >= 0.25 and shares["ordered_tie_cut"] > 0
        assert not bool(flagged[list(d.antipodal)].any())
        for z in d.zero:   # offered all N candidates (its threshold is below 0): flagged iff a region spans more ids than its cap
            rows, col = K.emit_regions(N, k, z)
            assert bool(flagged[z]) == (max(b - a for a, b in rows) > L.cap_r or col[1] > L.cap_c), z
            assert bool(flagged[z]) or k > 8    # (k <= 8: a region of 128 slots never spans fewer than 256 ids)
        lo, hi = d.block
        blk = np.arange(lo, hi)
        tl, th, tc = _region_tiles(N, k)
        inside = lambda a, b: np.clip(np.minimum(b, hi) - np.maximum(a, lo), 0, None)
        most_r = inside(tl[blk] * L.tile, th[blk] * L.tile).max(axis=1)
        most_c = inside(0, tc[blk] * L.tile)
        must = torch.from_numpy((most_r > L.cap_r) | (most_c > L.cap_c)).to(dev)
        assert bool(flagged[lo:hi][must].all())
        assert L.sym or k > 8 or bool(must.all())
    return dict(flags=flags.clone(), cnt=cnt.clone(), tau=tau.clone(), **shares)


# ---------------------------------------------------------------------------------------------------------------------
# the fp32 kernel below 1 536 rows: candidate splits + merge ((1500, 128, 13): 11 splits of 5 tiles, the last one empty;
# 97 / 33 rows: one split, a ragged tile; (16, 64, 16): k == N)
@pytest.mark.parametrize("N,D,k", K.SMALL_SHAPES)
def test_small_n_kernel_and_merge(dev, N, D, k):
    d = K.lattice(N, D)
    assert N < K.SCREEN_MIN_ROWS
    nbr, _, wb = _raw(_reference(dev, d)["x"], N, D, k)
    assert wb == K.workspace_bytes(N, D, k)
    _check(dev, d, k, nbr)


@pytest.mark.parametrize("k", [4, 16])
def test_small_n_block_of_300_copies_spans_the_splits(dev, k):
    """763 ordinary rows, 300 of them copies of one: for each of those a class of 300 at similarity 1 that spans four of
    the six candidate splits, k entries of it to be merged without a duplicate or a gap."""
    d = K.lattice(763, 256, specials=False)
    nbr, _, _ = _raw(_reference(dev, d)["x"], 763, 256, k)
    _check(dev, d, k, nbr)
    lo, hi = d.block
    inside = (nbr[lo:hi] >= lo) & (nbr[lo:hi] < hi)
    assert bool(inside.all())


# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,D,k", K.RECT_SHAPES + K.TRI_SHAPES, ids=lambda v: str(v))
def test_screen_128_rectangle_and_triangle(dev, N, D, k):
    """128 x 128 tiles: the full rectangle (1 536 and 2 085 rows: 12 tiles, and 17 with a ragged last one; D = 64 one K
    chunk, 768 the flagship width; k = 13 / 40 / 64: the wider regions, the bisection for tau, the batched rescoring of
    up to 2 085 entries) and the triangular sweep (24 741 rows at k = 4, 40 997 at k = 12 and 64: `knn_exact_rows_kernel`
    behind the flagged rows), special rows on both sides of the diagonal."""
    d = K.lattice(N, D)
    L = K.screen_layout(N, D, k)
    assert not L.big and L.sym == ((N, D, k) in K.TRI_SHAPES)
    nbr, ws, wb = _raw(_reference(dev, d)["x"], N, D, k)
    out = _check(dev, d, k, nbr, ws, wb)
    if k == 64 and L.sym:
        # queries inside the 300-block at k = 64: its first tile's rows find all 300 copies in one row region of 256 slots —
        # the exact-rows take-over (its last rows receive most of them through the column region and stay with the screen)
        lo, hi = d.block
        assert bool(out["flags"][lo:(lo // 128 + 1) * 128].all()) and not bool(out["flags"][lo:hi].all())


@pytest.mark.parametrize("N,D,k", K.BIG_SHAPES, ids=lambda v: str(v))
def test_screen_256_tiles(dev, N, D, k):
    """256 x 256 tiles from 49 152 rows (49 452: 194 tiles, 44 rows in the last): the LDS-DMA kernel with its record
    pool at D = 256, the register-staged kernel for one-chunk rows at D = 64."""
    d = K.lattice(N, D)
    assert K.screen_layout(N, D, k).big
    nbr, ws, wb = _raw(_reference(dev, d)["x"], N, D, k)
    _check(dev, d, k, nbr, ws, wb, dma=D > 64)


def test_screen_256_first_kernel_and_small_pool_agree(dev):
    """`knn_screen_first = 1`: the register-staged 256 x 256 kernel at D = 256, every region count by `emit_regions`;
    `knn_pool_chunks = 48`: a pool that runs out, the records appended directly — the same totals, flags and lists as
    with the default pool."""
    from dream_gnn_amd import _lib

    N, D, k = K.BIG_SHAPES[0]
    d = K.lattice(N, D)
    x = _reference(dev, d)["x"]
    nbr0, ws, wb = _raw(x, N, D, k)
    base = _check(dev, d, k, nbr0, ws, wb, dma=True)
    del ws
    _lib.set_tuning("knn_screen_first", 1)
    nbr1, ws, wb = _raw(x, N, D, k)
    _lib.set_tuning("knn_screen_first", 0)
    first = _check(dev, d, k, nbr1, ws, wb, screen_first=True)
    del ws
    _lib.set_tuning("knn_pool_chunks", 48)
    nbr2, ws, wb = _raw(x, N, D, k)
    _lib.set_tuning("knn_pool_chunks", 0)
    small = _check(dev, d, k, nbr2, ws, wb, dma=True, pool_chunks=48)
    assert torch.equal(small["flags"], base["flags"]) and torch.equal(small["tau"], base["tau"])
    un = base["flags"] == 0
    assert torch.equal(small["cnt"][un], base["cnt"][un])
    assert torch.equal(nbr2, nbr0)
    assert first["unflagged_tie_cut"] >= 0.25   # (it samples tile 192 too: thresholds and flags of its own)


# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,k", [(2048, 4), (4096 + 128 + 37, 40)])
def test_take_over_of_every_query_on_mostly_zero_rows(dev, N, k):
    """All rows zero except 64: a zero row's threshold is below 0 and every candidate is at or above it, so every region of
    every zero row overflows — 97 % of the answer or more comes from the take-over.  2 048 rows at k = 4: the fp32 tile kernel, whose lists
    start at -inf and whose candidates tie at 0 by the thousand.  k = 40: the exact-rows kernel, at 4 261 rows (34 tiles, 5
    per split: 640 candidates for a region of 512; at 2 048 rows a region spans 256 ids and nothing overflows)."""
    d = K.mostly_zero(N, 256)
    nbr, ws, wb = _raw(_reference(dev, d)["x"], N, 256, k)
    out = _check(dev, d, k, nbr, ws, wb, hollow=False)
    assert bool(out["flags"][list(d.zero)].all())


@pytest.mark.parametrize("N,D,k,dma", [(2048 + 37, 256, 4, False), (49152 + 300, 256, 4, True)])
def test_row_strided_input(dev, N, D, k, dma):
    """`wide[:, :D]` with ld = D + 8, through `ops.knn_cosine_topk` and through the raw call: bit-identical to the
    contiguous run, and a second run bit-identical to the first."""
    from dream_gnn_amd import ops

    d = K.lattice(N, D)
    x = _reference(dev, d)["x"]
    wide = torch.full((N, D + 8), float("nan"), device=dev)
    wide[:, :D] = x
    view = wide[:, :D]
    assert view.stride() == (D + 8, 1) and not view.is_contiguous()
    want, _, _ = _raw(x, N, D, k)
    nbr, ws, wb = _raw(view, N, D, k, ld=D + 8)
    _check(dev, d, k, nbr, ws, wb, dma=dma)
    assert torch.equal(nbr, want)
    assert torch.equal(_raw(view, N, D, k, ld=D + 8)[0], want)
    assert torch.equal(ops.knn_cosine_topk(view, k), want) and torch.equal(ops.knn_cosine_topk(x, k), want)


def test_graph_builder_on_lattice_rows(dev):
    """`graph.feature_similarity_graph(X, k, fused=True)` on a table with zero rows and duplicates: the adjacency
    `_normalized_adjacency` builds from lists that satisfy (a) — every edge (i, j) is in the integer top-k of i or of j
    (S[i, j] >= i's k-th value), every candidate strictly above a row's k-th value is an edge, the pattern is symmetric
    with a full diagonal, every row sums to 1, and indices and weights are bit for bit those `_normalized_adjacency` gives
    the search's own lists (multiplicity over the row's sum)."""
    from dream_gnn_amd import graph as G, ops

    N, D, k = 2048 + 37, 256, 4
    d = K.lattice(N, D)
    r = _reference(dev, d)
    X = r["x"] * 4.0          # un-normalised features: every norm is exactly 4 (or 0), the division exact
    nbr = ops.knn_cosine_topk(r["x"], k)
    _check(dev, d, k, nbr)    # (first: the builder is only handed ids that were checked)
    a = G.feature_similarity_graph(X, k, fused=True).coalesce()
    rows = torch.arange(N, device=dev).repeat_interleave(k)
    b = G._normalized_adjacency(rows, nbr.long().reshape(-1), N, True).coalesce()
    assert torch.equal(a.indices(), b.indices()) and torch.equal(a.values(), b.values())
    i, j = a.indices()
    M, nz = r["M"], d.nz
    kth = r["top"][:, k - 1] // M - nz
    S = (r["xi"] @ r["xi"].t()).long()
    s_ij = S[i, j]
    off = i != j
    assert bool(((s_ij >= kth[i]) | (s_ij >= kth[j]))[off].all())
    dense = torch.zeros((N, N), dtype=torch.bool, device=dev)
    dense[i, j] = True
    assert torch.equal(dense, dense.t()) and bool(dense.diagonal().all())
    assert bool(dense[S > kth[:, None]].all())
    rowsum = torch.zeros(N, dtype=torch.float64, device=dev).index_add_(0, i, a.values().double())
    assert float((rowsum - 1.0).abs().max()) <= 1e-6
