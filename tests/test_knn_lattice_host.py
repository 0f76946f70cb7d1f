"""The lattice rows of tests/_knn_cases.py and the restated screen geometry, without a GPU: the reference of
tests/test_gpu_knn_exact.py inside its own zero tolerance.  Every element is a bf16 number and every norm exactly 1; the
similarities are the same bits as an int64 product, a float64 matmul and fp32 sums in any order; `expected_topk` is a
brute-force sort; the designs cut tie classes, reach negative neighbours and hold zero rows and one class of 300 copies;
`screen_layout` equals `dgmi_knn_cosine_workspace_bytes`; `emit_regions` equals hand-computed cases."""
import numpy as np
import pytest
import torch

import _knn_cases as K

ALL_SHAPES = K.SMALL_SHAPES + K.SCREEN_SHAPES
DESIGNS = sorted({(N, D) for N, D, _ in ALL_SHAPES})
FULL = 2048 + 37    # up to here every query row is checked; above, the special rows and 600 random ones


def _query_rows(d, n=600):
    if d.N <= FULL:
        return np.arange(d.N)
    rng = np.random.default_rng(d.N + d.D)
    return np.unique(np.concatenate([rng.choice(d.N, n, replace=False), d.antipodal, d.zero, np.arange(*d.block)[:3]]))


def _random_rows(d, rows):
    """Positions in `rows` of the randomly drawn queries (large N: the specials were added to the draw, not drawn)."""
    if d.N <= FULL:
        return np.ones(len(rows), dtype=bool)
    special = set(d.antipodal) | set(d.zero) | set(range(*d.block))
    return np.array([int(r) not in special for r in rows])


@pytest.mark.parametrize("N,D", DESIGNS)
def test_lattice_rows_are_bf16_numbers_of_norm_exactly_one(N, D):
    for d in (K.lattice(N, D),) + ((K.lattice(N, D, specials=False), K.mostly_zero(2048, 256)) if (N, D) == (763, 256) else ()):
        x = d.x
        assert x.dtype == torch.float32 and x.shape == (d.N, d.D)
        assert torch.equal(x.to(torch.bfloat16).to(torch.float32), x)
        nrm = torch.norm(x, dim=1)
        zero = torch.zeros(d.N, dtype=torch.bool)
        zero[list(d.zero)] = True
        assert bool((nrm[~zero] == 1.0).all()) and bool((nrm[zero] == 0.0).all())
        assert bool(((x != 0).sum(dim=1)[~zero] == d.nz).all())
        assert np.array_equal(d.num.astype(np.float32) * np.float32(d.nz ** -0.5), x.numpy())
        lo, hi = d.block
        assert hi == lo or bool((x[lo:hi] == x[lo]).all())
        assert hi == lo or d.N < 700 or (hi - lo == 300 and lo // 256 != (hi - 1) // 256 and lo // 128 != (hi - 1) // 128)
        for a, b in d.pairs:
            assert bool((x[a] == x[b]).all()) and float(nrm[a]) == 1.0


@pytest.mark.parametrize("N,D", DESIGNS)
def test_similarities_are_the_same_bits_in_every_format_and_order(N, D):
    """int64 product == float64 `@` == fp32 sums of the products in 20 random element orders == an fp32 pairwise tree, for
    the special rows and 40 random ones against each other."""
    d = K.lattice(N, D)
    rng = np.random.default_rng(N * 7 + D)
    rows = np.unique(np.concatenate([rng.choice(N, min(40, N), replace=False), d.antipodal, d.zero, d.block[:1],
                                     [p[1] for p in d.pairs]]).astype(np.int64))
    want = d.num[rows].astype(np.int64) @ d.num[rows].astype(np.int64).T
    assert np.array_equal(K.similarity_numerators(d.num, rows)[:, rows], want)
    x = d.x[rows]
    assert np.array_equal((x.double() @ x.double().t()).numpy() * d.nz, want.astype(np.float64))
    assert np.array_equal((x @ x.t()).numpy() * np.float32(d.nz), want.astype(np.float32))
    prod = (x[:, None, :] * x[None, :, :]).numpy()            # fp32 products, exact (powers of two)
    assert prod.dtype == np.float32
    for _ in range(20):
        run = np.zeros(prod.shape[:2], dtype=np.float32)
        for c in rng.permutation(D):
            run = run + prod[:, :, c]                         # sequential fp32 adds in a random element order
        assert np.array_equal(run * np.float32(d.nz), want.astype(np.float32))
    tree = prod
    while tree.shape[2] > 1:                                  # (D is a power of two times 3: halves while even, then a fold)
        if tree.shape[2] % 2:
            tree = np.concatenate([tree[:, :, :1] + tree[:, :, 1:2], tree[:, :, 2:]], axis=2)
        else:
            tree = tree[:, :, 0::2] + tree[:, :, 1::2]
        assert tree.dtype == np.float32
    assert np.array_equal(tree[:, :, 0] * np.float32(d.nz), want.astype(np.float32))


def test_expected_topk_is_a_brute_force_sort_on_tuple_keys():
    rng = np.random.default_rng(4)
    for N, D, k in ((16, 64, 16), (97, 64, 13), (763, 256, 4), (2085, 256, 64)):
        d = K.lattice(N, D)
        rows = rng.choice(N, min(24, N), replace=False)
        S = K.similarity_numerators(d.num, rows)
        got = K.expected_topk(S, k)
        for i in range(len(rows)):
            want = sorted(range(N), key=lambda c: (-int(S[i, c]), c))[:k]
            assert got[i].tolist() == want
    S = rng.integers(-3, 4, (50, 40))                         # few levels: every row is mostly ties
    got = K.expected_topk(S, 7)
    assert all(got[i].tolist() == sorted(range(40), key=lambda c: (-int(S[i, c]), c))[:7] for i in range(50))


@pytest.mark.parametrize("N,D,k", ALL_SHAPES)
def test_designs_do_what_they_claim(N, D, k):
    """Tie-cut share >= 50 % at the shapes meant for the screen (N >= 1536) and at the small-N kernel's N >= 763; the
    antipodal rows' k-th neighbour is negative from k = 13 (D >= 128); zero rows have similarity 0 to everything; the block is one
    class of its size at similarity 1 for each of its rows."""
    d = K.lattice(N, D)
    rows = _query_rows(d)
    at = {int(r): i for i, r in enumerate(rows)}
    S = K.similarity_numerators(d.num, rows)
    assert S.min() >= -d.nz and S.max() == d.nz
    srt = -np.sort(-S, axis=1)
    if k < N:
        cut = (srt[:, k - 1] == srt[:, k])[_random_rows(d, rows)]
        print("N=%d D=%d k=%d: tie-cut share %.3f, %d levels" % (N, D, k, cut.mean(), len(np.unique(S))))
        assert N < 763 or cut.mean() >= 0.5
    for a in d.antipodal:
        assert S[at[a], a] == d.nz
        if k >= 13 and d.nz == 64:      # (nz = 16: the random part of 12 columns reaches the anchors' 4, no claim)
            assert srt[at[a], k - 1] < 0
    for z in d.zero:
        assert not S[at[z]].any()
    lo, hi = d.block
    for b in [r for r in range(lo, hi) if r in at][:3]:
        same = np.nonzero(S[at[b]] == d.nz)[0]
        assert same.tolist() == list(range(lo, hi))
    for a, b in d.pairs:
        assert np.nonzero(S[at[a]] == d.nz)[0].tolist() == sorted((a, b)) if a in at else True


def test_antipodal_row_reaches_zero_rows_then_negative_members():
    """N = 2048, D = 256: an antipodal row's sorted similarities x 64 start with itself, the other two antipodal rows
    (1/4 + a random part), the five zero rows, then negative members: k = 4 cuts the zero-row class, k = 13 and k = 40 end
    on a negative similarity."""
    d = K.lattice(2048, 256)
    S = K.similarity_numerators(d.num, list(d.antipodal))
    for i in range(3):
        s = -np.sort(-S[i])
        assert s[0] == 64 and (s[1:3] > 0).all() and not s[3:8].any() and (s[8:] < 0).all()
        assert s[3] == s[4] and s[12] < 0 and s[39] < 0


def test_mostly_zero_and_block_only_designs():
    d = K.mostly_zero(2048, 256)
    assert len(d.zero) == 2048 - 64 and int((d.num != 0).any(axis=1).sum()) == 64
    S = K.similarity_numerators(d.num)
    assert not S[list(d.zero)].any() and (np.diag(S)[(d.num != 0).any(axis=1)] == 64).all()
    b = K.lattice(763, 256, specials=False)
    assert b.antipodal == () and b.zero == () and b.pairs == () and b.block == (106, 406)
    # the fp32 kernel splits 763 rows' candidates into 6 ranges of 4 x 32: the block's class of 300 spans four of them
    s, per = K.knn_splits(763)
    assert (s, per) == (6, 4) and len({c // (32 * per) for c in range(*b.block)}) == 4
    # 1500 rows: 47 candidate tiles, 11 splits of 5 — split 10 starts at tile 50, past the end
    s, per = K.knn_splits(1500)
    assert (s, per) == (11, 5) and (s - 1) * per >= (1500 + 31) // 32
    assert [K.knn_splits(n)[0] for n in (16, 33, 97)] == [1, 1, 1] and K.knn_splits(1535) == (11, 5)


def _lib():
    from dream_gnn_amd import _lib as L
    return L


def test_screen_layout_by_hand():
    L = K.screen_layout(2048, 256, 4)
    assert (L.big, L.sym, L.tile, L.Np, L.Dp, L.cap_r, L.cap_c, L.pool_chunks) == (False, False, 128, 2048, 256, 128, 0, 0)
    L = K.screen_layout(2085, 256, 4)   # sizes 1 114 112 / 2 135 040 / 8 340 -> 8 448 / 8 704 / 75 060 -> 75 264 / 17 080 320 / 8 448
    assert (L.Np, L.xb, L.part, L.tau, L.thr, L.cnt, L.buf, L.flags, L.pool, L.pool_ctl, L.total) == (
        2176, 0, 1114112, 3249152, 3257600, 3266304, 3341568, 20421888, 20430336, 20430336, 20430336)
    assert K.screen_layout(24704, 256, 4)[:8] == (False, True, 128, 24704, 256, 128, 1024, 0)
    assert K.screen_layout(24704, 200, 12)[:8] == (False, False, 128, 24704, 256, 256, 0, 0)
    assert K.screen_layout(3000, 64, 64)[:8] == (False, False, 128, 3072, 64, 512, 0, 0)
    assert K.screen_layout(41000, 72, 40)[:8] == (False, True, 128, 41088, 128, 256, 2048, 0)
    assert K.screen_layout(49452, 200, 4)[:8] == (True, True, 256, 49664, 256, 128, 1024, 37089 + 2048)
    assert K.default_pool_chunks(49452, 4) == (49452 * 192 + 255) // 256 + 2048
    assert K.screen_layout(49452, 200, 4, pool_chunks=48).pool_chunks == 48 and K.screen_layout(2048, 64, 4, pool_chunks=48).pool_chunks == 0
    for N, D, k in K.SCREEN_SHAPES:
        L = K.screen_layout(N, D, k)
        assert all(o % 256 == 0 for o in L[8:]) and L.Np % L.tile == 0 and 0 <= L.Np - N < L.tile


def test_screen_layout_total_is_the_library_workspace_size():
    lib = _lib()
    rng = np.random.default_rng(50)
    shapes = list(ALL_SHAPES) + [(2048, 256, 4), (2048, 256, 40), (24704, 256, 4)]
    while len(shapes) < len(ALL_SHAPES) + 53:
        k = int(rng.integers(1, 65))
        N = int(rng.choice([rng.integers(1536, 3000), rng.integers(20000, 50000), rng.integers(49000, 130000)]))
        D = 8 * int(rng.integers(1, 113 if k <= 16 else 129))
        shapes.append((N, D, k))
    for N, D, k in shapes:
        assert lib.lib.dgmi_knn_cosine_supported(N, D, k) == 1, (N, D, k)
        assert lib.lib.dgmi_knn_cosine_workspace_bytes(N, D, k) == K.workspace_bytes(N, D, k), (N, D, k)
    lib.set_tuning("knn_pool_chunks", 48)
    try:
        for N, D, k in K.BIG_SHAPES + [(2048, 256, 4)]:
            assert lib.lib.dgmi_knn_cosine_workspace_bytes(N, D, k) == K.workspace_bytes(N, D, k, pool_chunks=48)
            assert K.workspace_bytes(N, D, k, pool_chunks=48) < K.workspace_bytes(N, D, k) or N < 49152
    finally:
        lib.set_tuning("knn_pool_chunks", 0)


def test_emit_regions_by_hand():
    # N = 2048: 16 tiles of 128, full rectangle: 2 tiles per split whatever the query, no column region
    for q in (0, 700, 2047):
        assert K.emit_regions(2048, 4, q) == ([(256 * s, 256 * s + 256) for s in range(8)], (0, 0))
    # k = 40 at 2048 rows: the same sweep (only the caps differ)
    assert K.emit_regions(2048, 40, 5) == K.emit_regions(2048, 4, 5)
    # N = 24704, k = 4: 193 tiles, triangular.  Query tile 0: ceil(193 / 8) = 25 tiles per split, the last split 18
    rows, col = K.emit_regions(24704, 4, 17)
    assert rows == [(3200 * s, 3200 * s + 3200) for s in range(7)] + [(22400, 24704)] and col == (0, 0)
    # query 150 * 128 + 70: 43 tiles from the diagonal on, 6 per split, the last split the one tile 192; everything in
    # front of tile 150 arrives through the column region
    rows, col = K.emit_regions(24704, 4, 150 * 128 + 70)
    assert rows == [(19200 + 768 * s, 19200 + 768 * s + 768) for s in range(7)] + [(24576, 24704)] and col == (0, 19200)
    # the last query tile: one tile for split 0, nothing for the others
    rows, col = K.emit_regions(24704, 4, 24703)
    assert rows == [(24576, 24704)] + [(24704, 24704)] * 7 and col == (0, 24576)
    # k = 12: the triangular sweep starts at 40 960 rows only
    assert K.emit_regions(24704, 12, 24703)[1] == (0, 0)
    # a ragged last tile: N = 24741 = 193 tiles + 37 rows -> 194 tiles, query tile 193 holds 37 candidates
    rows, col = K.emit_regions(24741, 4, 24740)
    assert rows[0] == (24704, 24741) and col == (0, 24704)
    assert K.emit_tile_ranges(24741, 4, 0) == [(25 * s, 25 * s + 25) for s in range(7)] + [(175, 194)]
    # every candidate falls into exactly one region of every query
    for N, k in ((2085, 4), (24741, 4), (49452, 12)):
        for q in (0, N // 3, N - 1):
            rows, col = K.emit_regions(N, k, q)
            ids = sorted([col] + rows)
            assert ids[0][0] == 0 and ids[-1][1] == N or col == (0, 0)
            covered = sum(hi - lo for lo, hi in rows) + col[1] - col[0]
            assert covered == N


def test_sampled_tiles_by_hand():
    assert K.sampled_tiles(1536, 256, 4) == (list(range(12)), 128)                 # fewer than 16 tiles: all
    assert K.sampled_tiles(2085, 256, 4) == (list(range(0, 17, 2)), 128)           # 17 tiles: every second
    assert K.sampled_tiles(24741, 256, 4) == (list(range(0, 194, 8)), 128)
    assert K.sampled_tiles(49452, 64, 4) == (list(range(0, 194, 8)), 256)          # register-staged kernel: 25 tiles
    assert K.sampled_tiles(49452, 256, 4) == (list(range(0, 192, 8)), 256)         # LDS-DMA kernel: 3 per split, tile 192 left out
    assert K.sampled_tiles(49452, 256, 4, screen_first=True) == (list(range(0, 194, 8)), 256)
    assert K.sampled_tiles(49452, 256, 40) == (list(range(0, 192, 4)), 256)        # k > 16 from 128 tiles: every fourth, 6 per split


@pytest.mark.parametrize("N,D,k", [s for s in K.SCREEN_SHAPES if s[2] <= 4])
def test_a_quarter_of_the_queries_is_tie_cut_and_screened(N, D, k):
    """The GPU test's floor, on the host: with the emission threshold of the sample pass (k <= 4: the exact k-th largest
    over the sampled tiles, minus 2 eps) no region of these queries overflows, and the k-th boundary cuts a tie class.  Up
    to 2 085 rows also with the most pessimistic threshold any sample could return (the k-th largest inside tile 0)."""
    d = K.lattice(N, D)
    rows = _query_rows(d)
    rnd = _random_rows(d, rows)
    at = {int(r): i for i, r in enumerate(rows)}
    S = K.similarity_numerators(d.num, rows)
    srt = -np.sort(-S, axis=1)
    cut = srt[:, k - 1] == srt[:, k]
    caps = K.region_caps(N, k)
    L = K.screen_layout(N, D, k)
    kth, thr = K.sample_threshold(S, N, D, k, d.nz)
    assert (kth <= srt[:, k - 1]).all()
    cnt = K.region_counts(S, rows, thr, N, k)
    ok = (cnt <= caps).all(axis=1)
    share = (ok & cut)[rnd].mean()
    msg = "N=%d D=%d k=%d: sampled threshold: unflagged and tie-cut %.3f, fullest unflagged buffer %d" % (N, D, k, share, cnt.sum(axis=1)[ok].max())
    assert share >= 0.25
    assert all(ok[at[a]] for a in d.antipodal) and not any(ok[at[z]] for z in d.zero)
    assert not any(ok[at[b]] for b in range(*d.block) if b in at)
    if N <= FULL:
        cnt_p = K.region_counts(S, rows, K.pessimistic_threshold(S, k, d.nz, L.tile), N, k)
        ok_p = (cnt_p <= caps).all(axis=1)
        msg += "; tile-0 threshold: %.3f, fullest %d" % ((ok_p & cut).mean(), cnt_p.sum(axis=1)[ok_p].max())
        assert (ok_p & cut).mean() >= 0.25
        assert not any(ok_p[at[z]] for z in d.zero) and not any(ok_p[b] for b in range(*d.block))
    print(msg)
