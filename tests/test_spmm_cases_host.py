"""The designed SpMM operands of _spmm_cases.py sit inside their own zero tolerance, and the host restatement of the
launch geometry says what the knob sweep of test_gpu_spmm_exact.py reaches (no GPU)."""
import itertools

import numpy as np
import pytest

import _spmm_cases as C

F = 8
VARIANTS = list(itertools.product(("unit", "vals", "mult"), (False, True), (False, True)))  # values, src_scale, dropped


def _orders_agree(oracle, dst, src, n_dst, n_src, w, ss, ds, kept, seed):
    """int64 == float64 reference == the oracle's sequential fp32 and f64 sums == fp32 sums in 20 random edge orders ==
    a pairwise tree, bit for bit."""
    X = C.features(n_src, F, seed)
    ref = C.reference(dst, src, n_dst, X, w, ss, None, kept)
    assert np.array_equal(ref.astype(np.float64) * 4, C.reference_int64(dst, src, n_dst, X, w, ss, kept).astype(np.float64))
    e = np.arange(dst.size) if kept is None else np.flatnonzero(kept)
    ip, ix, order = oracle.csr_from_coo(dst[e], src[e], n_dst)
    v = None if w is None else np.asarray(w, np.float32)[e][order]
    assert np.array_equal(oracle.spmm_csr(ip, ix, v, X, ss, None, acc="f32"), ref)
    assert np.array_equal(oracle.spmm_csr(ip, ix, v, X, ss, None, acc="f64"), ref.astype(np.float64))
    want_ds = C.reference(dst, src, n_dst, X, w, ss, ds, kept)
    assert np.array_equal(oracle.spmm_csr(ip, ix, v, X, ss, ds, acc="f32"), want_ds)
    wt = np.ones(e.size, np.float32) if w is None else np.asarray(w, np.float32)[e]
    if ss is not None:
        wt = wt * ss[src[e]]
    terms = X[src[e]] * wt[:, None]
    assert terms.dtype == np.float32
    rng = np.random.default_rng(seed)
    for _ in range(20):
        perm = rng.permutation(e.size)
        y = np.zeros((n_dst, F), np.float32)
        np.add.at(y, dst[e][perm], terms[perm])  # unbuffered: sequential fp32 adds in this order
        assert np.array_equal(y, ref)
    y = np.zeros((n_dst, F), np.float32)
    by_row = np.argsort(dst[e], kind="stable")
    bounds = np.searchsorted(dst[e][by_row], np.arange(n_dst + 1))
    for r in range(n_dst):
        a = terms[by_row[bounds[r]:bounds[r + 1]]]
        while a.shape[0] > 1:
            if a.shape[0] % 2:
                a = np.concatenate([a, np.zeros((1, F), np.float32)])
            a = a[0::2] + a[1::2]
        if a.shape[0]:
            y[r] = a[0]
    assert y.dtype == np.float32 and np.array_equal(y, ref)


@pytest.mark.parametrize("n_slices", [8, 3, 1, 64])
def test_sliced_designs_are_exact_in_every_order(oracle, n_slices):
    d = C.sliced_design(n_slices)
    for i, (kind, has_ss, dropped) in enumerate(VARIANTS):
        w = {"unit": None, "vals": d.vals, "mult": d.mult}[kind]
        _orders_agree(oracle, d.dst, d.src, d.n_dst, d.n_src, w, d.ss if has_ss else None, d.ds,
                      d.kept if dropped else None, 10 * n_slices + i)


@pytest.mark.parametrize("kind", ["light", "heavy"])
def test_split_graphs_are_exact_in_every_order(oracle, kind):
    g = C.split_graph(kind)
    for i, (w, ss, kept) in enumerate([(None, None, None), (g.vals, g.ss, None), (g.vals, g.ss, g.kept),
                                       (g.vals, None, g.kept & g.kept2), (None, g.ss, ~g.kept)]):
        _orders_agree(oracle, g.dst, g.src, g.n_dst, g.n_src, w, ss, g.ds, kept, i)
    # the transposed product: rows = sources, the gather-side scale is dst_scale (granularity 1/4)
    _orders_agree(oracle, g.src, g.dst, g.n_src, g.n_dst, g.vals, g.ds, g.ss, g.kept, 9)


def test_sliced_designs_hold_what_they_claim():
    for n_slices, n_src in C.SLICED_SHAPES.items():
        d = C.sliced_design(n_slices)
        assert (d.n_dst, d.n_src, d.seglen.shape) == (307, n_src, (n_slices, 307))
        assert all(d.n_dst % (4 * g * r) for g in (1, 2, 4, 8) for r in range(1, 64))
        assert set(C.DESIGNED_LENGTHS) <= set(d.seglen.ravel().tolist()) and d.seglen.max() >= 8 * 64 + 1
        for lpr in (8, 16, 32, 64):
            assert {lpr - 1, lpr, lpr + 1} <= set(C.DESIGNED_LENGTHS)
        deg = np.bincount(d.dst, minlength=d.n_dst)
        assert np.all(deg[list(C.EMPTY_ROWS)] == 0) and deg[-1] == 0 and deg[110] == 0 and deg.max() <= 3000
        assert 1000 <= d.dst.size <= 9000
        assert d.mult.min() == 1 and d.mult.max() == 8 and set(np.abs(d.vals)) == {1, 2, 3, 4} and (d.vals < 0).any()
        assert set(d.ss) == {0.5, 1, 2} and set(d.ds) == {0.25, 0.5, 1, 2}
        assert 0 < (~d.kept).sum() and d.dead.size == 4
    d64 = C.sliced_design(64)
    assert d64.n_src < d64.n_slices and np.all(d64.seglen[40:] == 0) and np.all(d64.seglen[:40].sum(1) > 0)  # empty trailing slices


def test_geometry_hand_computed():
    g = C.sliced_geometry(307, 128)  # 32-lane groups, 8 rows: 64 rows per block
    assert (g.lpr, g.R, g.chunks, g.workers, g.active_touchers, g.col_tiles, g.ragged_tile, g.tail_groups) == \
        (32, 8, 1, [5], [0], 1, False, [1])  # the toucher of block 0 would touch for row 24 * 64
    assert (C.pick_lpr(4), C.pick_lpr(128), C.pick_lpr(256), C.pick_lpr(344), C.pick_lpr(64)) == (8, 32, 64, 32, 16)
    g = C.sliced_geometry(307, 344, lpr=16, rows=1, chunk_rows=37, touch_lead=1)  # 16 rows per block
    assert (g.R, g.chunks, g.chunk_rows[-1], g.workers, g.col_tiles, g.ragged_tile) == (1, 9, 11, [3] * 8 + [1], 6, True)
    assert g.active_touchers == [1] * 8 + [0] and g.tail_groups == [0] * 9  # 16 < 37 rows; 16 >= 11 rows
    g = C.sliced_geometry(307, 4, lpr=8, rows=63)  # clamped to LPR - 1 = 7: 8 groups x 4 waves x 7 rows
    assert (g.R, g.workers, g.col_tiles, g.ragged_tile, g.tail_groups) == (7, [2], 1, True, [1])
    g = C.sliced_geometry(307, 128, lpr=64, rows=63, touch_lead=3)  # 252 rows per block, first touched row 756
    assert (g.R, g.workers, g.active_touchers, g.tail_groups) == (63, [2], [0], [1])
    g = C.sliced_geometry(307, 128, chunk_rows=1, touch_lead=0)
    assert (g.chunks, set(g.workers), set(g.active_touchers), set(g.tail_groups)) == (307, {1}, {0}, {1})
    g = C.sliced_geometry(3000, 128, touch_lead=-1)  # 47 blocks, 6 touchers: 24, 32 and 40 blocks in start inside
    assert (g.workers, g.active_touchers) == ([47], [3])
    s = C.split_geometry([0, 1, 16, 17, 53, 3000], 16, 4)  # 2 of 6 rows light: at least a quarter
    assert (s.has_light, s.n_virtual, s.per_row.tolist()) == (True, 1 + 2 + 4 + 188, [0, 0, 1, 2, 4, 188])
    s = C.split_geometry([0, 1, 16, 17, 53, 3000, 9, 9, 9], 16, 4)  # 2 of 9: no light path, an empty row keeps a virtual row
    assert (s.has_light, s.per_row.tolist()) == (False, [1, 1, 1, 2, 4, 188, 1, 1, 1])
    assert not C.split_geometry([1, 2, 3], 256, 24).has_light  # all light: nothing would be left for the first stage
    assert C.split_geometry([700, 3000, 256, 257], 256, 24).per_row.tolist() == [3, 12, 1, 2]


def test_knob_sweep_reaches_every_launch_shape():
    n = C.N_DST
    sweep = C.one_at_a_time(n)
    assert len(sweep) == 1 + 4 + 5 + 3 + 1 + 3 + 4 * 5 + 3 * 3 + 2 and all(set(k) == set(C.KNOBS) for k in sweep)
    cross = [k for lpr in C.knob_values(n)["sliced_lpr"] for k in C.full_cross(n, lpr)]
    assert len(cross) == 5 * 6 * 4 * 2 * 4 and len({tuple(sorted(k.items())) for k in cross}) == len(cross)
    for F, settings in ((4, sweep), (128, sweep), (344, sweep), (128, cross)):
        geo = [C.geometry_of(n, F, k) for k in settings]
        assert any(g.chunks > 1 for g in geo)
        assert any(g.chunks > 1 and g.chunk_rows[-1] < g.chunk_rows[0] for g in geo)
        assert any(g.chunks > 1 and any(g.active_touchers[1:]) for g in geo)  # a toucher of a chunk with r0 > 0
        assert any(sum(g.active_touchers) > 0 and g.chunks == 1 for g in geo)
        assert any(sum(g.tail_groups) > 0 for g in geo) and any(sum(g.tail_groups) == 0 for g in geo)
        for lpr in (8, 16, 32, 64):
            assert {1, lpr - 1} <= {g.R for g in geo if g.lpr == lpr}
        assert any(g.ragged_tile for g in geo)  # F = 128: the 64-lane groups' upper half idles
        if F > 4:
            assert any(g.col_tiles > 1 for g in geo)
    geo = [C.geometry_of(n, 344, k) for k in sweep]
    assert any(g.col_tiles > 1 and g.ragged_tile for g in geo)
    assert any(k["sliced_no_off32"] == 1 for k in sweep)
