"""The designed operands of _csr_cases.py sit inside their own zero tolerance, every designed row length and keep
pattern is really there, and the host restatement of the launch plan equals a brute-force loop and the library's buffer
sizes (no GPU)."""
import numpy as np
import pytest

import _csr_cases as C
from test_spmm_cases_host import _orders_agree  # int64 == f64 == the oracle's fp32 / f64 sums == 20 random fp32 orders == a tree


def test_plain_design_is_exact_in_every_order(oracle):
    d = C.plain_design()
    for i, (w, ss, kept) in enumerate([(None, None, None), (d.vals, None, None), (None, d.ss, None), (d.vals, d.ss, None),
                                       (None, None, d.kept), (d.vals, None, d.kept), (None, d.ss, d.kept), (d.vals, d.ss, d.kept)]):
        _orders_agree(oracle, d.dst, d.src, d.n_dst, d.n_src, w, ss, d.ds, kept, i)
    # the transposed product: rows = sources, the gather-side scale is dst_scale (granularity 1/4)
    _orders_agree(oracle, d.src, d.dst, d.n_src, d.n_dst, d.vals, d.ds, d.ss, d.kept, 9)


@pytest.mark.parametrize("kind", C.KINDS)
def test_pattern_designs_are_exact_in_every_order(oracle, kind):
    d = C.pattern_design(kind)
    _orders_agree(oracle, d.dst, d.src, d.n_dst, d.n_src, None, None, d.ds, d.kept, 1)
    _orders_agree(oracle, d.dst, d.src, d.n_dst, d.n_src, d.vals, d.ss, d.ds, d.kept, 2)
    _orders_agree(oracle, d.src, d.dst, d.n_src, d.n_dst, d.vals, d.ds, d.ss, d.kept, 3)


@pytest.mark.parametrize("chunk", C.CHUNKS)
def test_chunk_designs_are_exact_in_every_order(oracle, chunk):
    g = C.chunk_design(chunk)
    _orders_agree(oracle, g.dst, g.src, g.n_dst, g.n_src, g.vals, g.ss, g.ds, None, chunk)


def test_plain_design_holds_what_it_claims(oracle):
    d = C.plain_design()
    assert (d.n_dst, d.n_src) == (331, 200) and all(d.n_dst % p for p in range(2, 19))
    indptr, indices, _ = oracle.csr_from_coo(d.dst, d.src, d.n_dst)
    deg = np.diff(indptr)
    assert set(C.DESIGNED_LENGTHS) | set(C.BATCH_LENGTHS) <= set(deg.tolist()) and deg.max() == 3000
    for row, n in d.designed.items():
        assert deg[row] == n
    for n in (64, 128, 192):  # the last edge of a FULL batch, the first of the next, and one more
        assert {n - 1, n, n + 1} <= set(deg.tolist())
    assert np.all(deg[list(C.PLAIN_EMPTY)] == 0) and deg[-1] == 0 and deg[110] == 0
    background = np.setdiff1d(np.arange(d.n_dst), list(d.designed) + list(C.PLAIN_EMPTY))
    assert deg[background].max() <= 12 and 7000 <= d.dst.size <= 9000
    pairs = d.dst.astype(np.int64) * d.n_src + d.src
    assert np.unique(pairs).size < pairs.size  # duplicate (row, col) pairs: every copy counts
    assert set(np.abs(d.vals)) == {1, 2, 3, 4} and (d.vals < 0).any() and np.isfinite(d.vals).all()
    assert set(d.ss) == {0.5, 1, 2} and set(d.ds) == {0.25, 0.5, 1, 2}
    assert d.dead.size == 4 and np.all(np.bincount(d.src, minlength=d.n_src)[d.dead] > 0)
    assert np.all(np.bincount(d.src[d.kept], minlength=d.n_src)[d.dead] == 0)  # no surviving edge reads a dead column
    assert np.array_equal(d.kept, oracle.random_subset_mask(d.dst.size, int(d.dst.size * C.DROP_KEEP), C.DROP_SEED).astype(bool))


@pytest.mark.parametrize("kind", C.KINDS)
def test_every_keep_pattern_is_realised(oracle, kind):
    """From the mask of ``oracle.keep_mask`` and the CSR ``eid`` alone: kept edges per row and 64-edge id batch."""
    d = C.pattern_design(kind)
    E = d.dst.size
    assert d.desc.shape == (C.N_KEEP[kind], 8) and np.array_equal(d.kept, oracle.keep_mask(d.desc, E).astype(bool))
    assert 0 < d.kept.sum() < E
    indptr, indices, eid = oracle.csr_from_coo(d.dst, d.src, d.n_dst)
    kept_csr = oracle.keep_mask(d.desc, E).astype(bool)[eid]
    counts = lambda name: C.batch_counts(kept_csr, indptr, d.rows[name])
    row_mask = lambda name: kept_csr[indptr[d.rows[name]]:indptr[d.rows[name] + 1]]
    assert counts("a_first_batch_dropped") == [0, 64, 64, 1]
    assert counts("b_middle_batch_dropped") == [64, 0, 64, 1]
    assert counts("c_tail_batch_dropped") == [64, 64, 64, 0] and row_mask("c_tail_batch_dropped").size == 200
    assert counts("d_every_edge_dropped") == [0, 0, 0, 0] and row_mask("d_every_edge_dropped").size == 200
    assert counts("e_survivor_at_lane_0") == [1, 1, 1, 1]
    assert np.flatnonzero(row_mask("e_survivor_at_lane_0")).tolist() == [0, 64, 128, 192]
    assert np.flatnonzero(row_mask("e_survivor_at_lane_63")).tolist() == [63, 127, 191, 199]
    assert np.array_equal(row_mask("f_alternating"), np.arange(193) % 2 == 0)
    assert counts("g_full_batch_loses_one") == [64, 63, 64, 1] and not row_mask("g_full_batch_loses_one")[64 + 17]
    assert row_mask("h_single_dropped_edge").tolist() == [False]
    for row, want in d.want.items():
        assert np.array_equal(kept_csr[indptr[row]:indptr[row + 1]], want) and (want.size >= 193 or want.size == 1)
    # dead columns: reached, but by no surviving edge; every one of their edges sits on a dropped position of a designed row
    into_dead = np.isin(d.src, d.dead)
    assert np.all(np.bincount(d.src, minlength=d.n_src)[d.dead] > 0) and not d.kept[into_dead].any()
    assert set(d.dst[into_dead].tolist()) <= set(d.want)
    assert np.all(np.diff(indptr)[list(C.PATTERN_EMPTY)] == 0) and np.isfinite(d.vals).all()
    # the same graph under every kind: only the COO order differs
    first = C.pattern_design(C.KINDS[0])
    assert np.array_equal(np.bincount(d.dst, minlength=d.n_dst), np.bincount(first.dst, minlength=d.n_dst))


def test_descriptions_are_what_they_say(oracle):
    E = C.pattern_design("eight").dst.size
    u = {k: C.descriptions(k, E).view(np.uint32) for k in C.KINDS}
    assert sorted(C.N_KEEP.values()) == [1, 1, 2, 2, 3, 8]
    assert np.array_equal(C.descriptions("one", E)[0], oracle.random_subset_select(E, int(E * 0.7), 77))
    h = u["halves"]
    assert (h[0, 0], h[0, 1], h[1, 0], h[1, 1]) == (0, E // 2, E // 2, E)  # disjoint halves of the edge space
    n = u["nested"]
    assert (n[0, 0], n[0, 1]) == (n[1, 0], n[1, 1]) == (0, E)
    one, inv = (oracle.keep_mask(C.descriptions(k, E), E) for k in ("one", "inverted"))
    assert u["inverted"][0, 6] == 1 and np.array_equal(one + inv, np.ones(E, np.float32))
    # eight: the edges next to both ends of every hand-made word are pinned into one row, and the two words that drop
    # their range do so from edge b to edge e - 1 exactly
    d = C.pattern_design("eight")
    pinned = []
    for b, e, drops in C.hand_made(d.desc):
        assert 0 < b < e < E and e - b >= 70
        assert d.kept[[b - 1, b, e - 1, e]].tolist() == ([True, False, False, True] if drops else [True] * 4)
        assert d.kept[b:e].any() != drops
        pinned += [b - 1, b, e - 1, e]
    assert np.all(d.dst[pinned] == C.PIN_ROW) and np.flatnonzero(d.dst == C.PIN_ROW).tolist() == sorted(pinned)


def test_place_pattern_serves_wants_and_pins():
    kept = np.array([1, 0, 0, 1, 1, 0, 1, 1, 0, 1, 0, 0, 1, 1], bool)
    wants = {7: np.array([0, 1, 1, 0], bool), 2: np.array([1, 0], bool)}
    pos, rest = C.place_pattern(kept, wants, pins={9: [4, 5]})
    assert pos[9].tolist() == [4, 5]
    for row, want in wants.items():
        assert np.all(np.diff(pos[row]) > 0) and np.array_equal(kept[pos[row]], want)
    taken = np.concatenate(list(pos.values()))
    assert np.unique(taken).size == taken.size == 8 and sorted(taken.tolist() + rest.tolist()) == list(range(kept.size))
    with pytest.raises(AssertionError):
        C.place_pattern(kept, {0: np.zeros(7, bool)})  # six dropped positions only


def _plan_by_loop(indptr, chunk):
    items, long_rows, n_slots = [], [], 0
    for r in range(len(indptr) - 1):
        start, end = int(indptr[r]), int(indptr[r + 1])
        if end - start <= chunk:
            items.append((r, start, end, -1))
            continue
        slot0, s = n_slots, start
        while s < end:
            items.append((r, s, min(s + chunk, end), n_slots))
            n_slots, s = n_slots + 1, s + chunk
        long_rows.append((r, slot0, n_slots - slot0, 0))
    return items, long_rows, n_slots


def test_plan_items_equals_a_loop_and_the_library_sizes():
    from dream_gnn_amd import _lib  # loads without a GPU (test_abi.py)

    rng = np.random.default_rng(0)
    cases = [(np.concatenate([[0], np.cumsum(rng.integers(0, hi, n))]), chunk)
             for n, hi in ((1, 5), (7, 40), (40, 200), (200, 70)) for chunk in (16, 17, 64)]
    cases += [(np.concatenate([[0], np.cumsum(C.chunk_design(c).lengths)]), c) for c in C.CHUNKS]
    cases += [(np.zeros(6, np.int64), 16), (np.array([0, 16, 32, 49]), 16)]
    for indptr, chunk in cases:
        p = C.plan_items(indptr, chunk)
        items, long_rows, n_slots = _plan_by_loop(indptr, chunk)
        assert p.items.tolist() == [list(i) for i in items] and p.long_rows.reshape(-1, 4).tolist() == [list(l) for l in long_rows]
        assert p.n_slots == n_slots and p.header.tolist() == [len(items), len(long_rows), n_slots, chunk] + [0] * 12
        n_rows, nnz = len(indptr) - 1, int(indptr[-1])
        assert (p.items_cap, p.long_cap, p.slots_cap) == (n_rows + nnz // chunk, nnz // (chunk + 1), nnz // chunk + nnz // (chunk + 1))
        assert len(items) <= p.items_cap and len(long_rows) <= p.long_cap and n_slots <= p.slots_cap
        assert int(_lib.lib.dgmi_spmm_plan_bytes(n_rows, nnz, chunk)) == 4 * (C.PLAN_HEADER_WORDS + 4 * (p.items_cap + p.long_cap))
        assert int(_lib.lib.dgmi_spmm_partials_bytes(nnz, chunk, 128)) == max(16, p.slots_cap * 128 * 4)
        # every edge in exactly one item, in order
        covered = np.concatenate([np.arange(s, e) for _, s, e, _ in items]) if nnz else np.zeros(0, np.int64)
        assert np.array_equal(covered, np.arange(nnz))


@pytest.mark.parametrize("chunk", C.CHUNKS)
def test_chunk_designs_reach_every_reduce_shape(chunk):
    g = C.chunk_design(chunk)
    deg = np.bincount(g.dst, minlength=g.n_dst)
    assert np.array_equal(deg, g.lengths) and g.dst.size <= 200_000 and np.any(np.diff(g.dst) < 0)
    p = C.plan_items(np.concatenate([[0], np.cumsum(deg)]), chunk)
    nchunks = sorted(-(-n // chunk) for n in g.lengths if n > 0)
    if chunk < 65536:
        assert nchunks == sorted(C.CHUNK_COUNTS + (1,)) and sorted(p.long_rows[:, 2].tolist()) == [2, 2, 3, 8, 8, 9, 16, 17]
        assert g.lengths.tolist() != sorted(g.lengths.tolist())  # a shuffled row order
    else:
        assert sorted(g.lengths.tolist()) == [0, 1, chunk, chunk + 1] and p.long_rows[:, 2].tolist() == [2]


def test_width_list_reaches_every_lane_group_and_ragged_tiles():
    lpr = {F: C.pick_lpr(F) for F in C.VEC4_WIDTHS}
    assert set(lpr.values()) == {8, 16, 32, 64}
    assert (lpr[4], lpr[32], lpr[64], lpr[100], lpr[128], lpr[256], lpr[344], lpr[768]) == (8, 8, 16, 32, 32, 64, 32, 64)
    for F in (100, 344):  # a ragged last column tile: lanes past F in the last block of grid.y
        assert F % (4 * lpr[F]) != 0
    assert -(-344 // (4 * lpr[344])) == 3 and -(-768 // (4 * lpr[768])) == 3  # several column tiles, ragged and not
    assert all(F % 4 == 0 for F in C.VEC4_WIDTHS) and all(F % 4 for F in C.DWORD_WIDTHS)
    assert any(F > 64 and F % 64 for F in C.DWORD_WIDTHS)  # the dword kernel's own second, ragged column tile
    # the `!FULL && s * EPI >= n` break of a tail batch falls on another length for each lane-group width (a step of
    # the loop takes 8 * 64 / LPR edges: 64, 32, 16, 8): rows on both sides of each
    deg = set(C.plain_design().deg.tolist())
    for width in (8, 16, 32, 64):
        assert {width - 1, width, width + 1} <= deg
