"""The layout builders' designed inputs on the host (no GPU): the restated geometry of ``_layout_cases.py`` against hand
computation and the library's own size queries, the designs against what they claim, the numpy expectations against the
oracle and ``sorted()``, and the shapes that ``dgmi_csr_sliced_from_csr_i32`` refuses."""
import ctypes

import numpy as np
import pytest

import _layout_cases as LC
from oracle import oracle as O

# (n_rows, n_cols) and E of tests/test_gpu_layout_exact.py
GPU_ROWS = (2, 3, 512, 513, 2 ** 17 + 1, 2 ** 18 + 1, 2 ** 20, 1024, 2 ** 19, 100_000, 2_100_000)
GPU_E = (0, 1, 2, 63, 64, 65, 511, 512, 513, 8191, 8192, 8193, 16_384, 65_536, 65_537, 73_729, 20_000, 2 ** 18 - 1, 2 ** 18,
         2 ** 18 + 3, 8_388_609)
GPU_SLICES = (8, 3, 1, 64)


def test_sort_passes_by_hand_and_for_the_gpu_shapes():
    assert LC.sort_passes(0, 1) == [(0, 1)] and LC.sort_passes(0, 9) == [(0, 9)]
    assert LC.sort_passes(0, 10) == [(0, 5), (5, 5)] and LC.sort_passes(0, 18) == [(0, 9), (9, 9)]
    assert LC.sort_passes(0, 19) == [(0, 7), (7, 6), (13, 6)]
    assert LC.sort_passes(0, 28) == [(0, 7), (7, 7), (14, 7), (21, 7)]
    assert LC.sort_passes(17, 3) == [(17, 3)] and LC.sort_passes(0, 0) == [(0, 1)]
    assert [LC.bits_for(n) for n in (0, 1, 2, 3, 4, 5, 512, 513, 2 ** 20, 2 ** 20 + 1)] == [1, 1, 1, 2, 2, 3, 9, 10, 20, 21]
    assert [LC.bits_for(n) for n in GPU_ROWS[:7]] == [1, 2, 9, 10, 18, 19, 20]
    assert LC.bits_for(64 * 2_100_000) == 28 and len(LC.sort_passes(0, 28)) == 4
    for n in GPU_ROWS:
        for s in (1,) + GPU_SLICES:
            plan = LC.sort_passes(0, LC.bits_for(n * s))
            assert sum(b for _, b in plan) == LC.bits_for(n * s) and all(1 <= b <= 9 for _, b in plan)
            assert [sh for sh, _ in plan] == list(np.cumsum([0] + [b for _, b in plan[:-1]]))
            assert sorted((b for _, b in plan), reverse=True) == [b for _, b in plan]


def test_xcd_tile_order_is_a_permutation_with_idle_blocks():
    for n in list(range(1, 71)) + [1025]:
        order = LC.xcd_tile_order(n)
        assert len(order) == 8 * -(-n // 8)
        assert sorted(t for t in order if t >= 0) == list(range(n))
    order = LC.xcd_tile_order(9)  # per_xcd = 2: XCD x works through tiles 2x, 2x + 1
    assert order == [0, 2, 4, 6, 8, -1, -1, -1, 1, 3, 5, 7, -1, -1, -1, -1] and order.count(-1) == 7
    assert LC.sort_tiles(65_537) == 9 and LC.sort_tiles(8_388_609) == 1025 and LC.sort_tiles(8192) == 1
    assert LC.sort_tiles(8_388_609) > LC.SCAN_CHUNK  # the second chunk of sort_bucket_scan_kernel


def _queries():
    from dream_gnn_amd import _lib

    L, need = _lib.lib, ctypes.c_size_t(0)

    def csr(E, n_rows):
        assert L.dgmi_csr_from_coo_i32(None, None, E, n_rows, 7, None, None, None, None, ctypes.byref(need), None) == 0
        return need.value

    def coo(E, n_rows, s):
        assert L.dgmi_csr_sliced_from_coo_i32(None, None, E, n_rows, 7, s, None, None, None, None, ctypes.byref(need), None) == 0
        return need.value

    def from_csr(E, n_rows, s):
        st = L.dgmi_csr_sliced_from_csr_i32(None, None, None, E, n_rows, 7, s, None, None, None, None, ctypes.byref(need), None)
        return need.value if st == 0 else st

    return csr, coo, from_csr, L.dgmi_compact_layout_workspace_bytes


def test_restated_workspace_totals_equal_the_size_queries():
    csr, coo, from_csr, compact = _queries()
    rng = np.random.default_rng(5)
    shapes = [(E, n, s) for E in GPU_E for n in (2, 513, 2 ** 18 + 1, 2_100_000) for s in GPU_SLICES]
    shapes += [(int(rng.integers(0, 3_000_000)), int(rng.integers(1, 4_000_000)), int(rng.integers(1, 65))) for _ in range(50)]
    for E, n, s in shapes:
        assert csr(E, n) == LC.csr_from_coo_workspace(E, n), (E, n)
        assert coo(E, n, s) == LC.sliced_from_coo_workspace(E, n, s), (E, n, s)
        assert from_csr(E, n, s) == LC.sliced_from_csr_workspace(E, s), (E, n, s)
    for nnz in [1, 63, 64, 65, 4095, 4096, 4097, 12_289, LC.BIG_NNZ] + [int(x) for x in rng.integers(0, 50_000_000, 50)]:
        assert compact(nnz) == LC.compact_workspace_bytes(nnz), nnz
    g = LC.compact_geometry(LC.BIG_NNZ)
    assert g["tiles"] == 8193 and g["sweeps"] == 2 and LC.compact_geometry(LC.BIG_NNZ - 1)["sweeps"] == 1
    assert LC.compact_geometry(4097) == dict(tiles=2, words=128, sweeps=1, partial_last_word=True)
    assert [LC.word_owner(w) for w in (0, 1, 3, 4, 63, 64, 69)] == [(0, 0), (0, 1), (0, 3), (1, 0), (15, 3), (0, 0), (1, 1)]


def test_the_refused_and_the_nearest_admitted_shapes():
    """`dgmi_csr_sliced_from_csr_i32` refuses a shape whose (slice << row_bits) | row key needs 32 bits; the COO builder,
    whose key is slice * n_rows + row, takes the same shapes."""
    csr, coo, from_csr, _ = _queries()
    for s, n in ((33, 2 ** 25 + 1), (5, 2 ** 28 + 1), (3, 2 ** 29 + 1)):
        assert n * s < 2 ** 31 - 1 and not LC.sliced_from_csr_admits(n, s)
        assert from_csr(1000, n, s) == -2 and from_csr(0, n, s) == -2
        assert coo(1000, n, s) == LC.sliced_from_coo_workspace(1000, n, s)
    for s, n in ((32, 2 ** 25 + 1), (33, 2 ** 25), (4, 2 ** 28 + 1), (5, 2 ** 28), (2, 2 ** 29 + 1), (3, 2 ** 29)):
        assert LC.sliced_from_csr_admits(n, s)
        assert from_csr(1000, n, s) == LC.sliced_from_csr_workspace(1000, s)
    for n in GPU_ROWS:
        for s in GPU_SLICES:
            assert LC.sliced_from_csr_admits(n, s)


def _ballot_masks(rows, rnd):
    chunk = rows[rnd * 64:(rnd + 1) * 64]
    return {int(v): sum(1 << int(l) for l in np.flatnonzero(chunk == v)) for v in np.unique(chunk)}


@pytest.mark.parametrize("n_rows", [2, 3, 513, 2 ** 18 + 1, 2 ** 20])
def test_lane_edges_rounds_have_the_stated_ballot_masks(n_rows):
    E = 8193
    rows = LC.design_rows("lane_edges", E, n_rows)
    a, b = LC.lane_edge_rows(n_rows)
    assert a != b and a < n_rows
    for shift, bits in LC.sort_passes(0, LC.bits_for(n_rows)):  # the two rows differ in every pass's digit
        assert (a >> shift) & ((1 << bits) - 1) != (b >> shift) & ((1 << bits) - 1)
    full = (1 << 64) - 1
    seen = set()
    for rnd in range(E // 64):
        m = _ballot_masks(rows, rnd)
        want_b = (1, 1 << 63, 1 | 1 << 63)[rnd % 3]
        assert m == {b: want_b, a: full ^ want_b}
        seen.add(want_b)
    assert seen == {1, 1 << 63, 1 | 1 << 63}
    assert _ballot_masks(rows, E // 64) == {b: 1}  # the tile of one record


def test_round_robin_gives_every_lane_its_own_digit_or_alternates():
    r = LC.design_rows("round_robin", 8193, 512)
    assert all(np.unique(r[k * 64:(k + 1) * 64]).size == 64 for k in range(128))
    r = LC.design_rows("round_robin", 8193, 2)
    assert _ballot_masks(r, 5) == {0: int("01" * 32, 2), 1: int("10" * 32, 2)}


@pytest.mark.parametrize("n_rows", [1024, 2 ** 19, 2 ** 20])
def test_one_digit_per_pass_takes_every_digit_value(n_rows):
    plan = LC.sort_passes(0, LC.bits_for(n_rows))
    assert len(plan) == {1024: 2, 2 ** 19: 3, 2 ** 20: 3}[n_rows]
    for p in range(len(plan)):
        rows = LC.design_rows("one_digit", 8193, n_rows, p).astype(np.int64)
        for q, (shift, bits) in enumerate(plan):
            dig = (rows >> shift) & ((1 << bits) - 1)
            if q == p:
                assert np.array_equal(np.unique(dig), np.arange(1 << bits))  # extremes 0 and 2^bits - 1 included
                assert np.any(np.diff(dig) < 0)
            else:
                assert np.all(dig == 1)


def test_wave_carry_digit_occurs_once_per_round():
    for n_rows in (513, 2 ** 18 + 1):
        E = 65_537
        rows = LC.design_rows("wave_carry", E, n_rows)
        s = LC.wave_carry_row(n_rows)
        per_round = np.add.reduceat((rows == s).astype(np.int64), np.arange(0, E, 64))
        assert np.all(per_round[:-1] == 1)  # every full round: hence 8 per wave, 128 per tile, in every tile
        assert np.unique(np.flatnonzero(rows == s) % 64).size == 64  # at every lane


@pytest.mark.parametrize("first,last_gap,e_mod", [(0, 0, 63), (64, 64, 0), (70, 65, 63), (0, 300, 0)])
def test_gap_design_holds_every_listed_gap(first, last_gap, e_mod):
    n_rows = 100_000
    rows = LC.gap_design(n_rows, first, last_gap, e_mod)
    E = rows.size
    assert (E + 1) % 64 == (0 if e_mod == 63 else 1)
    srt = np.sort(rows)
    assert srt[0] == first and srt[-1] == n_rows - 1 - last_gap and np.unique(rows).size == E and not np.array_equal(srt, rows)
    assert set(LC.GAP_DIFFS + (LC.GAP_HUGE,)) <= set(np.diff(srt).tolist())
    prev, cur = LC.boundary_gaps(srt, n_rows)
    kinds = np.array([LC.fill_kind(a, b) == "wave" for a, b in zip(prev, cur)])
    assert LC.fill_kind(0, 64) == "lane" and LC.fill_kind(0, 65) == "wave" and LC.fill_kind(-1, 63) == "lane"
    assert kinds[0] == (first > 63) and kinds[E] == (last_gap > 63)  # a long gap at p = 0 / at p = E
    windows = [kinds[w:w + 64] for w in range(0, E + 1 - 63, 64)]
    assert any(k[0] and k[63] and k.sum() >= 3 for k in windows)  # the ballot loop: several long gaps, lanes 0 and 63
    lanes_long = {int(p) % 64 for p in np.flatnonzero(kinds)}
    assert lanes_long == set(range(64))
    for n_slices in (8, 3, 1):
        c = LC.gap_columns(E, 50_000, n_slices)
        width = -(-50_000 // n_slices)
        sl = np.unique(c // width)
        if n_slices > 1:
            assert sl.min() >= 1 and sl.max() <= n_slices - 2  # an empty leading slice, empty trailing slices
        assert c.min() >= 0 and c.max() < 50_000


def test_chunk_design_realises_every_combination():
    indptr, combos = LC.chunk_design()
    E = int(indptr[-1])
    assert E == 2 ** 18 + 3 and indptr[1] == 0 and np.all(np.diff(indptr[-6:]) == 0)  # empty first row, empty last rows
    lens = np.diff(indptr)
    assert len(combos) == 64
    for (o, k), row in combos.items():
        assert lens[row] > 0 and (indptr[row + 1] - 1) % 8 == o
        assert np.all(lens[row + 1:row + 1 + k] == 0) and lens[row + 1 + k] > 0
    ch = LC.position_chunks(indptr, E)
    assert ch.ppt == 8 and np.array_equal(ch.row, LC.rows_of(indptr))
    ev = {p: (off, stepped, searched) for p, off, stepped, searched in ch.events}
    for (o, k), row in combos.items():
        nxt = int(indptr[row + 1])  # the first position after the row
        if o == 7:
            assert nxt % 8 == 0 and nxt not in ev  # the next chunk starts exactly on a row start: its own search
        else:
            assert ev[nxt] == (o + 1, k + 1, k >= 4)  # walked up to 4 steps, searched beyond
    r100 = int(np.flatnonzero(lens == 100)[0])
    assert indptr[r100] % 8 == 3 and any(indptr[r100] <= p0 and p0 + 8 <= indptr[r100 + 1] for p0 in range(0, E, 8))
    assert not any(indptr[r100] < p < indptr[r100 + 1] for p in ev)
    for E2 in (2 ** 18 - 1, 2 ** 18):
        ip2 = LC.chunk_prefix(indptr, E2)
        ch2 = LC.position_chunks(ip2, E2)
        assert ch2.ppt == (1 if E2 < 2 ** 18 else 8) and np.array_equal(ch2.row, LC.rows_of(ip2))
        assert ip2[-1] == E2 and (ch2.events == [] if ch2.ppt == 1 else len(ch2.events) > 56)


def test_position_chunks_equals_searchsorted_on_random_layouts():
    rng = np.random.default_rng(3)
    for _ in range(30):
        n_rows = int(rng.integers(1, 400))
        lens = rng.integers(0, 9, n_rows) * (rng.random(n_rows) < 0.4)
        indptr = np.concatenate([[0], np.cumsum(lens)])
        E = int(indptr[-1])
        want = LC.rows_of(indptr)
        for ppt_e in (E,):
            assert np.array_equal(LC.position_chunks(indptr, E).row, want)
        # the 8-position walk on the same layout (the threshold only picks the template)
        old, LC.PPT_MIN_EDGES = LC.PPT_MIN_EDGES, 0
        try:
            assert np.array_equal(LC.position_chunks(indptr, E).row, want)
        finally:
            LC.PPT_MIN_EDGES = old


@pytest.mark.parametrize("nnz", [1, 63, 64, 65, 4095, 4096, 4097, 12_289])
def test_word_design_realises_every_word_and_probe(nnz):
    full = None
    for kind in LC.TABLE_KINDS:
        d = LC.word_design(nnz, kind)
        assert d.table.shape[0] == {"one": 1, "two": 2, "three": 3, "inverted": 1}[kind] and (d.table[0, 6] == 1) == (kind == "inverted")
        assert d.eid.min() >= 0 and d.eid.max() < d.n_ids
        assert np.array_equal(O.keep_mask(d.table, d.n_ids).astype(bool)[d.eid], d.mask)
        full = d.mask if full is None else full
        assert np.array_equal(full, d.mask)  # the same target bits under every table
        # the numpy expectation == the oracle's restatement of the kernel
        p, i, v = O.compact_layout(d.ptr, d.indices, d.vals.view(np.int32), d.eid, d.table)
        assert np.array_equal(p, d.want_ptr) and np.array_equal(i, d.want_indices)
        assert np.array_equal(v, d.want_vals.view(np.int32)) and d.nk == d.mask.sum()
    d = LC.word_design(nnz)
    words = [d.mask[w:w + 64] for w in range(0, nnz, 64)]
    got = {LC.word_kind_of(w, nnz) for w in range(len(words))}
    if nnz >= 4095:
        assert got == set(LC.WORD_KINDS)
    for w, m in enumerate(words):
        kind = LC.word_kind_of(w, nnz)
        n = m.size
        want = {"kept": np.ones(n, bool), "dropped": np.zeros(n, bool), "bit0": np.arange(n) == 0, "bit63": np.arange(n) == 63,
                "inner": (np.arange(n) > 0) & (np.arange(n) < 63), "alternating": np.arange(n) % 2 == 0}.get(kind)
        assert want is None or np.array_equal(m, want)
    if nnz == 12_289:
        assert not d.mask[4096:8192].any() and d.mask[8192:12_288].all() and LC.compact_geometry(nnz)["tiles"] == 4
        assert {LC.word_owner(w) for w in range(64)} == {(j, wv) for j in range(16) for wv in range(4)}
    assert LC.compact_geometry(nnz)["partial_last_word"] == (nnz % 64 != 0)
    ptr = d.ptr.tolist()
    assert ptr == sorted(ptr) and ptr[0] == 0 and ptr[-1] == nnz and len(set(ptr)) < len(ptr)
    for t in range(1, -(-nnz // 4096) + 1):
        assert {q for q in (t * 4096 - 1, t * 4096, t * 4096 + 1) if q <= nnz} <= set(ptr)
    assert {q for q in (63, 64, 65, 127, 128, 129) if q <= nnz} <= set(ptr)
    assert sum(np.isnan(d.vals)) > 0 or nnz < 3
    if nnz >= 64:
        bits = set(d.vals.view(np.uint32)[0::3].tolist())
        assert set(LC.SPECIAL_VALUE_BITS) <= bits


def test_compaction_expectation_is_the_layout_of_the_kept_edge_list():
    """Where the layout is a real CSR (eid a permutation), ``indices[mask]`` and the ranked pointers are the CSR of the
    kept edges."""
    rng = np.random.default_rng(11)
    for E, n_rows in ((4097, 50), (700, 900)):
        dst, src = rng.integers(0, n_rows, E).astype(np.int32), LC.columns(E, 77)
        ip, ix, ei = O.csr_from_coo(dst, src, n_rows)
        for kind in LC.TABLE_KINDS:
            table = LC.keep_tables(kind, E)
            mask = O.keep_mask(table, E).astype(bool)
            m = mask[ei]
            rank = np.concatenate([[0], np.cumsum(m)])
            kp, ki, _ = O.csr_from_coo(dst[mask], src[mask], n_rows)
            assert np.array_equal(rank[ip], kp) and np.array_equal(ix[m], ki)


def test_hand_made_words_and_the_big_case_arithmetic():
    """The 8193-tile case at a size the host can hold: the same construction over 3 tiles + 1."""
    for b, e in ((0, 10), (5, 64), (63, 65)):
        for inv in (False, True):
            m = O.keep_mask(np.stack([LC.drop_all(b, e, inv)]), 100).astype(bool)
            want = np.ones(100, bool)
            want[b:e] = inv
            assert np.array_equal(m, want)
    nnz = LC.BIG_NNZ
    drops, keeps = LC.big_ranges(nnz)
    assert LC.big_table(nnz).shape == (8, 8)
    ends = [x for r in drops + keeps for x in r]
    last = LC.COMPACT_SWEEP * LC.COMPACT_TILE
    assert last in ends and last - 1 in ends and nnz in ends and any(x % 4096 == 0 for x in ends) and any(x % 64 == 63 for x in ends)
    assert all(a[1] <= b[0] for a, b in zip(drops, drops[1:]))  # disjoint, ascending: big_rank may add them up
    q = LC.big_probes(nnz)
    assert q.size > 900 and q[0] == 0 and q[-1] == nnz and np.all(np.diff(q) >= 0)
    # big_rank against a mask, on a scaled-down copy of the ranges
    small = 3 * 4096 + 1
    sd = [(0, 63), (4095, 8193), (8192 + 64, 8192 + 128), (12_288, small)]
    mask = np.ones(small, bool)
    for b, e in sd:
        mask[b:e] = False
    table = np.stack([LC.drop_all(b, e) for b, e in sd] + [LC.drop_all(100, 200, invert=True)])
    assert np.array_equal(O.keep_mask(table, small).astype(bool), mask)
    qs = np.arange(small + 1)
    assert np.array_equal(qs - sum(np.clip(qs, b, e) - b for b, e in sd), np.concatenate([[0], np.cumsum(mask)]))
    assert LC.big_rank(np.array([0, 63, 64, nnz]), nnz).tolist() == [0, 0, 1, nnz - sum(e - b for b, e in drops)]


@pytest.mark.parametrize("kind", LC.KEY_DESIGNS)
def test_oracle_builders_equal_sorted_on_tuple_keys(kind):
    for E, n_rows, n_cols in ((513, 3, 40), (700, 513, 157), (8193, 512, 50)):
        for background in (False, True):
            rows = LC.design_rows(kind, E, n_rows)
            if background:
                rows = LC.over_random(rows, n_rows, E)
            cols = LC.columns(E, n_cols)
            order = sorted(range(E), key=lambda e: (int(rows[e]), e))
            ip, ix, ei = O.csr_from_coo(rows, cols, n_rows)
            assert ei.tolist() == order and ix.tolist() == [int(cols[e]) for e in order]
            assert ip.tolist() == [sum(1 for r in rows if r < k) for k in range(n_rows + 1)] if n_rows <= 3 else True
            assert np.array_equal(ip, np.searchsorted(np.sort(rows), np.arange(n_rows + 1)))
            for n_slices in (8, 3, 1, 64):
                width = max(1, -(-n_cols // n_slices))
                key = lambda e: (min(int(cols[e]) // width, n_slices - 1), int(rows[e]), e)
                order = sorted(range(E), key=key)
                sp, si, se = O.csr_sliced_from_coo(rows, cols, n_rows, n_cols, n_slices)
                assert se.tolist() == order and si.tolist() == [int(cols[e]) for e in order]
                flat = np.sort(np.array([key(e)[0] * n_rows + key(e)[1] for e in range(E)]))
                assert np.array_equal(sp, np.searchsorted(flat, np.arange(n_slices * n_rows + 1)))


def test_the_sort_cases_meet_every_row_count_plan_and_tile_shape():
    cases = LC.sort_design_cases() + LC.sort_edge_cases()
    assert {n for _, _, n, _ in cases} == set(LC.ROW_COUNTS) and len(cases) == 98 + 30
    for kind in LC.KEY_DESIGNS:
        mine = [(E, n, bg) for k, E, n, bg in cases if k == kind]
        for E in (8193, 65_537):
            assert {n for E2, n, _ in mine if E2 == E} == set(LC.ROW_COUNTS), kind
            assert {bg for E2, _, bg in mine if E2 == E} == {False, True}
    for kind in ("round_robin", "lane_edges"):
        assert {E for k, E, _, _ in cases if k == kind} >= set(LC.SORT_E)
    assert LC.xcd_tile_order(LC.sort_tiles(65_537)).count(-1) == 7 and LC.sort_tiles(73_729) == 10 and LC.sort_tiles(8193) == 2
    rows, cols, key, order = LC.four_pass_case()
    f = LC.FOUR_PASS
    assert LC.sort_passes(0, LC.bits_for(f["n_rows"] * f["n_slices"])) == [(0, 7), (7, 7), (14, 7), (21, 7)]
    assert key.max() < f["n_rows"] * f["n_slices"] < 2 ** 31 - 1 and LC.sliced_from_csr_admits(f["n_rows"], f["n_slices"])
    for shift, bits in LC.sort_passes(0, 28):  # every pass has work: many digit values, not sorted on arrival
        dig = (key >> shift) & ((1 << bits) - 1)
        assert np.unique(dig).size >= 60 and np.any(np.diff(dig) < 0)
    assert (key >> 21).max() == 64 and np.array_equal(np.unique(cols // 1000), np.arange(64))
    assert sorted(range(key.size), key=lambda e: (int(key[e]), e)) == order.tolist()
