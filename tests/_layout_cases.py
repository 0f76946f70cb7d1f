"""Designed inputs for the integer passes that build every layout (helper, like ``_csr_cases.py``; no GPU, no library):
the record radix sort (``csrc/dgmi_sort.hip``), COO -> CSR, COO -> sliced and CSR -> sliced (``csrc/dgmi_csr.hip``) and the
per-step compaction (``csrc/dgmi_compact.hip``).  The geometry of those files is restated here; the host file checks the
restatement against the library's own size queries and the designs against what they claim."""
from collections import namedtuple

import numpy as np

from oracle import oracle as O

WAVE = 64
SORT_TILE = 8192            # records per workgroup of the sort: 16 waves x 8 rounds x 64 lanes
SORT_WAVE_RECORDS = 512     # a wave owns 512 CONSECUTIVE records
SORT_ROUNDS = 8
SORT_WAVES = 16
MAX_DIGIT_BITS = 9
MAX_BUCKETS = 1 << MAX_DIGIT_BITS
SCAN_CHUNK = 1024           # tiles per sweep of sort_bucket_scan_kernel
COMPACT_TILE = 4096         # positions per workgroup of the compaction: 256 threads x 16
WORDS_PER_TILE = COMPACT_TILE // WAVE
COMPACT_SWEEP = 8192        # tile counts per sweep of compact_scan_kernel
LONG_GAP = 64               # boundaries_kernel fills wave-wide when cur - prev > 64
PPT_MIN_EDGES = 1 << 18     # position_key_kernel<8> from here on
GRID_BLOCK = 256
GRID_CAP = 2048             # grid_for: 2048 blocks of 256, grid-stride the rest
HASH = 2654435761


def bits_for(n):
    b = 1
    while b < 32 and (1 << b) < n:
        b += 1
    return b


def sort_passes(shift0, bits):
    """[(shift, bits)] of ``radix_sort_passes``: ceil(bits / 9) passes, the bits split as evenly as possible, larger
    digits first."""
    passes = max(1, -(-bits // MAX_DIGIT_BITS))
    shift, left, out = shift0, max(bits, 1), []
    for p in range(passes):
        b = -(-left // (passes - p))
        out.append((shift, b))
        shift += b
        left -= b
    return out


def sort_tiles(E):
    return -(-E // SORT_TILE)


def xcd_tile_order(n_tiles):
    """Tile of block b (``tile_of``), -1 for an idle block: 8 * per_xcd blocks, block b takes (b & 7) * per_xcd + (b >> 3)."""
    per = -(-n_tiles // 8)
    out = []
    for b in range(8 * per):
        t = (b & 7) * per + (b >> 3)
        out.append(t if t < n_tiles else -1)
    return out


def _al(x):
    return (x + 255) // 256 * 256


def sort_workspace_bytes(E, bits):
    passes = 1 if bits <= MAX_DIGIT_BITS else -(-bits // MAX_DIGIT_BITS)
    b = _al(MAX_BUCKETS * max(sort_tiles(E), 1) * 4) + _al(MAX_BUCKETS * 4)  # tile histograms, bucket totals
    if passes > 1:
        b += 2 * 3 * _al(E * 4)                                              # two record buffers (key, eid, col)
    return b


def csr_from_coo_workspace(E, n_rows):
    return 256 + _al(E * 4) + sort_workspace_bytes(E, bits_for(n_rows))      # flag word, sorted keys, sort


def sliced_from_coo_workspace(E, n_rows, n_slices):
    return 256 + 2 * _al(E * 4) + sort_workspace_bytes(E, bits_for(n_rows * n_slices))


def sliced_from_csr_workspace(E, n_slices):
    return 256 + 2 * _al(E * 4) + sort_workspace_bytes(E, bits_for(n_slices))  # ONE pass on the slice bits


def compact_workspace_bytes(nnz):
    nt = -(-nnz // COMPACT_TILE)
    nw = nt * WORDS_PER_TILE
    return _al(nw * 8) + _al(nt * 4) + _al((nt + 1) * 4) + _al(nw * 4) + 256


def sliced_from_csr_admits(n_rows, n_slices):
    """The position key (slice << row_bits) | row must stay in the positive half of an int32."""
    return bits_for(n_rows) + bits_for(n_slices) <= 31 and n_rows * n_slices < 2 ** 31 - 1


def fill_kind(prev, cur):
    """How ``boundaries_kernel`` fills ptr[prev + 1 .. cur]: by the lane that found the gap, or by the whole wave."""
    return "wave" if cur - prev > LONG_GAP else "lane"


def boundary_gaps(sorted_keys, n_keys):
    """(prev, cur) of every position p in [0, E] of the boundary pass."""
    k = np.asarray(sorted_keys, np.int64)
    return np.concatenate([[-1], k]), np.concatenate([k, [n_keys]])


def compact_geometry(nnz):
    nt = -(-nnz // COMPACT_TILE)
    return dict(tiles=nt, words=nt * WORDS_PER_TILE, sweeps=max(1, -(-nt // COMPACT_SWEEP)) if nt else 0,
                partial_last_word=nnz % WAVE != 0)


def word_owner(word):
    """(j, wave) of ``compact_flag_kernel`` / ``compact_scatter_kernel`` that handles a word: word t of its tile is
    round j = t // 4 of wave t % 4."""
    t = word % WORDS_PER_TILE
    return t // 4, t % 4


Chunks = namedtuple("Chunks", "ppt row events")


def position_chunks(indptr, E):
    """``position_key_kernel`` on the host.  ``ppt``: 8 iff E >= 2^18.  ``row``: the row the kernel assigns to every
    position.  ``events``: (p, offset in chunk, rows stepped, search branch taken) for every position at which the walk
    left a row — the previous row ended at offset - 1 of the chunk.  (A row that ends at offset ppt - 1 leaves no event:
    the next chunk starts with its own search.)"""
    indptr = np.asarray(indptr, np.int64)
    n_rows = indptr.size - 1
    ppt = 8 if E >= PPT_MIN_EDGES else 1
    row = np.empty(E, np.int64)
    first = np.searchsorted(indptr[1:], np.arange(0, E, ppt), side="right")  # first j with indptr[j + 1] > p0
    events = []
    ip = indptr.tolist()
    for c, p0 in enumerate(range(0, E, ppt)):
        lo = min(int(first[c]), n_rows - 1)
        row_end = ip[lo + 1]
        for i in range(min(ppt, E - p0)):
            p = p0 + i
            step, start, searched = 0, lo, False
            while p >= row_end and lo < n_rows - 1:
                if step == 4:
                    lo = min(int(np.searchsorted(indptr[1:], p, side="right")), n_rows - 1)
                    row_end = ip[lo + 1]
                    searched = True
                    break
                lo += 1
                row_end = ip[lo + 1]
                step += 1
            if lo != start:
                events.append((p, i, lo - start, searched))
            row[p] = lo
    return Chunks(ppt, row, events)


# ---------------------------------------------------------------------------------------------
# key designs: the row of the record at input position e
# ---------------------------------------------------------------------------------------------
def columns(E, n_cols):
    """A hash of the position: a payload that travels with the wrong record shows in ``indices``."""
    return ((np.arange(E, dtype=np.int64) * HASH) % n_cols).astype(np.int32)


def lane_edge_rows(n_rows):
    """(a, b): b = 0 and a = the largest id below n_rows with every lower bit set, so the two differ in every digit."""
    bits = bits_for(n_rows)
    a = n_rows - 1 if n_rows == 1 << bits else (1 << (bits - 1)) - 1
    return max(a, 1) if n_rows > 1 else 0, 0


def lane_edge_kind(e):
    return (np.asarray(e) // WAVE) % 3  # 0: lane 0 in b, 1: lane 63 in b, 2: both


def wave_carry_row(n_rows):
    return n_rows // 2


def wave_carry_lane(rnd):
    return (np.asarray(rnd) * 37 + 5) % WAVE


def design_rows(kind, E, n_rows, p=None):
    e = np.arange(E, dtype=np.int64)
    if kind == "first":
        r = np.zeros(E, np.int64)
    elif kind == "last":
        r = np.full(E, n_rows - 1, np.int64)
    elif kind == "descending":
        r = (n_rows - 1) - (e * n_rows) // max(E, 1)
    elif kind == "sorted":
        r = (e * n_rows) // max(E, 1)
    elif kind == "round_robin":
        r = e % n_rows
    elif kind == "lane_edges":
        a, b = lane_edge_rows(n_rows)
        lane, k = e % WAVE, lane_edge_kind(e)
        in_b = ((lane == 0) & (k != 1)) | ((lane == WAVE - 1) & (k != 0))
        r = np.where(in_b, b, a)
    elif kind == "one_digit":
        # keys that differ only in pass p's digit, which takes every value; the other digits hold 1.  n_rows = 2^bits.
        plan = sort_passes(0, bits_for(n_rows))
        assert n_rows == 1 << bits_for(n_rows) and 0 <= p < len(plan)
        shift, b = plan[p]
        base = sum(1 << s for q, (s, _) in enumerate(plan) if q != p)
        r = base | (((e * 5 + (e >> 9)) & ((1 << b) - 1)) << shift)
    elif kind == "wave_carry":
        s = wave_carry_row(n_rows)  # n_rows >= 2; the background goes round the other rows
        r = e % (n_rows - 1)
        r = r + (r >= s)
        r = np.where(e % WAVE == wave_carry_lane(e // WAVE), s, r)
    else:
        raise ValueError(kind)
    assert r.size == 0 or (r.min() >= 0 and r.max() < n_rows)
    return r.astype(np.int32)


KEY_DESIGNS = ("first", "last", "descending", "sorted", "round_robin", "lane_edges", "wave_carry")


def over_random(rows, n_rows, seed):
    """The design on every second 64-record round and on a random half of the other positions, random rows elsewhere."""
    rng = np.random.default_rng(seed)
    E = rows.size
    keep = ((np.arange(E) // WAVE) % 2 == 0) | (rng.random(E) < 0.5)
    return np.where(keep, rows, rng.integers(0, n_rows, E)).astype(np.int32)


# the (design, E, n_rows, over a random background) of the GPU file's sort cases
ROW_COUNTS = (2, 3, 512, 513, 2 ** 17 + 1, 2 ** 18 + 1, 2 ** 20)  # 1, 2, 9, 10, 18, 19 and 20 key bits
SORT_E = (1, 2, 63, 64, 65, 511, 512, 513, 8191, 8192, 8193, 16_384, 65_536, 65_537, 73_729)


def sort_design_cases():
    """Every key design at 8 193 records (2 tiles) and 65 537 (9 tiles: per_xcd = 2, seven idle blocks) with every row
    count; every second case over a random background."""
    return [(kind, E, n, bool((i + j + k) % 2)) for i, kind in enumerate(KEY_DESIGNS) for j, E in enumerate((8193, 65_537))
            for k, n in enumerate(ROW_COUNTS)]


def sort_edge_cases():
    """round_robin and lane_edges at every round, wave and tile edge."""
    return [(kind, E, ROW_COUNTS[(i + 3 * j) % 7], False) for j, kind in enumerate(("round_robin", "lane_edges"))
            for i, E in enumerate(SORT_E)]


FOUR_PASS = dict(n_rows=2_100_000, n_cols=64_000, n_slices=64, E=20_000)  # 134.4 M keys: 28 bits, four passes of 7


def four_pass_case():
    """(rows, cols, key, order) of the four-pass case: key = slice * n_rows + row, order its stable argsort."""
    n_rows, n_cols, n_slices, E = (FOUR_PASS[k] for k in ("n_rows", "n_cols", "n_slices", "E"))
    rows = over_random(design_rows("round_robin", E, n_rows), n_rows, 9)
    rows[::7] = design_rows("descending", E, n_rows)[::7]
    cols = columns(E, n_cols)
    key = (cols.astype(np.int64) // (n_cols // n_slices)) * n_rows + rows
    return rows, cols, key, np.argsort(key, kind="stable")


# ---------------------------------------------------------------------------------------------
# boundaries
# ---------------------------------------------------------------------------------------------
GAP_DIFFS = (1, 2, 63, 64, 65, 66, 67, 129)
GAP_HUGE = 5000
GAP_HUGE_AT = (10, 64 * 5 + 20)


def gap_design(n_rows, first=0, last_gap=0, e_mod=63):
    """Occupied rows (one edge each, ascending): differences cycle through 1, 2, 63 … 67, 129 — shifted by one per
    64-position window, so that every difference meets every lane — with 5000 twice; the first occupied row is
    ``first``, the last is n_rows - 1 - last_gap, and E % 64 == e_mod (63: E + 1 fills whole waves; 0: one position
    more).  Returned in a shuffled COO order."""
    rows, i = [first], 1
    while True:
        d = GAP_HUGE if i in GAP_HUGE_AT else GAP_DIFFS[(i + i // WAVE) % len(GAP_DIFFS)]
        if rows[-1] + d >= n_rows - 1 - last_gap - GAP_HUGE:
            break
        rows.append(rows[-1] + d)
        i += 1
    while (len(rows) + 1) % WAVE != e_mod:
        rows.pop()
    rows.append(n_rows - 1 - last_gap)
    rows = np.array(rows, np.int64)
    assert np.all(np.diff(rows) > 0) and rows.size % WAVE == e_mod and rows.size > GAP_HUGE_AT[1] + WAVE
    order = np.random.default_rng(n_rows + first + last_gap).permutation(rows.size)
    return rows[order].astype(np.int32)


def gap_columns(E, n_cols, n_slices):
    """Source ids that leave slice 0 and the trailing slices empty (one slice: everything in it)."""
    width = max(1, -(-n_cols // n_slices))
    h = (np.arange(E, dtype=np.int64) * HASH) >> 7
    if n_slices == 1:
        return (h % n_cols).astype(np.int32)
    sl = 1 + h % max(1, n_slices // 2 - 1)
    c = sl * width + (h >> 3) % width
    assert c.max() < n_cols
    return c.astype(np.int32)


# ---------------------------------------------------------------------------------------------
# position keys
# ---------------------------------------------------------------------------------------------
CHUNK_EMPTY_RUNS = (0, 1, 2, 3, 4, 5, 6, 70)
CHUNK_E = PPT_MIN_EDGES + 3


def chunk_design():
    """indptr of a CSR with E = 2^18 + 3: an empty first row; for every offset o in 0 .. 7 and every k in 0 .. 6, 70 a row
    whose last edge sits at offset o of an 8-chunk, followed by k empty rows; a 100-edge row; long filler rows; empty
    last rows.  Returns (indptr, combos) with combos[(o, k)] = the row."""
    lens, combos, P = [0], {}, 0
    for rep, k in enumerate(CHUNK_EMPTY_RUNS):
        for o in range(8):
            L = (o - P) % 8 + 1 + 8 * ((o + rep) % 3)
            combos[(o, k)] = len(lens)
            lens.append(L)
            P += L
            lens += [0] * k
    lens.append((-P) % 8 + 3)  # the next row starts 3 positions into a chunk
    P += lens[-1]
    lens.append(100)
    P += 100
    while CHUNK_E - P > 1500:
        lens.append(997)
        P += 997
    lens.append(CHUNK_E - P)
    lens += [0] * 5
    indptr = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    assert indptr[-1] == CHUNK_E
    return indptr, combos


def chunk_prefix(indptr, E):
    """The CSR of the first E edges: later rows become empty last rows."""
    return np.minimum(indptr, E)


def rows_of(indptr):
    return np.repeat(np.arange(indptr.size - 1), np.diff(indptr)).astype(np.int32)


# ---------------------------------------------------------------------------------------------
# compaction
# ---------------------------------------------------------------------------------------------
WORD_KINDS = ("kept", "dropped", "bit0", "bit63", "inner", "alternating", "random")
TABLE_KINDS = ("one", "two", "three", "inverted")
SPECIAL_VALUE_BITS = (0x7FC00001, 0xFFC12345, 0x7F800001, 0x00000000, 0x80000000, 0x7F800000, 0xFF800000, 0x3F800000,
                      0x00000001, 0x807FFFFF)  # NaN payloads (quiet, negative, signalling), +-0, +-inf, 1, denormals


def _word_bits(kind, rng):
    b = np.zeros(WAVE, bool)
    if kind == "kept":
        b[:] = True
    elif kind == "bit0":
        b[0] = True
    elif kind == "bit63":
        b[63] = True
    elif kind == "inner":
        b[1:63] = True
    elif kind == "alternating":
        b[0::2] = True
    elif kind == "random":
        b = rng.random(WAVE) < 0.5
    return b


def word_kind_of(word, nnz):
    """The designed kind of a 64-position word: tile 1 wholly dropped and tile 2 wholly kept where there are three
    tiles, the kinds in turn elsewhere (shifted per tile, so that every (j, wave) owner meets several kinds)."""
    tile = word // WORDS_PER_TILE
    if nnz >= 3 * COMPACT_TILE and tile in (1, 2):
        return "dropped" if tile == 1 else "kept"
    return WORD_KINDS[(word + tile) % len(WORD_KINDS)]


def keep_tables(kind, n_ids):
    h = n_ids // 2
    sel = O.random_subset_select
    if kind == "one":
        d = [sel(n_ids, int(n_ids * 0.6), 31, 0)]
    elif kind == "two":
        d = [sel(h, int(h * 0.6), 32, 0), sel(n_ids - h, (n_ids - h) // 2, 33, h)]
    elif kind == "three":
        d = [sel(h, int(h * 0.6), 32, 0), sel(n_ids - h, (n_ids - h) // 2, 33, h), sel(n_ids, int(n_ids * 0.8), 34, 0)]
    else:
        assert kind == "inverted"
        d = [sel(n_ids, int(n_ids * 0.6), 35, 0).copy()]
        d[0][6] = 1
    return np.stack(d).astype(np.int32)


def pointer_probes(nnz):
    """Non-decreasing pointers in [0, nnz]: 0, a few word edges +- 1, every tile edge +- 1, nnz, repeated values."""
    p = [0, 0, nnz, nnz, nnz]
    for w in (1, 2, 3, 63, 65, nnz // WAVE):
        p += [w * WAVE - 1, w * WAVE, w * WAVE, w * WAVE + 1, w * WAVE + 63]
    for t in range(1, -(-nnz // COMPACT_TILE) + 1):
        p += [t * COMPACT_TILE - 1, t * COMPACT_TILE, t * COMPACT_TILE + 1]
    p = np.array(p, np.int64)
    return np.sort(p[(p >= 0) & (p <= nnz)]).astype(np.int32)


WordDesign = namedtuple("WordDesign", "nnz n_ids table mask ptr indices vals eid want_ptr want_indices want_vals nk")


def word_design(nnz, table_kind="one", n_cols=1000):
    """A layout of ``nnz`` positions whose keep bits are the designed words: ``eid[p]`` is an edge id that the real
    description table keeps or drops as position p's target bit says (a made-up eid array, ids may repeat).  The
    expectation is plain numpy: indices[mask], vals[mask], ptr_out[k] = mask[:ptr[k]].sum()."""
    rng = np.random.default_rng(nnz)
    n_words = -(-nnz // WAVE)
    mask = np.concatenate([_word_bits(word_kind_of(w, nnz), rng) for w in range(n_words)])[:nnz]
    n_ids = max(2 * nnz, 64)
    table = keep_tables(table_kind, n_ids)
    kept_ids = O.keep_mask(table, n_ids).astype(bool)
    pools = {True: np.flatnonzero(kept_ids), False: np.flatnonzero(~kept_ids)}
    assert pools[True].size and pools[False].size
    eid = np.empty(nnz, np.int64)
    for bit in (True, False):
        at = np.flatnonzero(mask == bit)
        eid[at] = pools[bit][(at * 7 + 3) % pools[bit].size]
    assert np.array_equal(kept_ids[eid], mask)
    indices = columns(nnz, n_cols)
    bits = rng.integers(0, 2 ** 32, nnz, dtype=np.uint64).astype(np.uint32)
    special = np.array(SPECIAL_VALUE_BITS, np.uint32)
    at = np.arange(0, nnz, 3)
    bits[at] = special[(at // 3) % special.size]
    vals = bits.view(np.float32)
    ptr = pointer_probes(nnz)
    rank = np.concatenate([[0], np.cumsum(mask)])
    return WordDesign(nnz, n_ids, table, mask, ptr, indices, vals, eid.astype(np.int32), rank[ptr].astype(np.int32),
                      indices[mask], vals[mask], int(mask.sum()))


def drop_all(b, e, invert=False):
    """A hand-made description word over edge ids [b, e): no hash is below 0 and no tie is kept, so it drops them all;
    inverted it keeps them all (the words of ``_csr_cases.descriptions('eight', ...)``)."""
    return np.array([b, e, 0x1234, 0x5678, 0, -1, 1 if invert else 0, 0], np.int64).astype(np.uint32).view(np.int32)


BIG_NNZ = COMPACT_SWEEP * COMPACT_TILE + 1  # 33 554 433: 8193 tiles, the second sweep of compact_scan_kernel


def big_ranges(nnz=BIG_NNZ):
    """Dropped position ranges [b, e) of the 8193-tile case (eid = position), and two "keep all" words: ends on and next
    to word and tile edges, and on both sides of position 8192 * 4096."""
    T, last = COMPACT_TILE, COMPACT_SWEEP * COMPACT_TILE
    drops = [(0, 63), (T - 1, 2 * T + 1), (5 * T + 64, 5 * T + 128), (1000 * T + 1, 1000 * T + 63),
             (last - T - 1, last - 1), (last, nnz)]
    keeps = [(3 * T, 4 * T), (last - 1, last)]
    return drops, keeps


def big_table(nnz=BIG_NNZ):
    drops, keeps = big_ranges(nnz)
    t = np.stack([drop_all(b, e) for b, e in drops] + [drop_all(b, e, invert=True) for b, e in keeps])
    assert t.shape[0] <= 8
    return t


def big_rank(q, nnz=BIG_NNZ):
    """Kept positions before q, by host arithmetic on the ranges."""
    q = np.asarray(q, np.int64)
    dropped = sum(np.clip(q, b, e) - b for b, e in big_ranges(nnz)[0])
    return (q - dropped).astype(np.int32)


def big_probes(nnz=BIG_NNZ):
    rng = np.random.default_rng(7)
    p = [0, nnz, nnz - 1, COMPACT_SWEEP * COMPACT_TILE, COMPACT_SWEEP * COMPACT_TILE - 1]
    for b, e in big_ranges(nnz)[0] + big_ranges(nnz)[1]:
        p += [b - 1, b, b + 1, e - 1, e, e + 1, (b | 63), (b | 63) + 1]
    p = np.concatenate([np.array(p, np.int64), rng.integers(0, nnz + 1, 900)])
    return np.sort(np.clip(p, 0, nnz)).astype(np.int32)
