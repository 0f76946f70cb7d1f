"""Designed operands for the plain CSR SpMM (csrc/dgmi_spmm.hip, dgmi_segment.h: a wave per row or per plan item) and
the launch plan (csrc/dgmi_plan.hip) restated on the host.  Plain module (like _spmm_cases.py, whose operand ranges,
``reference`` and exactness condition it shares), used by test_csr_cases_host.py and test_gpu_csr_exact.py.

A wave reads the ids (and weights) of its segment 64 at a time, one per lane: a batch is FULL (64 edges) or a tail, edge
dropout on the fly compacts the survivors of a batch to its first lanes, and a plan cuts a row into chunks of at most
``chunk`` edges whose partial sums a second pass adds up, eight at a time and then one by one.  The designs put a row on
every one of these edges, and dropped / kept edges on chosen lanes of chosen batches."""
from collections import namedtuple

import numpy as np

from oracle import oracle as O

from _spmm_cases import (DESIGNED_LENGTHS, DROP_KEEP, DROP_SEED, MASK_SCALE, SLOPE, drop_mask, features, out_mask,  # noqa: F401
                         pick_lpr, place_dead, reference, reference_int64)

WAVE = 64
VEC4_WIDTHS = (4, 32, 64, 100, 128, 256, 344, 768)
DWORD_WIDTHS = (1, 3, 65, 341)
FORM_WIDTHS = (32, 64, 128, 256, 341)
# second and third id batch, FULL + FULL + tail, one long row
BATCH_LENGTHS = (127, 128, 129, 191, 192, 193, 1025, 3000)
PLAIN_N_DST, PLAIN_N_SRC = 331, 200           # 331 is prime
PLAIN_EMPTY = (110, 111, 112, 113, 327, 328, 329, 330)

Plain = namedtuple("Plain", "n_dst n_src dst src vals ss ds kept dead designed deg")
Pattern = namedtuple("Pattern", "kind n_dst n_src dst src vals ss ds desc kept dead rows want pins")
Plan = namedtuple("Plan", "items long_rows n_slots items_cap long_cap slots_cap header")
ChunkGraph = namedtuple("ChunkGraph", "n_dst n_src dst src vals ss ds lengths")


def _freeze(t):
    for a in t:
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return t


def weights(rng, E, n_src, n_dst):
    return ((rng.integers(1, 5, E) * rng.choice([-1, 1], E)).astype(np.float32),
            rng.choice([0.5, 1.0, 2.0], n_src).astype(np.float32), rng.choice([0.25, 0.5, 1.0, 2.0], n_dst).astype(np.float32))


_cache = {}


def plain_design():
    """331 destination rows over 200 sources: one row of every length in ``DESIGNED_LENGTHS`` and ``BATCH_LENGTHS`` (rows
    3, 17, 31, ...), a background of 0 .. 12 edges per row, empty rows in the middle and at the end, duplicate
    (row, col) pairs (a 3 000-edge row over 200 sources), four source columns dead under the shared drop mask."""
    if "plain" in _cache:
        return _cache["plain"]
    rng = np.random.default_rng(2024)
    n_dst, n_src = PLAIN_N_DST, PLAIN_N_SRC
    designed = {3 + 14 * k: n for k, n in enumerate(DESIGNED_LENGTHS + BATCH_LENGTHS)}
    deg = np.zeros(n_dst, np.int64)
    free = np.setdiff1d(np.arange(n_dst), list(PLAIN_EMPTY) + list(designed))
    deg[free] = rng.integers(0, 13, free.size)
    for row, n in designed.items():
        deg[row] = n
    dst = np.repeat(np.arange(n_dst), deg)
    src = rng.integers(0, n_src, dst.size)
    E = dst.size
    kept = drop_mask(E)
    col_deg = np.bincount(src, minlength=n_src)
    dead = np.argsort(np.where(col_deg > 0, col_deg, E + 1), kind="stable")[:4]
    dst, src = place_dead(rng, dst, src, kept, dead_src=dead)
    assert np.array_equal(np.bincount(dst, minlength=n_dst), deg) and not set(designed) & set(PLAIN_EMPTY)
    assert np.all(np.bincount(src[kept], minlength=n_src)[dead] == 0) and np.all(col_deg[dead] > 0)
    vals, ss, ds = weights(rng, E, n_src, n_dst)
    d = _freeze(Plain(n_dst, n_src, dst.astype(np.int32), src.astype(np.int32), vals, ss, ds, kept, dead, designed, deg))
    _cache["plain"] = d
    return d


# ---------------------------------------------------------------------------------------------
# edge dropout on the fly: dropped and kept edges on chosen lanes of chosen batches
# ---------------------------------------------------------------------------------------------
KINDS = ("one", "halves", "nested", "inverted", "three", "eight")
N_KEEP = {"one": 1, "halves": 2, "nested": 2, "inverted": 1, "three": 3, "eight": 8}
PATTERN_N_DST, PATTERN_N_SRC = 331, 200
PATTERN_EMPTY = (150, 151, 330)
PIN_ROW, PIN_EDGES = 290, 16


def _k(n, *dropped):
    """``n`` kept positions, those listed (or sliced) dropped."""
    w = np.ones(n, bool)
    for d in dropped:
        w[d] = False
    return w


# row -> (name, wanted keep pattern over the row's CSR positions); batches of a 193-edge row: 64, 64, 64, 1
PATTERN_ROWS = {
    5: ("a_first_batch_dropped", _k(193, slice(0, 64))),
    35: ("b_middle_batch_dropped", _k(193, slice(64, 128))),
    65: ("c_tail_batch_dropped", _k(200, slice(192, 200))),
    95: ("d_every_edge_dropped", _k(200, slice(0, 200))),
    125: ("e_survivor_at_lane_0", np.arange(200) % 64 == 0),
    155: ("e_survivor_at_lane_63", (np.arange(200) % 64 == 63) | (np.arange(200) == 199)),  # the tail batch: its last lane
    185: ("f_alternating", np.arange(193) % 2 == 0),
    215: ("g_full_batch_loses_one", _k(193, 64 + 17)),
    245: ("h_single_dropped_edge", _k(1, 0)),
}


def place_pattern(kept, wants, pins=None):
    """A generalisation of ``_spmm_cases.place_dead``.  A position of the COO list takes part iff ``kept[p]``, and the CSR
    order inside a row is the COO order of its edges: so row ``r`` shows the keep pattern ``wants[r]`` over its CSR
    positions when its edges sit at increasing COO positions ``p_0 < p_1 < ...`` with ``kept[p_i] == wants[r][i]``.
    ``pins``: row -> the exact COO positions of its edges (whatever ``kept`` says there).  Rows are served in turn, each
    scanning the free positions from a start of its own (so that the designed rows spread over the edge space) and from
    0 if that runs out.  Returns (row -> positions, the positions left)."""
    E = kept.size
    free = np.ones(E, bool)
    out = {}
    for row, pos in (pins or {}).items():
        pos = np.asarray(pos, np.int64)
        assert np.all(np.diff(pos) > 0) and free[pos].all()
        free[pos] = False
        out[row] = pos
    for i, (row, want) in enumerate(wants.items()):
        for start in (i * (E // (len(wants) + 2)), 0):
            got, p = [], start
            for w in want:
                while p < E and not (free[p] and kept[p] == w):
                    p += 1
                if p == E:
                    break
                got.append(p)
                p += 1
            if len(got) == len(want):
                break
        assert len(got) == len(want), "no room for row %d's pattern" % row
        free[got] = False
        out[row] = np.array(got, np.int64)
    return out, np.flatnonzero(free)


def _real(E, keep_fraction, seed, e_offset=0, invert=False):
    d = O.random_subset_select(E, int(E * keep_fraction), seed, e_offset).copy()
    if invert:
        d[6] = 1  # kKeepInvert: the edges the description drops take part
    return d


def _hand_made_ranges(E, others):
    """[b, e) of the four hand-made words of the ``eight`` kind, moved up until the descriptions around them keep edges
    b - 1, b, e - 1 and e: what the word does to the edges next to its two ends then shows in the output."""
    out = []
    for at, width in ((0.10, 100), (0.30, 100), (0.60, 70), (0.80, 100)):
        b = int(at * E)
        while not (others[b - 1] and others[b]):
            b += 1
        e = b + width
        while not (others[e - 1] and others[e]):
            e += 1
        out.append((b, e))
    return out


def descriptions(kind, E):
    """(n_keep, 8) int32 subset descriptions over the ``E`` edges of a COO list; the mask they stand for is always
    ``oracle.keep_mask(descriptions(kind, E), E)``.
      one       one real description (``oracle.random_subset_select``, 70 %)
      halves    two over the disjoint halves of the edge space (a relation-fused layout)
      nested    two over the same edges (a dropout of a dropped view): 70 % and 50 %
      inverted  one with flags bit 0: the 30 % the description drops take part
      three     the two halves and a third over everything: the table loop past the two preloaded descriptions
      eight     three real ones (two halves, one across the middle), a "drop all" word, a "keep all" word, an inverted
                "keep all" (drops all), an inverted "drop all" (keeps all) over sub-ranges, and a real one near the end"""
    h = E // 2
    if kind == "one":
        d = [_real(E, 0.7, 77)]
    elif kind == "halves":
        d = [_real(h, 0.7, 11), _real(E - h, 0.6, 12, h)]
    elif kind == "nested":
        d = [_real(E, 0.7, 77), _real(E, 0.5, 5)]
    elif kind == "inverted":
        d = [_real(E, 0.7, 77, invert=True)]
    elif kind == "three":
        d = [_real(h, 0.7, 11), _real(E - h, 0.6, 12, h), _real(E, 0.8, 13)]
    else:
        assert kind == "eight"
        real = [_real(h, 0.7, 11), _real(E - h, 0.7, 12, h), _real(E // 2, 0.8, 13, E // 4),
                _real(E // 10, 0.5, 14, int(0.85 * E))]
        (b3, e3), (b4, e4), (b5, e5), (b6, e6) = _hand_made_ranges(E, O.keep_mask(np.stack(real), E).astype(bool))
        d = real[:3] + [_real(e3 - b3, 0.0, 21, b3), _real(e4 - b4, 1.0, 22, b4), _real(e5 - b5, 1.0, 23, b5, invert=True),
                        _real(e6 - b6, 0.0, 24, b6, invert=True), real[3]]
    d = np.stack(d).astype(np.int32)
    assert d.shape == (N_KEEP[kind], 8)
    return d


def hand_made(desc):
    """(e_begin, e_end, drops) of the hand-made words of an ``eight`` description table (entries 3 .. 6)."""
    u = desc.view(np.uint32)
    return [(int(u[k, 0]), int(u[k, 1]), drops) for k, drops in ((3, True), (4, False), (5, True), (6, False))]


def pattern_design(kind):
    """331 rows over 200 sources, 0 .. 24 background edges per row, and the rows of ``PATTERN_ROWS`` arranged by
    ``place_pattern`` under ``descriptions(kind, E)``.  The same rows, lengths and columns for every kind (only the COO
    order differs).  Source columns 0 .. 3 are dead: every edge into them sits on a dropped position of a designed row.
    ``eight``: row ``PIN_ROW``'s 16 edges are edges b - 1, b, e - 1, e of the four hand-made words."""
    if kind in _cache:
        return _cache[kind]
    rng = np.random.default_rng(4242)  # the same draws for every kind
    n_dst, n_src = PATTERN_N_DST, PATTERN_N_SRC
    dead = np.arange(4)
    wants = {row: want for row, (_, want) in PATTERN_ROWS.items()}
    deg = rng.integers(0, 25, n_dst)
    deg[list(PATTERN_EMPTY)] = 0
    for row, want in wants.items():
        deg[row] = want.size
    deg[PIN_ROW] = PIN_EDGES
    E = int(deg.sum())
    desc = descriptions(kind, E)
    kept = O.keep_mask(desc, E).astype(bool)
    pins = None
    if kind == "eight":
        pins = {PIN_ROW: np.array(sorted(p for b, e, _ in hand_made(desc) for p in (b - 1, b, e - 1, e)))}
        assert pins[PIN_ROW].size == PIN_EDGES == np.unique(pins[PIN_ROW]).size
    pos, rest = place_pattern(kept, wants, pins)
    dst, src = np.full(E, -1, np.int64), np.full(E, -1, np.int64)
    live_cols = np.arange(dead.size, n_src)
    for row, p in pos.items():
        dst[p] = row
        src[p] = rng.choice(live_cols, p.size)
        if row in wants:  # every other dropped position of a designed row reads a dead column
            dropped = p[~wants[row]]
            src[dropped[0::2]] = dead[np.arange(dropped[0::2].size) % dead.size]
    others = np.repeat(np.arange(n_dst), np.where(np.isin(np.arange(n_dst), list(pos)), 0, deg))
    assert others.size == rest.size
    dst[rest] = rng.permutation(others)
    src[rest] = rng.choice(live_cols, rest.size)
    assert dst.min() >= 0 and np.array_equal(np.bincount(dst, minlength=n_dst), deg)
    assert np.all(np.bincount(src[kept], minlength=n_src)[dead] == 0) and np.all(np.bincount(src, minlength=n_src)[dead] > 0)
    vals, ss, ds = weights(rng, E, n_src, n_dst)
    d = _freeze(Pattern(kind, n_dst, n_src, dst.astype(np.int32), src.astype(np.int32), vals, ss, ds, desc, kept, dead,
                        {name: row for row, (name, _) in PATTERN_ROWS.items()}, wants, pins))
    _cache[kind] = d
    return d


def batch_counts(kept_csr, indptr, row):
    """Kept edges per 64-edge id batch of ``row`` (``kept_csr``: the mask in CSR order, ``keep_mask(desc, E)[eid]``)."""
    k = kept_csr[indptr[row]:indptr[row + 1]]
    return [int(k[b:b + WAVE].sum()) for b in range(0, k.size, WAVE)]


# ---------------------------------------------------------------------------------------------
# the launch plan: csrc/dgmi_plan.hip (header comment), csrc/dgmi_kernels.h (caps, buffer layout)
# ---------------------------------------------------------------------------------------------
PLAN_HEADER_WORDS = 16
CHUNKS = (16, 17, 64, 100, 512, 65536)
CHUNK_COUNTS = (1, 1, 2, 2, 3, 8, 8, 9, 16, 17)  # the reduce pass: no chunk to add, a chain of 2 / 3, one tree, tree + 1, two trees, + 1


def plan_items(indptr, chunk):
    """Every row is cut into chunks of at most ``chunk`` edges, one wave each (an empty row keeps one empty item):
    ``items`` (n, 4) = {row, start, end, slot} in row order, slot -1 when the row is a single chunk, else the index of the
    chunk's partial sum; ``long_rows`` (m, 4) = {row, slot0, nchunks, 0} for the rows of more than one chunk; the caps the
    host sizes the buffer by; the 16 header words {n_items, n_long, n_slots, chunk, 0 ...}."""
    indptr = np.asarray(indptr, np.int64)
    n_rows, nnz = indptr.size - 1, int(indptr[-1])
    deg = np.diff(indptr)
    c = np.where(deg <= chunk, 1, -(-deg // chunk))
    is_long = c > 1
    slot0 = np.cumsum(np.where(is_long, c, 0)) - np.where(is_long, c, 0)
    row = np.repeat(np.arange(n_rows), c)
    k = np.arange(row.size) - np.repeat(np.cumsum(c) - c, c)
    start = indptr[row] + k * chunk
    end = np.minimum(start + chunk, indptr[row + 1])
    slot = np.where(is_long[row], slot0[row] + k, -1)
    items = np.stack([row, start, end, slot], 1).astype(np.int32)
    lr = np.flatnonzero(is_long)
    long_rows = np.stack([lr, slot0[lr], c[lr], np.zeros_like(lr)], 1).astype(np.int32)
    n_slots = int(c[is_long].sum())
    long_cap = nnz // (chunk + 1)
    header = np.zeros(PLAN_HEADER_WORDS, np.int32)
    header[:4] = (items.shape[0], long_rows.shape[0], n_slots, chunk)
    return Plan(items, long_rows, n_slots, n_rows + nnz // chunk, long_cap, nnz // chunk + long_cap, header)


def chunk_lengths(chunk):
    """Row lengths on both sides of every chunk count of ``CHUNK_COUNTS``, an empty row and a single edge; for a chunk so
    large that these rows would hold millions of edges (65 536), one row of ``chunk + 1`` edges and one of ``chunk``."""
    full = (chunk - 1, chunk, chunk + 1, 2 * chunk, 2 * chunk + 1, 7 * chunk + 1, 8 * chunk, 8 * chunk + 1, 16 * chunk,
            16 * chunk + 1, 0, 1)
    return full if sum(full) <= 200_000 else (chunk + 1, chunk, 0, 1)


def chunk_design(chunk):
    """One row of every length in ``chunk_lengths(chunk)`` over 64 sources, in a fixed shuffled row order."""
    key = ("chunk", chunk)
    if key in _cache:
        return _cache[key]
    rng = np.random.default_rng(chunk)
    lengths = np.array(chunk_lengths(chunk))[np.random.default_rng(5).permutation(len(chunk_lengths(chunk)))]
    n_dst, n_src = lengths.size, 64
    dst = np.repeat(np.arange(n_dst), lengths)
    order = rng.permutation(dst.size)  # the COO list is not sorted by row
    dst, src = dst[order], rng.integers(0, n_src, dst.size)
    vals, ss, ds = weights(rng, dst.size, n_src, n_dst)
    g = _freeze(ChunkGraph(n_dst, n_src, dst.astype(np.int32), src.astype(np.int32), vals, ss, ds, lengths))
    _cache[key] = g
    return g
