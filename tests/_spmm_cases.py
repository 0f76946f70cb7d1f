"""Designed operands for the XCD-local SpMM (``ops.SlicedCSR.spmm``, ``ops._SplitSliced``) and the launch geometry
restated on the host.  Plain module (like _rank_cases.py), shared by test_spmm_cases_host.py and test_gpu_spmm_exact.py.

Every operand is a small integer times a power of two, so a product is EXACT in fp32 under any summation order, any fma
contraction and any split into partial planes, virtual rows or chunks, and the kernels are held to ``torch.equal``:
``X`` in [-8, 8], edge values in {+-1 .. +-4}, multiplicities 1 .. 8 (packed into the id words at ``MULT_SHIFT``),
``src_scale`` in {0.5, 1, 2}, ``dst_scale`` in {0.25, 0.5, 1, 2}, leaky slope 0.25, ``mask_scale`` 2.  Condition on every
case (``reference`` asserts it): with ``g`` the granularity of a term (1/2 when a source scale takes part), the row's
``sum |terms| / g`` stays below 2**23, so every partial sum is a multiple of ``g`` below 2**24 * g — representable.  The
longest row has 3 000 edges: 8 * 8 * 2 * 3000 / 0.5 = 768 000 at worst."""
from collections import namedtuple

import numpy as np

from oracle import oracle as O

MULT_SHIFT = 28                      # ops.MULT_SHIFT / kMultShift (test_gpu_spmm_exact.py asserts the former)
SLOPE, MASK_SCALE = 0.25, 2.0
DROP_SEED, DROP_KEEP = 77, 0.7       # the subset every dropped case uses: oracle.random_subset_mask(E, int(0.7 E), 77)
DESIGNED_LENGTHS = (0, 1, 7, 8, 9, 15, 16, 17, 31, 32, 33, 63, 64, 65, 8 * 64 + 1)  # LPR - 1, LPR, LPR + 1 for 8 / 16 / 32 / 64
EMPTY_ROWS = (110, 111, 112, 113, 303, 304, 305, 306)  # in the middle and at the end
N_DST = 307                          # prime: no multiple of any 4 * G * R
SLICED_SHAPES = {8: 157, 3: 157, 1: 50, 64: 40}  # n_slices -> n_src (64 slices of 40 sources: empty trailing slices)

Design = namedtuple("Design", "n_dst n_src n_slices dst src vals mult ss ds kept dead designed seglen")
Geometry = namedtuple("Geometry", "lpr R chunks chunk_rows workers active_touchers col_tiles ragged_tile tail_groups")
Split = namedtuple("Split", "has_light n_virtual per_row")


def col_slices(n_src, n_slices):
    """Slice of every source column, READ BACK from the oracle's layout of one edge per column (not restated)."""
    segptr, indices, _ = O.csr_sliced_from_coo(np.zeros(n_src, np.int32), np.arange(n_src, dtype=np.int32), 1, n_src, n_slices)
    out = np.empty(n_src, np.int64)
    for s in range(n_slices):
        out[indices[segptr[s]:segptr[s + 1]]] = s
    return out


def segment_lengths(dst, src, n_dst, n_src, n_slices):
    """(n_slices, n_dst) lengths of the (row, slice) segments, from ``oracle.csr_sliced_from_coo``."""
    segptr = O.csr_sliced_from_coo(dst, src, n_dst, n_src, n_slices)[0]
    return np.diff(segptr.astype(np.int64)).reshape(n_slices, n_dst)


def place_dead(rng, dst, src, kept, dead_src=(), dead_dst=()):
    """Reorder the edge list so that every edge of a dead source column / destination row sits at a DROPPED position of
    ``kept``: those nodes are then touched by dropped edges only, and a test may fill their feature rows with Inf / NaN.
    The multiset of edges — every segment length — is unchanged."""
    E = dst.size
    is_dead = np.isin(src, dead_src) | np.isin(dst, dead_dst)
    dropped_pos = rng.permutation(np.flatnonzero(~kept))
    assert is_dead.sum() <= dropped_pos.size
    pos = np.empty(E, np.int64)  # edge -> position
    pos[np.flatnonzero(is_dead)] = dropped_pos[:is_dead.sum()]
    rest = np.concatenate([dropped_pos[is_dead.sum():], np.flatnonzero(kept)])
    pos[np.flatnonzero(~is_dead)] = rng.permutation(rest)
    order = np.argsort(pos)
    return dst[order], src[order]


def drop_mask(E):
    return O.random_subset_mask(E, int(E * DROP_KEEP), DROP_SEED).astype(bool)


_designs = {}


def sliced_design(n_slices):
    """307 destination rows over ``SLICED_SHAPES[n_slices]`` sources: one (row, slice) segment of every length in
    ``DESIGNED_LENGTHS`` (rows 3, 23, 43, ... in slices 0, 1, 2, ... round robin), a background of 0 .. 12 edges per row,
    empty rows in the middle and at the end.  A few source columns are dead under the shared drop mask."""
    if n_slices in _designs:
        return _designs[n_slices]
    rng = np.random.default_rng(1000 + n_slices)
    n_src = SLICED_SHAPES[n_slices]
    slice_of = col_slices(n_src, n_slices)
    used = np.unique(slice_of)  # slices that hold a column
    designed = {}               # (row, slice) -> length
    dst, src = [], []
    for k, length in enumerate(DESIGNED_LENGTHS):
        row, s = 3 + 20 * k, int(used[k % used.size])
        designed[(row, s)] = length
        dst.append(np.full(length, row))
        src.append(rng.choice(np.flatnonzero(slice_of == s), length))
    free = np.setdiff1d(np.arange(N_DST), list(EMPTY_ROWS) + [r for r, _ in designed])
    deg = rng.integers(0, 13, free.size)
    dst.append(np.repeat(free, deg))
    src.append(rng.integers(0, n_src, int(deg.sum())))
    dst, src = np.concatenate(dst), np.concatenate(src)
    E = dst.size
    kept = drop_mask(E)
    col_deg = np.bincount(src, minlength=n_src)
    dead = np.argsort(np.where(col_deg > 0, col_deg, E + 1), kind="stable")[:4]  # the four lightest columns with an edge
    dst, src = place_dead(rng, dst, src, kept, dead_src=dead)
    seglen = segment_lengths(dst, src, N_DST, n_src, n_slices)
    for (row, s), length in designed.items():
        assert seglen[s, row] == length and seglen[:, row].sum() == length
    assert set(DESIGNED_LENGTHS) <= set(seglen.ravel().tolist())
    assert np.all(seglen[:, list(EMPTY_ROWS)] == 0) and len(designed) == len(DESIGNED_LENGTHS)
    assert np.all(np.bincount(src[kept], minlength=n_src)[dead] == 0) and np.all(col_deg[dead] > 0)
    d = Design(N_DST, n_src, n_slices, dst.astype(np.int32), src.astype(np.int32),
               (rng.integers(1, 5, E) * rng.choice([-1, 1], E)).astype(np.float32), rng.integers(1, 9, E).astype(np.int32),
               rng.choice([0.5, 1.0, 2.0], n_src).astype(np.float32), rng.choice([0.25, 0.5, 1.0, 2.0], N_DST).astype(np.float32),
               kept, dead, designed, seglen)
    for a in d:
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    _designs[n_slices] = d
    return d


def features(n, F, seed, dead=()):
    """Integers in [-8, 8] as float32; rows ``dead`` alternate Inf / NaN."""
    X = np.random.default_rng(seed).integers(-8, 9, (n, F)).astype(np.float32)
    X[list(dead)[0::2]] = np.inf
    X[list(dead)[1::2]] = np.nan
    return X


def out_mask(n, F, seed):
    return (np.random.default_rng(seed).random((n, F)) < 0.6).astype(np.float32)


def reference(dst, src, n_dst, X, w=None, ss=None, ds=None, kept=None, mask=None, act=False, x_gran=1.0):
    """``mask * 2 * leaky_0.25(diag(ds) A diag(ss) X)`` in float64 over the COO list (the surviving edges only), as
    float32.  Rows of ``X`` that no surviving edge reads may hold anything; ``x_gran``: the granularity of ``X`` (1 for
    integers).  Asserts the exactness condition."""
    e = np.arange(dst.size) if kept is None else np.flatnonzero(kept)
    wt = np.ones(e.size) if w is None else np.asarray(w, np.float64)[e]
    g = float(x_gran)
    if ss is not None:
        wt = wt * np.asarray(ss, np.float64)[src[e]]
        g *= float(np.min(np.abs(ss)))
    order = np.argsort(dst[e], kind="stable")
    rows, cols, wt = dst[e][order], src[e][order], wt[order]
    terms = X.astype(np.float64)[cols] * wt[:, None]
    assert np.isfinite(terms).all(), "a surviving edge reads a dead row"
    y = np.zeros((n_dst, X.shape[1]))
    if e.size:
        starts = np.flatnonzero(np.diff(rows, prepend=-1))
        y[rows[starts]] = np.add.reduceat(terms, starts, axis=0)
        assert np.add.reduceat(np.abs(terms), starts, axis=0).max() / g < 2 ** 23, "the design leaves fp32's exact range"
    assert np.array_equal(y / g, np.rint(y / g))
    if ds is not None:
        y = y * np.asarray(ds, np.float64)[:, None]
    if act:
        y = np.where(y > 0, y, y * SLOPE)
    if mask is not None:
        y = y * mask * MASK_SCALE
    y32 = y.astype(np.float32)
    assert np.array_equal(y32.astype(np.float64), y)
    return y32


def reference_int64(dst, src, n_dst, X, w=None, ss=None, kept=None):
    """``4 * A diag(ss) X`` in int64 (every factor is an integer once the gather-side scale, >= 1/4, is multiplied by 4)."""
    e = np.arange(dst.size) if kept is None else np.flatnonzero(kept)
    wt = np.ones(e.size, np.int64) if w is None else np.asarray(w)[e].astype(np.int64)
    wt = wt * (4 if ss is None else np.rint(4 * np.asarray(ss, np.float64)[src[e]]).astype(np.int64))
    y = np.zeros((n_dst, X.shape[1]), np.int64)
    np.add.at(y, dst[e], X[src[e]].astype(np.int64) * wt[:, None])
    return y


# ---------------------------------------------------------------------------------------------
# launch geometry: csrc/dgmi_sliced_common.h (sliced_geometry; the chunks: spmm_sliced_chunks in csrc/dgmi_sliced.hip),
# csrc/dgmi_kernels.h (pick_lpr)
# ---------------------------------------------------------------------------------------------
WAVE, WAVES_PER_BLOCK, ROWS_PER_GROUP, TOUCH_LEAD, TOUCH_GROUP = 64, 4, 8, 24, 8


def pick_lpr(F):
    f4 = (F + 3) // 4
    best, best_util = 8, 0.0
    for lpr in (64, 32, 16, 8):
        util = f4 / (-(-f4 // lpr) * lpr)
        if util >= 0.85:
            return lpr
        if util > best_util + 1e-9:
            best, best_util = lpr, util
    return best


def sliced_geometry(n_rows, F, lpr=0, rows=0, chunk_rows=0, touch_lead=-1):
    """What one ``dgmi_spmm_sliced_f32`` call launches under the five ``sliced_*`` knobs (0 / -1: the built-in choice),
    for a product below the column-pass rule's 32 768 rows.  ``workers`` / ``active_touchers`` / ``tail_groups``: one entry
    per chunk, per slice (a toucher is active when the first row it touches for lies inside the chunk)."""
    lpr = lpr if lpr in (8, 16, 32, 64) else pick_lpr(F)
    R = min(max(rows if rows > 0 else ROWS_PER_GROUP, 1), lpr - 1)
    chunk = min(chunk_rows, n_rows) if chunk_rows > 0 else n_rows
    lead = touch_lead if touch_lead >= 0 else TOUCH_LEAD
    group = TOUCH_GROUP if lead > 0 else 0
    per_block = WAVES_PER_BLOCK * (WAVE // lpr) * R
    chunks = [min(chunk, n_rows - r0) for r0 in range(0, n_rows, chunk)]
    workers = [-(-c // per_block) for c in chunks]
    touchers = [sum(1 for t in range(-(-b // group) if group else 0) if (t * group + lead) * per_block < c)
                for b, c in zip(workers, chunks)]
    return Geometry(lpr, R, len(chunks), chunks, workers, touchers, -(-F // (4 * lpr)), F % (4 * lpr) != 0,
                    [int(c % R != 0) for c in chunks])


def split_geometry(deg, row_edges, light_edges):
    """``ops._SplitSliced``: rows below ``light_edges`` edges are light when they are at least a quarter of the rows and
    not all of them; every other row (an empty one too) becomes ``max(1, ceil(deg / row_edges))`` virtual rows."""
    deg = np.asarray(deg, np.int64)
    light = deg < light_edges
    has_light = bool(4 * light.sum() >= deg.size and light.sum() < deg.size)
    if not has_light:
        light = np.zeros_like(light)
    per_row = np.where(light, 0, np.maximum(1, -(-deg // row_edges)))
    return Split(has_light, int(per_row.sum()), per_row)


# ---------------------------------------------------------------------------------------------
# the knob sweep of test_gpu_spmm_exact.py
# ---------------------------------------------------------------------------------------------
KNOBS = ("sliced_lpr", "sliced_rows", "sliced_chunk_rows", "sliced_no_off32", "sliced_touch_lead")
DEFAULTS = dict(zip(KNOBS, (0, 0, 0, 0, -1)))


def knob_values(n_dst):
    return {"sliced_lpr": (0, 8, 16, 32, 64), "sliced_rows": (0, 1, 3, 7, 15, 63),
            "sliced_chunk_rows": (0, 1, 37, n_dst - 1), "sliced_no_off32": (0, 1), "sliced_touch_lead": (-1, 0, 1, 3)}


def one_at_a_time(n_dst):
    """The default setting, each knob alone, the pairs (lpr, rows) and (chunk_rows, touch_lead), and — so that a toucher
    block runs in a chunk with ``r0 > 0`` at every width — (rows = 1, chunk_rows = 37) with a lead of 1 and of 3."""
    v = knob_values(n_dst)
    out = [dict(DEFAULTS)]
    for k in KNOBS:
        out += [dict(DEFAULTS, **{k: x}) for x in v[k] if x != DEFAULTS[k]]
    out += [dict(DEFAULTS, sliced_lpr=a, sliced_rows=b) for a in v["sliced_lpr"] for b in v["sliced_rows"]
            if a != 0 and b != 0]
    out += [dict(DEFAULTS, sliced_chunk_rows=a, sliced_touch_lead=b) for a in v["sliced_chunk_rows"]
            for b in v["sliced_touch_lead"] if a != 0 and b != -1]
    out += [dict(DEFAULTS, sliced_rows=1, sliced_chunk_rows=37, sliced_touch_lead=b) for b in (1, 3)]
    return out


def no_off32_at_every_width():
    """64-bit row addresses at every forced lane-group width: ``one_at_a_time`` takes ``sliced_no_off32`` at the built-in
    width only, so a form that only those sweeps run never met the other widths' 64-bit kernels (a width the table's
    element type does not have is ignored by the library: the built-in one)."""
    return [dict(DEFAULTS, sliced_lpr=a, sliced_no_off32=1) for a in (8, 16, 32, 64)]


def full_cross(n_dst, lpr):
    v = knob_values(n_dst)
    return [dict(sliced_lpr=lpr, sliced_rows=r, sliced_chunk_rows=c, sliced_no_off32=o, sliced_touch_lead=t)
            for r in v["sliced_rows"] for c in v["sliced_chunk_rows"] for o in v["sliced_no_off32"]
            for t in v["sliced_touch_lead"]]


def geometry_of(n_dst, F, knobs):
    return sliced_geometry(n_dst, F, knobs["sliced_lpr"], knobs["sliced_rows"], knobs["sliced_chunk_rows"],
                           knobs["sliced_touch_lead"])


# ---------------------------------------------------------------------------------------------
# the long-row graphs of the split form
# ---------------------------------------------------------------------------------------------
SPLIT_N_DST, SPLIT_N_SRC = 300, 280
SPLIT_ROWS = {7: 3000, 150: 700, 20: 1, 21: 16, 22: 17, 23: 3 * 16 + 5}   # row -> edges
SPLIT_EMPTY = (100, 101, 299)
SPLIT_LONG_COL, SPLIT_LONG_COL_EDGES = 5, 2500
SplitGraph = namedtuple("SplitGraph", "n_dst n_src dst src vals ss ds kept kept2 dead_src dead_dst deg deg_t")
_split_graphs = {}


def split_graph(kind):
    """300 rows, one of 3 000 edges and one of 700, rows of 1 / 16 / 17 / 53 edges, three empty rows, and source column 5
    with 2 500 more edges into rows 160 .. 298 (the transposed graph's long row).  ``kind == "light"``: rows 30 .. 140 hold 0 .. 3
    edges (more than a quarter of the rows are light under both layouts); ``"heavy"``: every background row holds
    24 .. 40.  A few source columns and destination rows are dead under the shared drop mask; ``kept2`` is a second
    mask (half the edges, seed 5)."""
    if kind in _split_graphs:
        return _split_graphs[kind]
    rng = np.random.default_rng({"light": 31, "heavy": 32}[kind])
    n_dst, n_src = SPLIT_N_DST, SPLIT_N_SRC
    deg = np.zeros(n_dst, np.int64)
    background = np.setdiff1d(np.arange(n_dst), list(SPLIT_ROWS) + list(SPLIT_EMPTY))
    deg[background] = rng.integers(24, 41, background.size)
    if kind == "light":
        quiet = background[(background >= 30) & (background <= 140)]
        deg[quiet] = rng.integers(0, 4, quiet.size)
    for row, n in SPLIT_ROWS.items():
        deg[row] = n
    dst = np.repeat(np.arange(n_dst), deg)
    src = rng.integers(0, n_src, dst.size)
    busy = np.arange(160, 299)
    dst = np.concatenate([dst, rng.choice(busy, SPLIT_LONG_COL_EDGES)])
    src = np.concatenate([src, np.full(SPLIT_LONG_COL_EDGES, SPLIT_LONG_COL)])
    E = dst.size
    kept = drop_mask(E)
    col_deg = np.bincount(src, minlength=n_src)
    dead_src = np.argsort(col_deg, kind="stable")[:4]  # the lightest columns
    # dead destination rows: one short background row read through the first stage (or the light path) and the
    # 17-edge row; the transposed product gathers THEIR rows of dY
    dead_dst = np.array([22, background[(background >= 30) & (deg[background] > 0)][0]])
    dst, src = place_dead(rng, dst, src, kept, dead_src=dead_src, dead_dst=dead_dst)
    kept2 = O.random_subset_mask(E, E // 2, 5).astype(bool)
    deg, deg_t = np.bincount(dst, minlength=n_dst), np.bincount(src, minlength=n_src)
    for row, n in SPLIT_ROWS.items():
        assert deg[row] == n
    assert np.all(deg[list(SPLIT_EMPTY)] == 0) and deg_t[SPLIT_LONG_COL] >= SPLIT_LONG_COL_EDGES
    assert np.all(deg_t[dead_src] > 0) and np.all(np.bincount(src[kept], minlength=n_src)[dead_src] == 0)
    assert np.all(deg[dead_dst] > 0) and np.all(np.bincount(dst[kept], minlength=n_dst)[dead_dst] == 0)
    g = SplitGraph(n_dst, n_src, dst.astype(np.int32), src.astype(np.int32),
                   (rng.integers(1, 5, E) * rng.choice([-1, 1], E)).astype(np.float32),
                   rng.choice([0.5, 1.0, 2.0], n_src).astype(np.float32), rng.choice([0.25, 0.5, 1.0, 2.0], n_dst).astype(np.float32),
                   kept, kept2, dead_src, dead_dst, deg, deg_t)
    for a in g:
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    _split_graphs[kind] = g
    return g
