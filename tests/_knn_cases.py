"""Designed rows for the bf16-screened cosine kNN (csrc/dgmi_knn_screen.hip), and the screen's arithmetic restated on the
host.  Plain module (like _rank_cases.py), shared by test_knn_cases_host.py, test_gpu_spmm.py and tools/knn_soak.py; its
second half (unit rows on a lattice, the screen's workspace layout and emission regions restated) serves
test_knn_lattice_host.py and test_gpu_knn_exact.py.

The screen multiplies bf16 copies of unit rows (round to nearest even: unit roundoff 2**-8 per element) and keeps every
candidate within ``2 * eps`` of a lower bound of the query's k-th best approximate score; the answer is exact only if
``|approx - exact| <= eps`` for EVERY pair.  On random rows the roundings cancel to ~1e-4, so random data cannot tell a
sound eps from one several times too small.  These rows make every rounding pull the same way:

  q   columns [0, h)   p (1 + 2**-8)(1 - eta): just below a bf16 midpoint, rounds DOWN to p
      columns [h, 2h)  p (1 + 2**-8)(1 + eta): just above it, rounds UP to p (1 + 2**-7)
  A   columns [0, h)   p (1 + 53/128 + 2**-8)(1 - eta): rounds down         -> approx(q, A) is too SMALL by ~0.0047
  B_j columns [h, 2h)  p (1 + 53/128 + 2**-8)(1 + eta): rounds up           -> approx(q, B_j) is too LARGE by ~0.0047
      of which ``nlow`` sit one bf16 step lower, p (1 + 52/128 + 2**-8)(1 + eta), so that exact(q, A) > exact(q, B_j)

and every row carries a filler, in columns where q is zero (q's own: where every other row is zero), that makes its fp32
norm 1.  A is q's true nearest neighbour; a screen whose eps is below the attained error never lets A reach the exact
rescoring once k decoys B_j have set the threshold.

eta = 2**-18 survives the rounding of the designed values to fp32 (half an ulp is 2**-24 relative) and is far below what
the scores resolve."""
import functools
import math
from collections import namedtuple

import numpy as np
import torch

ETA = 2.0 ** -18
U_BF16 = 2.0 ** -8                       # unit roundoff of bf16 under round to nearest: 8 significant bits
EPS_TRUE = 2.0 ** -7 + 2.0 ** -16        # (1 + u)**2 - 1: |approx - exact| <= EPS_TRUE |q| |c|, products summed exactly
EPS_OLD = 0.0042                         # the margin the screen shipped with (2**-8 + 2**-18 + slack): too small

Design = namedtuple("Design", "D k p h nlow q A B")   # q, A: (D,) float32; B: (k, D) float32


def shape_of(D):
    """(p, h) for width D: p = 2**-e and h columns per half, h <= (D - 4) / 2 (four columns stay free for fillers), with
    the largest h p**2 <= 0.4961 (q's designed part has squared norm 2 h p**2 (1 + 2**-8)**2 < 1): the highest score."""
    best = None
    for e in range(1, 12):
        p = 2.0 ** -e
        h = min((D - 4) // 2, int(0.4961 / (p * p)))
        if h >= 1 and (best is None or h * p * p >= best[1] * best[0] ** 2):  # (a tie: the wider design)
            best = (p, h)
    assert best is not None, "D too small for the design"
    return best


# Decoy elements one bf16 step lower: each takes p**2 (1 + 2**-8) / 128 off the decoy's exact score and as much off its
# approximate one.  With none, exact(B) is 1e-5 ABOVE exact(A) (the two eta terms).  p <= 2**-4 (D >= 256): 10, an exact
# gap of 3.0e-4 (D = 1024: 6.6e-5).  p = 2**-3 (D <= 128), where one step is worth 1.2e-4: 2, an exact gap of 2.3e-4 — with
# 10 the decoys' approximate scores would fall far enough for A to pass the old margin.
def default_nlow(D):
    return 10 if shape_of(D)[0] < 2.0 ** -3 else 2


def _with_filler(main64, cols, weights):
    """float32 row: the designed part (rounded to fp32 first) plus a filler spread over `cols` in proportion to
    `weights` (a unit vector) that brings the norm OF THE FP32 ROW to 1."""
    row = main64.astype(np.float32)
    rest = 1.0 - float(np.sum(row.astype(np.float64) ** 2))
    assert rest > 0.0, "no room for a filler"
    assert np.all(row[list(cols)] == 0)
    row[list(cols)] = (math.sqrt(rest) * np.asarray(weights, dtype=np.float64)).astype(np.float32)
    return row


def build(D, k, nlow=None):
    """q, A and k decoys for width D.  The decoys differ only in their fillers — distinct columns where D leaves room,
    otherwise distinct directions in the last two columns — so they are k distinct rows with the SAME exact and the same
    approximate similarity to q (q is zero in every filler column but its own)."""
    p, h = shape_of(D)
    nlow = default_nlow(D) if nlow is None else nlow
    assert 0 <= nlow <= h and k >= 1
    lo, hi = 1.0 - ETA, 1.0 + ETA
    q = np.zeros(D)
    q[:h] = p * (1 + U_BF16) * lo
    q[h:2 * h] = p * (1 + U_BF16) * hi
    a = np.zeros(D)
    a[:h] = p * (1 + 53 / 128 + U_BF16) * lo
    b = np.zeros(D)
    b[h:2 * h] = p * (1 + 53 / 128 + U_BF16) * hi
    b[h:h + nlow] = p * (1 + 52 / 128 + U_BF16) * hi
    free = D - 2 * h - 2                 # columns after q's and A's fillers
    assert free >= 2
    rows_b = []
    for j in range(k):
        if free >= k:
            rows_b.append(_with_filler(b, [2 * h + 2 + j], [1.0]))
        else:
            th = 0.5 * math.pi * (j + 1) / (k + 1)
            rows_b.append(_with_filler(b, [D - 2, D - 1], [math.cos(th), math.sin(th)]))
    t = torch.from_numpy
    return Design(D, k, p, h, nlow, t(_with_filler(q, [2 * h], [1.0])), t(_with_filler(a, [2 * h + 1], [1.0])),
                  t(np.stack(rows_b)))


def bf16_round(x):
    """fp32 -> bf16 (round to nearest even, what knn_to_bf16_kernel does) -> float64."""
    return x.to(torch.float32).to(torch.bfloat16).to(torch.float64)


def exact_scores(q, C):
    """<q, c> of fp32 rows in float64."""
    return C.to(torch.float64) @ q.to(torch.float64)


def approx_scores(q, C):
    """What the screen computes, up to fp32 accumulation order: bf16 x bf16 products summed in float64."""
    return bf16_round(C) @ bf16_round(q)


def embed(base, design, q_at, a_at, b_at=0):
    """A copy of the unit rows `base` (N, D) with the design written over rows q_at, a_at and b_at .. b_at + k - 1."""
    x = base.clone()
    k = design.B.shape[0]
    assert len({q_at, a_at} | set(range(b_at, b_at + k))) == k + 2
    x[q_at], x[a_at], x[b_at:b_at + k] = design.q, design.A, design.B
    return x


# ---------------------------------------------------------------------------------------------------------------------
# Unit rows on a lattice: every similarity exact in every number format and summation order of the search.
#
# A row has exactly nz = 4**m non-zeros, each +-2**-m (nz = 64, +-1/8 for D >= 128; nz = 16, +-1/4 for D = 64): its fp32
# norm is exactly 1, every element is a bf16 number, every dot product is an integer multiple of 1 / nz in [-1, 1] whose
# partial sums are multiples of 1 / nz too — the fp32 MFMA chain, the bf16 screen and the rescoring's `wave_dot` return the
# same value, and the reference is an integer matrix product (`Lattice.num`: the numerators -1 / 0 / +1 of the elements).
#   ordinary   nz / 4 anchor columns (0 .. nz / 4 - 1) all +, the other 3 nz / 4 at random columns with random signs:
#              similarity 1/4 + a small random part to each other — few levels, so the k-th boundary cuts a tie class
#   antipodal  the anchors all -: similarity -1/4 + a small random part to every ordinary row; their k-th neighbour is
#              negative once k passes their few non-negative candidates (self, the other antipodal rows, the zero rows)
#   zero       all-zero rows (what `feature_similarity_graph` makes of a zero-norm feature row): similarity 0 to everything
#   block      `block` exact copies of one ordinary row, contiguous, across a 128- and a 256-row boundary (and 32-row ones)
#   pairs      scattered exact copies of single ordinary rows
# Special rows sit at the front (ids < 32: the first tile of every kernel), around 2 N / 3 and among the last five rows.
Lattice = namedtuple("Lattice", "N D nz x num antipodal zero block pairs")


def lattice_nz(D):
    return 64 if D >= 128 else 16


@functools.lru_cache(maxsize=None)
def lattice(N, D, seed=3, specials=True, block=None):
    """The rows described above.  `specials=False`: ordinary rows and the block only.  `block`: copies in the block
    (default 300 from 700 rows, N / 4 below).  Returns x (N, D) float32, num (N, D) int8, the ids of the special rows,
    the block as (lo, hi) and the pairs as (original, copy)."""
    assert D >= 64 and N >= 16
    nz = lattice_nz(D)
    anchors, rest = nz // 4, nz - nz // 4
    rng = np.random.default_rng(seed)
    num = np.zeros((N, D), dtype=np.int8)
    num[:, :anchors] = 1
    cols = anchors + np.argpartition(rng.random((N, D - anchors), dtype=np.float32), rest, axis=1)[:, :rest]
    np.put_along_axis(num, cols, (rng.integers(0, 2, (N, rest)) * 2 - 1).astype(np.int8), axis=1)
    if block is None:
        block = 300 if N >= 700 else N // 4
    if N >= 700:
        lo = 256 * max(1, (N // 4 + 128) // 256) - 150       # straddles a multiple of 256 (and of 128 on either side)
    else:
        lo = min(32, N // 2) - block // 2                    # straddles row 32 (tiny N: row N / 2)
    assert 0 <= lo and lo + block <= N
    num[lo:lo + block] = num[lo]
    antipodal, zero, pairs = (), (), ()
    if specials:
        mid = 2 * N // 3
        if N >= 64:
            antipodal, zero = (5, mid + 5, N - 2), (9, 10, mid + 9, N - 3, N - 1)
            pairs = ((12, mid + 12), (mid + 14, N - 4), (14, N - 5))
        else:
            antipodal, zero, pairs = (1,), (2, N - 1), ((3, N - 2),)
        used = list(antipodal + zero) + [i for p in pairs for i in p]
        assert len(set(used)) == len(used) and all(0 <= i < N and not lo <= i < lo + block for i in used)
        for a, b in pairs:
            num[b] = num[a]
        for i in antipodal:
            num[i, :anchors] = -1
        for i in zero:
            num[i] = 0
    x = torch.from_numpy(num.astype(np.float32) * np.float32(1.0 / math.sqrt(nz)))
    num.setflags(write=False)
    return Lattice(N, D, nz, x, num, antipodal, zero, (lo, lo + block), pairs)


@functools.lru_cache(maxsize=None)
def mostly_zero(N, D, live=64, seed=3):
    """All rows zero except `live` lattice rows spread evenly: every query's threshold is <= 0, so every region of every
    query overflows and the whole answer comes from the exact take-over."""
    base = lattice(N, D, seed, specials=False)
    keep = np.linspace(0, N - 1, live).astype(np.int64)
    num = np.zeros_like(base.num)
    num[keep] = base.num[keep]
    num.setflags(write=False)
    zero = tuple(sorted(set(range(N)) - set(keep.tolist())))
    x = torch.from_numpy(num.astype(np.float32) * np.float32(1.0 / math.sqrt(base.nz)))
    return Lattice(N, D, base.nz, x, num, (), zero, (0, 0), ())


def similarity_numerators(num, rows=None):
    """S[i, j] * nz as int64 (exact), for the query rows `rows` (default all) against every row."""
    a = num if rows is None else num[np.asarray(rows)]
    return (a.astype(np.float32) @ num.astype(np.float32).T).astype(np.int64)   # |sums| <= 64: exact in fp32 in any order


def expected_topk(S, k):
    """Ids of the k best candidates of every row of S by (similarity descending, id ascending)."""
    return np.argsort(-np.asarray(S), axis=1, kind="stable")[:, :k]


# --- the small-N kernel's candidate splits and the screen's workspace, restated (dgmi_knn.hip, dgmi_knn_screen.hip) ---
SCREEN_MIN_ROWS, SCREEN_BIG_MIN_ROWS, SPLITS, POOL_CHUNK = 1536, 49152, 8, 256
SCREEN_EPS = np.float32(0.008)
OVERFLOW_MARK = 0x40000000

ScreenLayout = namedtuple("ScreenLayout", "big sym tile Np Dp cap_r cap_c pool_chunks xb part tau thr cnt buf flags pool "
                                          "pool_ctl total")


def knn_splits(N):
    """`knn_splits`: (splits, 32-candidate tiles per split) of the fp32 kernel below the screen's crossover."""
    q_tiles = c_tiles = (N + 31) // 32
    s = max(1, min((512 + q_tiles - 1) // q_tiles, (c_tiles + 3) // 4, 64))
    return s, (c_tiles + s - 1) // s


def _align256(b):
    return (b + 255) & ~255


def default_pool_chunks(N, k):
    """The built-in `knn_pool_chunks` of the 256 x 256 shape: room for 20 k + 112 records per query in 256-record chunks,
    plus one partly filled chunk per wave of every workgroup in flight."""
    return min((N * (20 * k + 112) + POOL_CHUNK - 1) // POOL_CHUNK + 2048, 1 << 30)


def screen_layout(N, D, k, pool_chunks=0):
    """`screen_layout`: tile shape, sweep, padded sizes, region caps, pool chunks (`pool_chunks` > 0: the tuning knob) and the
    byte offset of every array in the workspace, each rounded up to 256 bytes."""
    big = N >= SCREEN_BIG_MIN_ROWS
    tile = 256 if big else 128
    Np, Dp = (N + tile - 1) // tile * tile, (D + 63) // 64 * 64
    sym = N >= (24576 if k <= 8 else 40960)
    cap_r = 128 if k <= 8 else (256 if (k <= 16 or sym) else 512)
    cap_c = SPLITS * cap_r if sym else 0
    chunks = default_pool_chunks(N, k) if big else 0
    if chunks and pool_chunks > 0:
        chunks = pool_chunks
    at, offs = 0, []
    for size in (Np * Dp * 2, N * 64 * 4 * 4, N * 4, Np * 4, N * (SPLITS + 1) * 4, N * (SPLITS * cap_r + cap_c) * 8, N * 4,
                 chunks * POOL_CHUNK * 16, (chunks + 1) * 4 if chunks else 0):
        offs.append(at)
        at += _align256(size)
    return ScreenLayout(big, sym, tile, Np, Dp, cap_r, cap_c, chunks, *offs, at)


def workspace_bytes(N, D, k, pool_chunks=0):
    """`dgmi_knn_cosine_workspace_bytes` for a supported shape."""
    if N >= SCREEN_MIN_ROWS and D <= 1024:
        return screen_layout(N, D, k, pool_chunks).total
    s, _ = knn_splits(N)
    return 0 if s == 1 else s * N * k * 8


def emit_tile_ranges(N, k, q_tile):
    """The candidate tiles [t0, t1) of the 8 workgroups (splits) that emit for query tile `q_tile`: contiguous ranges of
    ceil(remaining / 8) tiles, from tile 0 on the full rectangle and from the diagonal tile under the triangular sweep."""
    L = screen_layout(N, 64, k)
    n_tiles = L.Np // L.tile
    first = q_tile if L.sym else 0
    per = (n_tiles - first + SPLITS - 1) // SPLITS
    out = []
    for s in range(SPLITS):
        t0 = first + s * per
        out.append((t0, t0 + (per if t0 + per <= n_tiles else max(n_tiles - t0, 0))))
    return out


def emit_regions(N, k, q):
    """Where query q's buffer entries come from: ([lo, hi) candidate ids of its 8 row regions, [0, hi) of its column
    region).  A row region takes every candidate of its split's tiles, the diagonal tile whole (self included); the column
    region (triangular sweep) takes what the query tiles BEFORE q's own offer, i.e. the candidates in front of q's tile."""
    L = screen_layout(N, 64, k)
    qt = q // L.tile
    rows = [(min(t0 * L.tile, N), min(t1 * L.tile, N)) for t0, t1 in emit_tile_ranges(N, k, qt)]
    return rows, (0, qt * L.tile if L.sym else 0)


def region_counts(S, q_ids, thr, N, k):
    """(len(q_ids), 9) entries offered to the 8 row regions and the column region of the queries `q_ids`, whose rows of
    similarities are S (len(q_ids), N), under the per-query emission thresholds `thr` (same unit as S)."""
    hit = np.asarray(S) >= np.asarray(thr)[:, None]
    run = np.concatenate([np.zeros((hit.shape[0], 1), dtype=np.int64), np.cumsum(hit, axis=1)], axis=1)
    out = np.zeros((len(q_ids), SPLITS + 1), dtype=np.int64)
    for i, q in enumerate(q_ids):
        rows, col = emit_regions(N, k, int(q))
        out[i, :SPLITS] = [run[i, hi] - run[i, lo] for lo, hi in rows]
        out[i, SPLITS] = run[i, col[1]] - run[i, col[0]]
    return out


def region_caps(N, k):
    L = screen_layout(N, 64, k)
    return np.array([L.cap_r] * SPLITS + [L.cap_c], dtype=np.int64)


def pessimistic_threshold(S, k, nz, tile):
    """The lowest emission threshold the k <= 4 sample can produce, in numerators: each lane keeps its four best, so tau' is
    the exact k-th largest over the sampled candidates, and candidate tile 0 is always sampled — tau' >= the k-th largest
    inside tile 0.  Minus 2 eps = 0.016 (just over one lattice step at nz = 64)."""
    assert k <= 4
    kth = -np.sort(-np.asarray(S)[:, :tile], axis=1)[:, k - 1]
    tau = (kth / nz).astype(np.float32)
    return (tau - np.float32(2.0) * SCREEN_EPS).astype(np.float64) * nz


def sampled_tiles(N, D, k, screen_first=False):
    """The candidate tiles the SAMPLE pass multiplies: every `stride`-th tile (8 from 64 tiles, n_tiles / 8 below, every
    tile below 8; the LDS-DMA kernel: 4 for k > 16 from 128 tiles), dealt round-robin to the 8 splits; the LDS-DMA kernel
    (256 x 256 tiles, two or more 64-column chunks, not `knn_screen_first`) gives every split the same number of tiles
    and leaves the few beyond a multiple of 8 out.  Tile 0 is always among them."""
    L = screen_layout(N, D, k)
    n_tiles = L.Np // L.tile
    dma = L.big and L.Dp >= 128 and not screen_first
    stride = 4 if dma and k > 16 and n_tiles >= 128 else (8 if n_tiles >= 64 else (n_tiles // 8 if n_tiles >= 8 else 1))
    out = []
    for s in range(SPLITS):
        t0, step = stride * s, stride * SPLITS
        nt = (n_tiles - t0 + step - 1) // step if n_tiles > t0 else 0
        sampled = (n_tiles + stride - 1) // stride
        if dma and sampled >= 2 * SPLITS:
            nt = min(nt, sampled // SPLITS)
        out += [t0 + step * i for i in range(nt)]
    return sorted(out), L.tile


def sample_threshold(S, N, D, k, nz, screen_first=False):
    """(tau', emission threshold) in numerators for k <= 4, where every lane's four best hold the k best of its subset and
    tau' is the exact k-th largest over the sampled candidates."""
    assert k <= 4
    tiles, T = sampled_tiles(N, D, k, screen_first)
    cols = np.concatenate([np.arange(t * T, min((t + 1) * T, N)) for t in tiles])
    kth = -np.sort(-np.asarray(S)[:, cols], axis=1)[:, k - 1]
    tau = (kth / nz).astype(np.float32)
    return kth, (tau - np.float32(2.0) * SCREEN_EPS).astype(np.float64) * nz


# (N, D, k) of tests/test_gpu_knn_exact.py, the smallest N at which each path exists (test_knn_lattice_host.py checks the
# designs at exactly these shapes)
SMALL_SHAPES = [(763, 256, 4), (1500, 128, 13), (1535, 64, 16), (97, 64, 13), (33, 64, 16), (16, 64, 16)]
RECT_SHAPES = [(N, D, k) for N in (1536, 2048 + 37) for D, k in ((256, 4), (256, 13), (256, 40), (256, 64), (64, 4), (768, 4))]
TRI_SHAPES = [(24576 + 128 + 37, 256, 4), (40960 + 37, 256, 12), (40960 + 37, 256, 64)]
BIG_SHAPES = [(49152 + 300, 256, 4), (49152 + 300, 256, 12), (49152 + 300, 256, 40), (49152 + 300, 64, 4)]
SCREEN_SHAPES = RECT_SHAPES + TRI_SHAPES + BIG_SHAPES
