"""Designed inputs for the per-edge, epilogue and selection kernels (helper, like ``_layout_cases.py``; no GPU, no
library): the gather-concat and gather-add forms, the epilogue's backward, the complement form's column sums and their
gradient, the row pre-scale, the multiplicity detection (``csrc/dgmi_edge.hip``) and the subset selection
(``csrc/dgmi_select.hip``, ``csrc/dgmi_keep.h``).  The geometry of those files is restated here; the host file checks the
designs against what they claim under that restatement, and every reference against a second evaluation.

Operands of the kernels that compute are exact in fp32 under any order or fma contraction: tables and gradients are
integers in [-8, 8], ``coef`` in {0, +-0.5, +-1, +-2}, ``scale`` in {0.25, 0.5, 1, 2}, slope 0.25, ``mask_scale`` 2; every
reference is an int64 or float64 evaluation that asserts ``sum|terms| / granularity < 2^24``."""
import math
from collections import namedtuple
from fractions import Fraction

import numpy as np

BLOCK = 256
GRID_CAP = 8192             # grid_for of dgmi_edge.hip, and scale_rows
EPILOGUE_CAP = 4096         # epilogue_backward and rank_add
COLSUM_WAVES = 16
WAVE = 64
HASH = 2654435761
SLOPE = 0.25
MASK_SCALE = 2.0
REL_TOL = 2.4e-7            # ops.MULT_REL_TOL
WINDOW_MIN_E = 1 << 16      # kWindowMinE
BINS = 4096
COLL_CAP = 1024

SENT_BITS = 0x7FC5A5A5                          # a quiet NaN no table holds: the fill of every copy output
SENT_F = np.float32(-1.2345678e30)              # the fill of every computed output (a value no result takes)
SPARE_BITS = 0x7FFFDEAD                         # NaN in the spare columns of a strided table
SPECIAL_BITS = (0x7FC00001, 0xFFC12345, 0x7F800001, 0x00000000, 0x80000000, 0x7F800000, 0xFF800000, 0x3F800000,
                0x00000001, 0x807FFFFF)  # NaN payloads (quiet, negative, signalling), +-0, +-inf, 1, denormals


def exact(total_abs, granularity):
    """The exactness condition of every reference: integers below 2^24 in units of the granularity."""
    assert np.all(np.asarray(total_abs, np.float64) / granularity < 2 ** 24)


# ---------------------------------------------------------------------------------------------
# geometry restated from dgmi_edge.hip
# ---------------------------------------------------------------------------------------------
def grid_for(n):
    return min(max(-(-n // BLOCK), 1), GRID_CAP)


def concat_form(Fa, Fb, lda, ldb, ldo, pa=0, pb=0, po=0):
    """'pow2' | 'vec4' | 'dword' from widths, leading dimensions and the pointers modulo 16."""
    vec = all(x % 4 == 0 for x in (Fa, Fb, lda, ldb, ldo)) and all(p % 16 == 0 for p in (pa, pb, po))
    if not vec:
        return "dword"
    W4 = (Fa + Fb) // 4
    return "pow2" if W4 <= BLOCK and BLOCK % W4 == 0 else "vec4"


def add_form(F, lda, ldb, ldo, pa=0, pb=0, po=0, pbias=None):
    """(VEC, HAS_BIAS) of ``gather_add_kernel``; ``pbias`` None: no bias."""
    vec = all(x % 4 == 0 for x in (F, lda, ldb, ldo)) and all(p % 16 == 0 for p in (pa, pb, po))
    vec = vec and (pbias is None or pbias % 16 == 0)
    return (4 if vec else 1), pbias is not None


def scale_form(F, ldx, ldo, px=0, po=0):
    return 4 if all(x % 4 == 0 for x in (F, ldx, ldo)) and px % 16 == 0 and po % 16 == 0 else 1


Stride = namedtuple("Stride", "units grid stride trips_min trips_max capped")


def stride_geometry(units, cap=GRID_CAP):
    """A grid-stride loop over ``units`` work items with blocks of 256: the trips of the busiest and the idlest thread."""
    grid = min(max(-(-units // BLOCK), 1), cap)
    stride = grid * BLOCK
    return Stride(units, grid, stride, units // stride, -(-units // stride), -(-units // BLOCK) > cap)


def concat_units(form, E, Fa, Fb):
    return E * ((Fa + Fb) if form == "dword" else (Fa + Fb) // 4)


Pow2 = namedtuple("Pow2", "W4 epb grid stride strides trips tail")


def pow2_geometry(E, Fa, Fb):
    """``gather_concat_vec4_pow2_kernel``: edges per block iteration, the grid (half the blocks: two edges in flight),
    the stride in edges, ``strides`` = ceil(E / stride), and per edge slot e0 < stride the trips of the two-edge loop and
    whether the tail statement runs."""
    W4 = (Fa + Fb) // 4
    epb = BLOCK // W4
    blocks = -(-E * W4 // BLOCK)
    grid = grid_for(blocks * BLOCK // 2)
    stride = grid * epb
    e0 = np.arange(stride, dtype=np.int64)
    trips = np.maximum(0, -(-(E - stride - e0) // (2 * stride)))  # trips t = 0, 1, ... while e0 + 2 t stride + stride < E
    tail = e0 + 2 * trips * stride < E
    return Pow2(W4, epb, grid, stride, -(-E // stride), trips, tail)


def pow2_edge_counts(Fa, Fb):
    """E = 1, below one stride, exactly one stride, two strides - 1 / exact / + 1 (the + 1 doubles the stride: one
    slot loops, the rest take the tail), and a ragged multi-block count.  Below the cap the grid is half the blocks, so E
    never spans more than two strides: an odd number above one needs the cap (``cap_edge_count``)."""
    epb = BLOCK // ((Fa + Fb) // 4)
    return sorted({1, max(1, epb - 1), epb, 2 * epb - 1, 2 * epb, 2 * epb + 1, 3 * epb, 6 * epb - 1, 6 * epb, 37 * epb + 3})


def stride_edge_counts(W):
    """For the grid-stride kernels (generic vec4, dword, gather_add) with W work items per edge: one edge, less than a
    block, a block boundary inside an edge, several blocks."""
    per = max(1, BLOCK // W)
    return sorted({1, 2, per, per + 1, 3 * per + 1, 1000 // W + 70})


def cap_edge_count(form, Fa, Fb):
    """The smallest E just past the 8192-block cap, plus three edges.  'pow2': three strides — every slot loops once and
    the first three also take the tail."""
    if form == "pow2":
        epb = BLOCK // ((Fa + Fb) // 4)
        return 2 * GRID_CAP * epb + 3
    W = (Fa + Fb) if form == "dword" else (Fa + Fb) // 4
    return GRID_CAP * BLOCK // W + 4


def colsum_geometry(n):
    """Per wave of ``weighted_colsum_kernel``: (8-row trips, tail rows)."""
    out = []
    for w in range(COLSUM_WAVES):
        rows = max(0, -(-(n - w) // COLSUM_WAVES))
        out.append((rows // 8, rows % 8))
    return out


# the widths of the GPU file, by the kernel a plain call takes
POW2_WIDTHS = ((128, 128), (16, 16), (8, 24), (4, 0), (0, 4), (512, 512))
VEC4_WIDTHS = ((344, 344), (128, 64), (12, 12), (0, 12))
DWORD_WIDTHS = ((5, 7), (341, 3), (0, 5), (1, 0))
ADD_WIDTHS = (128, 64, 12, 344, 7, 1)
N_A, N_B = 37, 29


def concat_variants(Fa, Fb):
    """name -> (lda, ldb, ldo, offset of A, of B, of out in elements off a 16-byte boundary).  'strided' keeps the
    16-byte path (8 spare columns everywhere); for widths of that path, one leading dimension = 1 (mod 4) or one base 4
    bytes off must fall to the dword kernel."""
    W = Fa + Fb
    v = {"plain": (Fa, Fb, W, 0, 0, 0), "strided": (Fa + 8, Fb + 8, W + 8, 0, 0, 0)}
    if Fa % 4 == 0 and Fb % 4 == 0:
        v.update(lda1=(Fa + 5, Fb, W, 0, 0, 0), ldb1=(Fa, Fb + 5, W, 0, 0, 0), ldo1=(Fa, Fb, W + 5, 0, 0, 0),
                 A_off=(Fa, Fb, W, 1, 0, 0), B_off=(Fa, Fb, W, 0, 1, 0), out_off=(Fa, Fb, W, 0, 0, 1))
    return v


def add_variants(F):
    """The same for gather_add (lda, ldb, ldo, offsets of A, B, out); the bias (none / aligned / 4 bytes off) and ``act``
    are crossed with 'plain' and 'strided' by the GPU file."""
    v = {"plain": (F, F, F, 0, 0, 0), "strided": (F + 8, F + 8, F + 8, 0, 0, 0)}
    if F % 4 == 0:
        v.update(lda1=(F + 5, F, F, 0, 0, 0), ldb1=(F, F + 5, F, 0, 0, 0), ldo1=(F, F, F + 5, 0, 0, 0),
                 A_off=(F, F, F, 1, 0, 0), B_off=(F, F, F, 0, 1, 0), out_off=(F, F, F, 0, 0, 1))
    return v


BIAS_KINDS = ("none", "aligned", "off")


# ---------------------------------------------------------------------------------------------
# indices and tables
# ---------------------------------------------------------------------------------------------
def unnamed_node(n):
    return n // 2 if n > 2 else None


def edge_ids(E, n, salt, first_last):
    """Node ids of E edges: a hash of the position, runs of seven equal ids on every third group of seven, never
    ``unnamed_node(n)``, and ``first_last`` = (id of edge 0, id of edge E - 1) (node 0 and node n - 1)."""
    e = np.arange(E, dtype=np.int64)
    ids = ((e * HASH + salt * 977) >> 7) % n
    run = (e // 7) % 3 == 0
    ids = np.where(run, ids[e - e % 7], ids)
    skip = unnamed_node(n)
    if skip is not None:
        ids = np.where(ids == skip, skip + 1, ids)
    ids[-1] = first_last[1]
    ids[0] = first_last[0]
    return ids.astype(np.int32)


def edge_pairs(E, n_a, n_b):
    return edge_ids(E, n_a, 1, (0, n_a - 1)), edge_ids(E, n_b, 2, (n_b - 1, 0))


def bit_table(n, F, ld, salt):
    """(n, ld) uint32 bit patterns: random words with the special values on every third element, the spare columns
    ``SPARE_BITS``; never the sentinel."""
    rng = np.random.default_rng(1000 * salt + F)
    t = rng.integers(0, 2 ** 32, (n, ld), dtype=np.uint64).astype(np.uint32)
    flat = t.reshape(-1)
    at = np.arange(0, flat.size, 3)
    flat[at] = np.array(SPECIAL_BITS, np.uint32)[(at // 3) % len(SPECIAL_BITS)]
    flat[flat == np.uint32(SENT_BITS)] = 0
    t[:, F:] = SPARE_BITS
    return t


def concat_reference(src, dst, A, Fa, B, Fb):
    """Bit patterns of cat(A[src, :Fa], B[dst, :Fb])."""
    out = np.empty((src.size, Fa + Fb), np.uint32)
    out[:, :Fa] = A[src, :Fa]
    out[:, Fa:] = B[dst, :Fb]
    return out


def int_table(n, F, ld, salt):
    """(n, ld) float32 integers in [-8, 8], NaN in the spare columns."""
    rng = np.random.default_rng(2000 * salt + F)
    t = rng.integers(-8, 9, (n, ld)).astype(np.float32)
    t[:, F:] = np.nan
    return t


ADD_SPECIALS = (np.nan, np.inf, -np.inf, -0.0, 0.0, 3.0, -3.0)


def special_tables(F, lda, ldb, n_a=11, n_b=13):
    """Integer tables whose first seven rows hold one special value each in EVERY column (NaN, +inf, -inf, -0, +0, 3,
    -3), and 49 + 20 edges of which the first 49 are all (src, dst) pairs of those rows."""
    A, B = int_table(n_a, F, lda, 5), int_table(n_b, F, ldb, 6)
    for i, v in enumerate(ADD_SPECIALS):
        A[i, :F] = v
        B[i, :F] = v
    src = np.concatenate([np.repeat(np.arange(7), 7), edge_ids(20, n_a, 3, (7, n_a - 1))]).astype(np.int32)
    dst = np.concatenate([np.tile(np.arange(7), 7), edge_ids(20, n_b, 4, (n_b - 1, 7))]).astype(np.int32)
    return A, B, src, dst


def relu_ref(x):
    """``torch.relu``: NaN stays NaN, -inf becomes 0, +inf stays."""
    with np.errstate(invalid="ignore"):
        return np.where(np.isnan(x), x, np.maximum(x, 0.0))


def add_reference(src, dst, A, B, bias, F, act):
    """float64 A[src] + B[dst] (+ bias), relu under ``act`` = 1: sums of three integers in [-8, 8] (or IEEE specials,
    which float64 and fp32 treat alike)."""
    with np.errstate(invalid="ignore"):
        x = A[src, :F].astype(np.float64) + B[dst, :F].astype(np.float64)
        if bias is not None:
            x = x + bias[:F].astype(np.float64)
    fin = np.isfinite(x)
    exact(np.abs(x[fin]).max(initial=0.0), 1.0)
    return (relu_ref(x) if act == 1 else x).astype(np.float32)


def same_values(got, want):
    """Zeros by value, NaN by position, everything else exactly."""
    got, want = np.asarray(got), np.asarray(want)
    return got.shape == want.shape and bool(np.all((got == want) | (np.isnan(got) & np.isnan(want))))


# ---------------------------------------------------------------------------------------------
# epilogue backward
# ---------------------------------------------------------------------------------------------
Y_KINDS = (2.0, -3.0, 0.0, -0.0, np.nan)
EPILOGUE_N = (1, 255, 256, 257, EPILOGUE_CAP * BLOCK - 1, EPILOGUE_CAP * BLOCK + 1, EPILOGUE_CAP * BLOCK + 77)


def epilogue_operands(n):
    """dY: non-zero integers in [-8, 8] (+inf, -inf, NaN at positions 40 … 54 where n allows); Y cycles through positive,
    negative, +0, -0, NaN against them (5 and 16 are coprime: every Y kind meets every dY); mask 0 / 1 with period 3."""
    i = np.arange(n, dtype=np.int64)
    dY = (i % 16 - 8).astype(np.float32)
    dY[dY >= 0] += 1
    Y = np.array(Y_KINDS, np.float32)[i % 5]
    for k, v in enumerate((np.inf, -np.inf, np.nan)):
        dY[40 + 5 * k:45 + 5 * k] = v
    mask = ((i % 3) != 1).astype(np.float32)
    return dY, Y, mask


def epilogue_reference(dY, Y, mask, act):
    """The formula of ``include/dgmi.h`` in float64."""
    with np.errstate(invalid="ignore"):
        g, y = dY.astype(np.float64), Y.astype(np.float64)
        if act == 2:
            return np.where(y > 0, g * MASK_SCALE, 0.0).astype(np.float32)
        if act == 1:
            g = g * np.where(y > 0, 1.0, SLOPE)
        if mask is not None:
            g = g * (mask.astype(np.float64) * MASK_SCALE)
    exact(np.abs(g[np.isfinite(g)]).max(initial=0.0), SLOPE)
    return g.astype(np.float32)


# ---------------------------------------------------------------------------------------------
# column sums, their gradient, the row pre-scale
# ---------------------------------------------------------------------------------------------
COLSUM_N = (0, 1, 15, 16, 17, 127, 128, 129, 255, 256, 261, 763) + (49, 65, 81, 97)  # the second group: tails of 3 … 6 rows
COLSUM_W = (1, 63, 64, 65, 344)
COLSUM_B = (1, 3, 64)
COEF_VALUES = np.array([0.0, 0.5, -0.5, 1.0, -1.0, 2.0, -2.0], np.float32)
SCALE_VALUES = np.array([0.25, 0.5, 1.0, 2.0], np.float32)


def colsum_operands(n, W, B, lda, ldc):
    """A: (n, lda) integers without a zero in the last 16 rows (every wave's last row counts); coef: (B, ldc) from
    ``COEF_VALUES``, non-zero on the last 16 rows; spare columns NaN."""
    A = int_table(n, W, lda, 7 + n)
    tail = A[max(0, n - 16):, :W]
    tail[tail == 0] = 3.0
    rng = np.random.default_rng(31 * n + B)
    coef = COEF_VALUES[rng.integers(0, COEF_VALUES.size, (B, ldc))]
    last = coef[:, max(0, n - 16):n]
    last[last == 0] = 1.0
    coef[:, n:] = np.nan
    return A, coef


def colsum_reference(A, coef, n, W):
    """out[b, c] = sum_u coef[b, u] A[u, c] as int64 in units of 0.5."""
    a = A[:n, :W].astype(np.int64)
    c2 = np.rint(coef[:, :n].astype(np.float64) * 2).astype(np.int64)
    exact(np.abs(c2) @ np.abs(a), 1.0)
    return ((c2 @ a).astype(np.float64) / 2).astype(np.float32)


def rank_add_operands(n, W, B, ldg, ldc, lds):
    G = int_table(n, W, ldg, 11 + n)
    gs = int_table(B, W, lds, 13 + B)
    rng = np.random.default_rng(17 * n + B)
    coef = COEF_VALUES[rng.integers(0, COEF_VALUES.size, (B, ldc))]
    coef[:, n:] = np.nan
    return G, coef, gs


def rank_add_reference(G, coef, gs, n, W):
    """G[u, c] + sum_b coef[b, u] gs[b, c] as int64 in units of 0.5."""
    c2 = np.rint(coef[:, :n].astype(np.float64) * 2).astype(np.int64)
    g = gs[:, :W].astype(np.int64)
    exact(2 * np.abs(G[:n, :W].astype(np.int64)) + np.abs(c2).T @ np.abs(g), 1.0)
    return ((2 * G[:n, :W].astype(np.int64) + c2.T @ g).astype(np.float64) / 2).astype(np.float32)


def scale_operands(n, F, ldx):
    X = int_table(n, F, ldx, 19)
    scale = SCALE_VALUES[(np.arange(n) * 7 + 3) % 4]
    return X, scale


def scale_reference(X, scale, n, F):
    """scale[u] X[u, c] as int64 in units of 0.25."""
    s4 = np.rint(scale.astype(np.float64) * 4).astype(np.int64)
    return ((X[:n, :F].astype(np.int64) * s4[:, None]).astype(np.float64) / 4).astype(np.float32)


# ---------------------------------------------------------------------------------------------
# row scale x multiplicity
# ---------------------------------------------------------------------------------------------
MULT_LENGTHS = (1, 63, 64, 65, 129, 200)
MULT_POSITIONS = (0, 63, 64, -1)
FAIL_KINDS = ("zero", "negative", "inf", "nan", "nine", "all_inf", "all_nan")
Row = namedtuple("Row", "name vals scale mult")  # scale 0 and mult None: a failed (or empty) row


def multiplicity_expectation(k, s):
    """Row of values k_i * s (k_i positive integers): the first c in 1 .. 8 with every k_i * c / k_min an integer in
    1 .. 8, in rational arithmetic -> (row scale, mult) or (0, None)."""
    k = [int(x) for x in k]
    kmin = min(k)
    for c in range(1, 9):
        m = [Fraction(x * c, kmin) for x in k]
        if all(f.denominator == 1 and 1 <= f <= 8 for f in m):
            return float(Fraction(kmin, c)) * s, np.array([int(f) - 1 for f in m], np.int32)
    return 0.0, None


def kernel_multiplicity_fp32(vals, rel_tol=REL_TOL, min_over=None):
    """The detection of ``row_multiplicity_kernel`` for one row, step by step in fp32: the second evaluation.
    ``min_over``: take the minimum over that many leading values only (what a minimum loop without its second trip
    would do)."""
    v = np.asarray(vals, np.float32)
    if v.size == 0:
        return np.float32(0), None, False
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        vmin = np.float32(np.inf)
        for x in v[:min_over]:
            vmin = x if x < vmin else vmin  # fminf: a NaN never becomes the minimum
        if vmin > 0 and vmin < np.inf:
            for c in range(1, 9):
                cand = np.float32(vmin / np.float32(c))
                m = np.rint(v / cand).astype(np.float32)
                ok = (m >= 1) & (m <= 8) & (np.abs(v - m * cand).astype(np.float32) <= np.float32(rel_tol) * v)
                if ok.all():
                    return cand, (np.rint(v / cand).astype(np.int32) - 1), False
    return np.float32(0), None, True


def _row(name, k, s):
    k = np.asarray(k, np.int64)
    scale, mult = multiplicity_expectation(k, s)
    return Row(name, (k * s).astype(np.float32), np.float32(scale), mult)


def multiplicity_rows():
    """The rows that have a form (and the empty ones): a unique minimum at positions 0, 63, 64 and last of rows of 1, 63,
    64, 65, 129 and 200 values; smallest value c * s for c = 1 .. 7 under multiplicities up to 8 (c = 8 with a form means
    every value is 8 s, which c = 1 takes); all-equal rows; all-8 s; two empty rows."""
    rows = []
    for L in MULT_LENGTHS:
        for pos in sorted({p % L for p in MULT_POSITIONS if -L <= p < L}):
            s = 2.0 ** -(1 + (L + pos) % 9)
            k = 2 + (np.arange(L) * 5 + pos) % 7   # 2 .. 8
            k[pos] = 1
            rows.append(_row("min@%d/%d" % (pos, L), k, s))
    rows.append(Row("empty", np.zeros(0, np.float32), np.float32(0), None))
    for c in range(1, 8):
        L = 64 + c
        k = c + np.arange(L) % (9 - c)             # c .. 8, consecutive integers: gcd 1
        k[(17 * c) % L] = c
        k[L - 1] = c + 1
        rows.append(_row("c=%d" % c, k, 2.0 ** -(c + 2)))
    rows.append(_row("all-equal", np.full(70, 3), 0.125))
    rows.append(_row("all-8s", np.full(130, 8), 2.0 ** -7))
    rows.append(_row("even", 2 * (1 + np.arange(66) % 4), 0.25))  # 2 s .. 8 s: c = 1 under scale 2 s
    rows.append(Row("empty", np.zeros(0, np.float32), np.float32(0), None))
    return rows


def breaker_rows():
    """Rows whose ONLY element outside the form (s (1 + 2^-10) among values s, 2 s, … 8 s) sits at position 0, 63, 64 or
    last."""
    rows = []
    for L in MULT_LENGTHS[1:]:
        for pos in sorted({p % L for p in MULT_POSITIONS if -L <= p < L}):
            s = np.float32(2.0 ** -(2 + (L + pos) % 5))
            v = ((1 + (np.arange(L) * 3 + pos) % 8) * s).astype(np.float32)
            v[(pos + 1) % L] = s
            v[pos] = s * np.float32(1 + 2.0 ** -10)
            rows.append(Row("breaker@%d/%d" % (pos, L), v, np.float32(0), None))
    return rows


def failing_row(kind):
    L, s = 150, np.float32(0.0625)
    v = ((1 + np.arange(L) % 8) * s).astype(np.float32)
    at = 100  # behind the first 64 values
    if kind == "zero":
        v[at] = 0.0
    elif kind == "negative":
        v[at] = -s
    elif kind == "inf":
        v[at] = np.inf
    elif kind == "nan":
        v[at] = np.nan
    elif kind == "nine":
        v[at] = 9 * s
    elif kind == "all_inf":
        v[:] = np.inf
    elif kind == "all_nan":
        v[:] = np.nan
    else:
        raise ValueError(kind)
    return Row(kind, v, np.float32(0), None)


ROWSUM_ROWS = ((3, 74), (5, 65), (7, 67))  # (k, q) with fl(fl(k / q) / k) != fl(1 / q)


def rowsum_rows():
    """Rows of values m / q as the reference's row normalisation makes them (q no power of two): 64 and more values k / q
    in front, the smallest value 1 / q behind them.  The scale is the smallest value itself; derived from one of the
    leading values it would be fl(fl(k / q) / k), one ulp off.  (With power-of-two scales that derivation is exact, and a
    minimum taken over the first 64 values alone would go unnoticed: the c-loop recovers s from any multiple of it.)"""
    rows = []
    for k, q in ROWSUM_ROWS:
        m = np.full(70, k, np.int64)
        m[[64, 69]] = 1
        m[66] = 2
        vals = (m / np.float64(q)).astype(np.float32)
        rows.append(Row("rowsum %d/%d" % (k, q), vals, vals.min(), (m - 1).astype(np.int32)))
    return rows


Mult = namedtuple("Mult", "indptr vals row_scale mult fail names")


def multiplicity_case(rows):
    """CSR of the rows and the exact expectation: ``mult`` 0 on every position of a failed row, ``row_scale`` 0 for empty
    and failed rows, ``fail`` 1 iff a non-empty row has no form."""
    indptr = np.concatenate([[0], np.cumsum([r.vals.size for r in rows])]).astype(np.int32)
    vals = np.concatenate([r.vals for r in rows] + [np.zeros(0, np.float32)]).astype(np.float32)
    mult = np.concatenate([np.zeros(r.vals.size, np.int32) if r.mult is None else r.mult for r in rows]
                          + [np.zeros(0, np.int32)]).astype(np.int32)
    scale = np.array([r.scale for r in rows], np.float32)
    fail = int(any(r.mult is None and r.vals.size for r in rows))
    return Mult(indptr, vals, scale, mult, fail, [r.name for r in rows])


def multiplicity_cases():
    """name -> rows.  'good' (no failure) with 1, 2 and 3 rows (mod 4) by dropping trailing rows; one failing row of every
    kind in the middle of the good rows; the breaker rows among the good ones; the ``rowsum_rows``."""
    good = multiplicity_rows()
    out = {}
    for drop in range(4):
        rows = good[:len(good) - drop]
        out["good-%dmod4" % (len(rows) % 4)] = rows
    for i, kind in enumerate(FAIL_KINDS):
        at = 3 + 4 * i
        out["fail-" + kind] = good[:at] + [failing_row(kind)] + good[at:]
    br = breaker_rows()
    mixed = []
    for i, r in enumerate(good):
        mixed.append(r)
        if i < len(br):
            mixed.append(br[i])
    out["breakers"] = mixed + br[len(good):]
    out["rowsum"] = good[:2] + rowsum_rows() + good[2:5]
    return out


def reference_adjacency(n=150, k=45, seed=5):
    """D^-1 (A + A^T + I) of a 0/1 k-neighbour matrix, as the reference builds its similarity graphs: rows of 70 and more
    values m / rowsum, m in 1 .. 2, every row holding an m = 1 (its diagonal).  Returns (indptr, vals fp32, m) in CSR order."""
    rng = np.random.default_rng(seed)
    a = np.zeros((n, n), np.int64)
    for i in range(n):
        others = np.delete(np.arange(n), i)
        a[i, rng.choice(others, k, replace=False)] = 1
    m = a + a.T + np.eye(n, dtype=np.int64)
    r_inv = np.power(m.sum(1).astype(np.float64), -1.0)
    rows, cols = np.nonzero(m)
    vals = (r_inv[rows] * m[rows, cols]).astype(np.float32)
    indptr = np.concatenate([[0], np.cumsum(np.bincount(rows, minlength=n))]).astype(np.int32)
    return indptr, vals, m[rows, cols].astype(np.int32)


# ---------------------------------------------------------------------------------------------
# selection
# ---------------------------------------------------------------------------------------------
def edge_hash(seed, e):
    """``edge_hash`` of ``dgmi_keep.h`` in numpy uint32 (wrapping multiplies)."""
    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    with np.errstate(over="ignore"):
        x = np.asarray(e, np.uint32) ^ np.uint32(seed & 0xFFFFFFFF)
        x = x ^ (x >> np.uint32(16))
        x = x * np.uint32(0x85EBCA6B)
        x = x ^ (x >> np.uint32(13))
        x = x * np.uint32(0xC2B2AE35)
        x = x ^ (x >> np.uint32(16))
        x = x + np.uint32(seed >> 32)
        x = x ^ (x >> np.uint32(16))
        x = x * np.uint32(0x7FEB352D)
        x = x ^ (x >> np.uint32(15))
        x = x * np.uint32(0x846CA68B)
        x = x ^ (x >> np.uint32(16))
    return x.astype(np.uint32)


def select_description(E, keep, seed, e_offset=0):
    """The 8 words as int32 bits, by ``lexsort`` on (hash, id): threshold hash and id of the keep-th smallest key."""
    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    thr, cut = 0, -1
    if keep > 0:
        h = edge_hash(seed, np.arange(E, dtype=np.uint32))
        last = int(np.lexsort((np.arange(E), h))[keep - 1])
        thr, cut = int(h[last]), last
    words = np.array([e_offset, e_offset + E, seed & 0xFFFFFFFF, seed >> 32, thr, cut & 0xFFFFFFFF, 0, 0], np.uint64)
    return words.astype(np.uint32).view(np.int32)


def select_mask(E, keep, seed):
    h = edge_hash(seed, np.arange(E, dtype=np.uint32))
    mask = np.zeros(E, np.float32)
    mask[np.lexsort((np.arange(E), h))[:keep]] = 1.0
    return mask


def select_path(E, keep, window_min=WINDOW_MIN_E):
    if keep <= 0:
        return "none"
    return "block" if E < window_min or keep >= E else "window"


Window = namedtuple("Window", "lo binw hi lo_clamped hi_clamped outcome bin bin_hi_clamped n_coll")


def select_window(E, keep, seed, narrow=False):
    """The window passes on the host: [lo, lo + 4096 binw) as ``select_or_init_kernel`` places it, whether either end was
    clamped to the hash space, and the outcome: 'window' (the bin's keys are ordered), 'miss' or 'overflow' (the workgroup
    select takes over)."""
    scale = 4294967296.0 / E
    centre = keep * scale
    half = scale if narrow else (4.0 * math.sqrt(E) + 64.0) * scale
    lo_c, hi_c = centre - half < 0.0, centre + half > 4294967296.0
    lo = int(0.0 if lo_c else centre - half)
    hi = int(4294967296.0 if hi_c else centre + half)
    binw = ((hi - lo + BINS - 1) // BINS + 1) & 0xFFFFFFFF
    h = edge_hash(seed, np.arange(E, dtype=np.uint32)).astype(np.int64)
    below = int((h < lo).sum())
    inside = np.sort(h[(h >= lo) & (h < lo + binw * BINS)])
    rem = keep - below
    if rem <= 0 or rem > inside.size:
        return Window(lo, binw, hi, lo_c, hi_c, "miss", None, False, 0)
    b = int((inside[rem - 1] - lo) // binw)
    blo, bhi = lo + b * binw, lo + b * binw + binw - 1
    clamped = bhi > 0xFFFFFFFF
    n_coll = int(((h >= blo) & (h <= min(bhi, 0xFFFFFFFF))).sum())
    return Window(lo, binw, hi, lo_c, hi_c, "window" if n_coll <= COLL_CAP else "overflow", b, clamped, n_coll)


SELECT_SEEDS = (0, 12345678901234567, 2 ** 64 - 1)
EDGE_E = (65_535, 65_536, 65_537)
SMALL_WINDOW_E = (2, 3, 64, 4_097, 8_191)


LAST_BIN_SEED = 2_424_492   # hashes of edges 0 and 1 both in the last of the 4096 bins of the whole hash space: with
LAST_BIN_CASES = ((2, 1), (3, 2))  # ``select_window_min`` = 2 the chosen bin's upper end is clamped to 0xffffffff


def edge_keeps(E):
    return (1, 2, E // 2, E - 2, E - 1)


def small_window_keeps(E):
    return sorted({1, E // 2, E - 1})


# a batch of 8: window lists, block lists, keep 0 and keep E, offsets
BATCH = dict(E=[65_536, 1_000, 65_537, 70_001, 50, 65_535, 131_072, 1],
             keep=[32_768, 999, 0, 70_001, 1, 65_534, 13, 1],
             seed=[0, 1, 2 ** 64 - 1, 12345678901234567, 5, 2 ** 63, 7, 9],
             off=[0, 5, 0, 1000, 0, 7, 0, 3])
