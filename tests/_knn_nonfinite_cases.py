"""Lattice rows of _knn_cases.py with chosen rows made non-finite, and the contract of `dgmi_knn_cosine_topk_f32` for
them restated on the host (include/dgmi.h).  Plain module, shared by test_knn_nonfinite_host.py and
test_gpu_knn_nonfinite.py.

A NaN row comes in two forms — ONE element NaN (at a column where the lattice row may well hold a zero: NaN x 0 is NaN too)
and ALL elements NaN — and with several bit patterns: the quiet NaN 0x7fc00000 and payloads that a careless
round-to-nearest-even to bf16 (`(u + 0x7fff + lsb) >> 16`) carries into +Inf (0x7f800001), -0 (0x7fffffff), +0 (0xffffffff)
or -Inf (0xff800001): a screen that lost the NaN there would treat the row as comparable.

The expected list of a finite row is `_knn_cases.expected_topk` over the finite columns only, then -1; a NaN row's list is
k times -1.  Ties at the k-th value stay free on the GPU (checks (a) of test_gpu_knn_exact.py); `expected_lists` fixes
them by id only so that the host file can compare it with a brute-force `sorted()`."""
import functools
from collections import namedtuple

import numpy as np
import torch

import _cases as C
import _knn_cases as K

NAN_BITS = (0x7FC00000, 0x7F800001, 0x7FFFFFFF, 0xFFFFFFFF, 0xFF800001, 0xFFC00000)
SENTINEL = -7.0     # spare columns of the ld = D + 8 buffer

Case = namedtuple("Case", "lat x bad finite forms")   # x (N, D) float32 tensor; bad: ids; finite: (N,) bool array


def old_bf16_bits(u):
    """The rounding `knn_to_bf16_kernel` had: round to nearest even on the raw bits, NaN not looked at."""
    u = np.asarray(u, dtype=np.uint64)
    return ((u + 0x7FFF + ((u >> 16) & 1)) & 0xFFFFFFFF) >> 16


def tile_of(N):
    """Rows per tile of the kernel that takes N rows: 32 (fp32 kernel), 128 / 256 (screen)."""
    return 32 if N < K.SCREEN_MIN_ROWS else (256 if N >= K.SCREEN_BIG_MIN_ROWS else 128)


def placement(d):
    """Ids of the rows made non-finite, by what they are there for."""
    N = d.N
    lo, hi = d.block
    t = tile_of(N)
    last0 = (N - 1) // t * t
    if N < 64:
        return dict(front=(4,), block=(lo + 2,), last_tile=(N - 1,), late=(N - 5,))
    edge = (lo // 256 + 1) * 256                     # the multiple of 256 the block straddles
    assert lo < edge < hi
    return dict(front=(3, 17),                        # ids < 32: tile 0 of every kernel, always sampled
                block=(lo + 5, edge - 1, edge),       # inside the 300 copies, on both sides of a tile boundary
                late=(2 * N // 3 + 1,),               # behind the diagonal for the first two thirds of the queries
                last_tile=(max(last0, N - 6),))       # the (ragged) last tile


def _write(x, rows, patterns):
    """Rows `rows` of the float32 array x made non-finite; even positions: one element, odd positions: all elements."""
    u = x.view(np.uint32)
    forms = {}
    for i, r in enumerate(rows):
        bits = patterns[i % len(patterns)]
        if i % 2 == 0:
            u[r, (7 * r + 3) % x.shape[1]] = bits
            forms[r] = "one"
        else:
            u[r, :] = bits
            forms[r] = "all"
    return forms


@functools.lru_cache(maxsize=None)
def nan_case(N, D, rows=None):
    """lattice(N, D) with the rows of `placement` (or `rows`) holding NaN."""
    d = K.lattice(N, D)
    if rows is None:
        rows = tuple(sorted({r for v in placement(d).values() for r in v}))
    x = d.x.numpy().copy()
    forms = _write(x, rows, NAN_BITS)
    finite = np.ones(N, dtype=bool)
    finite[list(rows)] = False
    assert np.array_equal(np.isnan(x).any(axis=1), ~finite)
    return Case(d, torch.from_numpy(x), tuple(rows), finite, forms)


INF_BITS = (0x7F800000, 0xFF800000)


@functools.lru_cache(maxsize=None)
def inf_case(N, D):
    """lattice(N, D) with the rows of `placement` holding +-Inf and no NaN: one +Inf or -Inf element, a whole row of one
    sign, and (rows at the `late` placement) one +Inf next to one -Inf element — scores of +Inf, -Inf and NaN from finite and
    infinite operands alike."""
    d = K.lattice(N, D)
    p = placement(d)
    rows = tuple(sorted({r for v in p.values() for r in v}))
    x = d.x.numpy().copy()
    forms = _write(x, rows, INF_BITS + INF_BITS[::-1])   # one +Inf, all -Inf, one -Inf, all +Inf, ...
    u = x.view(np.uint32)
    for r in p["late"]:
        u[r, 0], u[r, 1] = INF_BITS
        forms[r] = "both"
    finite = np.ones(N, dtype=bool)
    finite[list(rows)] = False
    assert not np.isnan(x).any() and np.array_equal(np.isinf(x).any(axis=1), ~finite)
    return Case(d, torch.from_numpy(x), rows, finite, forms)


# fewer finite rows than k: (N, D, k, the finite rows); every other row holds a NaN
FEW_33 = (33, 64, 16, tuple(range(0, 33, 3)) + (31, 32))            # 13 finite rows, 20 NaN rows
FEW_1536 = (1536, 64, 13, (7, 130, 700, 701, 1400, 1535))            # 6 finite rows in 5 tiles


def few_case(N, D, k, keep):
    assert len(keep) < k
    return nan_case(N, D, tuple(r for r in range(N) if r not in keep))


def expected_lists(case, k):
    """(N, k) int64: a finite row's top min(k, #finite) finite rows by (similarity desc, id asc), then -1; a non-finite
    row: k times -1."""
    N = case.lat.N
    fin = np.flatnonzero(case.finite)
    kf = min(k, fin.size)
    out = np.full((N, k), -1, dtype=np.int64)
    if kf:
        S = K.similarity_numerators(case.lat.num, fin)[:, fin]
        out[fin, :kf] = fin[K.expected_topk(S, kf)]
    return out


def magnets(case):
    """Two guard rows for either end of the table: copies of finite rows, row -1 a copy of the FIRST finite row and row N a
    copy of the last — each its source's best neighbour (similarity 1, and the lower id).  A kernel that scores "row -1"
    ranks it in front of real neighbours; nothing faults, the rows are the test's own memory."""
    fin = np.flatnonzero(case.finite)
    pick = lambda i: case.x[fin[i % fin.size]]
    return torch.stack([pick(1), pick(0)]), torch.stack([pick(-1), pick(-2)])


# (N, D, k) of the GPU file: the smallest that reach each path, from _knn_cases' lists
SMALL_SHAPES = [(763, 256, 4), (1500, 128, 13), (33, 64, 16)]
RECT_SHAPES = [(1536, 256, 4), (1536, 256, 40), (2048 + 37, 256, 13)]
TRI_SHAPES = [(24576 + 128 + 37, 256, 4)]
BIG_SHAPES = [(49152 + 300, 256, 4), (49152 + 300, 64, 4)]
EXACT_ROWS_SHAPE = (40960 + 37, 256, 64)
INF_SHAPES = [(763, 256, 4), (1536, 256, 4), (1536, 256, 40), (24576 + 128 + 37, 256, 4), (49152 + 300, 256, 4)]
for _s in SMALL_SHAPES:
    assert _s in K.SMALL_SHAPES
for _s in RECT_SHAPES + TRI_SHAPES + BIG_SHAPES + [EXACT_ROWS_SHAPE]:
    assert _s in K.SCREEN_SHAPES


# ---------------------------------------------------------------------------------------------------------------------
class Counting:
    """`ops._T` with calls of `knn_cosine_topk` counted."""

    def __init__(self, inner):
        self._inner, self.calls = inner, 0

    def __getattr__(self, name):
        f = getattr(self._inner, name)
        if name != "knn_cosine_topk":
            return f

        def counted(*a):
            self.calls += 1
            return f(*a)
        return counted


FEATGRAPH = ["n64_k4", "n200_k4", "n200_d256_k13", "zero_row", "clamp", "clamp2"]
FEATGRAPH_SHAPES = dict(n64_k4=(64, 64, 4, (True, False)), n200_k4=(200, 64, 4, (True,)), n200_d256_k13=(200, 256, 13, (True,)),
                        zero_row=(64, 64, 4, (False,)), clamp=(5, 64, 4, (True, False)), clamp2=(3, 64, 20, (True, False)))


def compare_with_fixture(name, build):
    """`build(features, k, symm)` -> sparse COO; after coalesce() on both sides the same indices and bit-equal fp32 values
    as the reference's tensor.  The zero row of `zero_row` (neighbours an arbitrary choice among ties) by structure only,
    on both sides: k_actual distinct unit entries plus the diagonal, over a row sum of k_actual + 1 — when it chose itself
    the diagonal entry counts 2 and there are k_actual entries, the sum is the same."""
    g = C.load("featgraph_" + name)
    N, D, k, symms = FEATGRAPH_SHAPES[name]
    x = torch.from_numpy(g["features"])
    assert tuple(x.shape) == (N, D) and x.dtype == torch.float32 and int(g["k"]) == k and tuple(g["symm"].tolist()) == symms
    k_actual = min(k, N - 1)
    zero = [int(r) for r in (x == 0).all(dim=1).nonzero().reshape(-1)]
    assert zero == ([17] if name == "zero_row" else [])
    for symm in symms:
        want = torch.sparse_coo_tensor(torch.from_numpy(g["idx_%d" % symm]), torch.from_numpy(g["val_%d" % symm]), (N, N)).coalesce()
        got = build(x, k, symm).coalesce().cpu()
        assert got.dtype == torch.float32 and tuple(got.shape) == (N, N)
        gi, gv, wi, wv = got.indices(), got.values(), want.indices(), want.values()
        keep_g, keep_w = torch.ones(gi.shape[1], dtype=torch.bool), torch.ones(wi.shape[1], dtype=torch.bool)
        for z in zero:
            assert not symm
            for idx, val, keep in ((gi, gv, keep_g), (wi, wv, keep_w)):
                mine = idx[0] == z
                cols = idx[1][mine].tolist()
                keep &= ~mine
                chose_itself = len(cols) == k_actual                 # its own id among the k_actual: merged with + I
                assert len(cols) == (k_actual if chose_itself else k_actual + 1) and z in cols and len(set(cols)) == len(cols)
                total = np.float64(k_actual + 1)
                for c, v in zip(cols, val[mine].tolist()):
                    m = 2.0 if (chose_itself and c == z) else 1.0
                    assert np.float32(v) == np.float32(np.float64(m) / total), (z, c, v)
        assert torch.equal(gi[:, keep_g], wi[:, keep_w])
        assert torch.equal(gv[keep_g].view(torch.int32), wv[keep_w].view(torch.int32))
