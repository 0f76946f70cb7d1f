"""Designs and restatements for the fused training decoder (``ops.pair_mlp_train``): the dropout mask of
``csrc/dgmi_pair_dropout.h`` in numpy, integer designs whose every sum is exact in fp32 in any order, and the float64
restatement of logits and gradients (with the absolute-value twin that the elementwise bar is taken from)."""
import math

import numpy as np

H1, H2 = 128, 64
M64 = (1 << 64) - 1
M32 = 0xFFFFFFFF
EXACT_SIZES = (1, 33, 129, 385, 40_000)


# ---------------------------------------------------------------------------------------------------------------------
# the mask function
def mix64(z):
    z = (z + 0x9E3779B97F4A7C15) & M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
    return z ^ (z >> 31)


def layer_key(seed, layer):
    return mix64((mix64(int(seed) & M64) + layer) & M64)


def hash32(seed, layer, e, j):
    """The 32-bit hash of element (e, j) of ``layer`` (broadcasts over numpy arrays)."""
    k = layer_key(seed, layer)
    lo, hi = k & M32, k >> 32
    x = (np.asarray(e, dtype=np.uint64) & M32) ^ np.uint64(lo)
    x ^= x >> np.uint64(16)
    x = (x * np.uint64(0x85EBCA6B)) & np.uint64(M32)
    x ^= x >> np.uint64(13)
    x = (x * np.uint64(0xC2B2AE35)) & np.uint64(M32)
    x ^= x >> np.uint64(16)
    x = (x + np.uint64(hi) + np.asarray(j, dtype=np.uint64) * np.uint64(0x9E3779B9)) & np.uint64(M32)
    x ^= x >> np.uint64(16)
    x = (x * np.uint64(0x7FEB352D)) & np.uint64(M32)
    x ^= x >> np.uint64(15)
    x = (x * np.uint64(0x846CA68B)) & np.uint64(M32)
    x ^= x >> np.uint64(16)
    return x


def threshold(p):
    """floor((1 - p) 2^32) with p as the fp32 the C ABI takes; 2^32 means "keep all"."""
    return int(math.floor((1.0 - float(np.float32(p))) * 4294967296.0))


def scale(p):
    return np.float32(1.0 / (1.0 - float(np.float32(p))))


def keep(seed, layer, e, j, p):
    thr = threshold(p)
    h = hash32(seed, layer, e, j)
    if thr > M32:
        return np.ones(h.shape, dtype=bool)
    return h < np.uint64(thr)


def masks(seed, E, p):
    """(m1, m2): bool (E, 128) and (E, 64), keyed by the list position."""
    e = np.arange(E, dtype=np.uint64)[:, None]
    return (keep(seed, 1, e, np.arange(H1, dtype=np.uint64)[None, :], p),
            keep(seed, 2, e, np.arange(H2, dtype=np.uint64)[None, :], p))


# ---------------------------------------------------------------------------------------------------------------------
# the float64 restatement
def reference(P, Q, W2, b2, w3, b3, src, dst, p, seed, g, absolute=False, form="product", open_gates=False):
    """Logits and every gradient in float64 with the restated masks.  ``absolute=True``: the same expressions on the
    absolute values of every operand, with the gates (masks, relu) of the true computation: sum|terms|.

    ``form``: how a gate meets a value.  ``"product"`` multiplies by the 0 / scale factor, as the torch chain does;
    ``"select"`` is the kernels' contract (include/dgmi_train.h): a unit whose gate is closed is exactly 0 whatever lies
    under it, an open one is ``value * scale`` under IEEE rules (relu keeps NaN, ``relu(+Inf) = +Inf``, the backward's
    relu gate ``[z > 0]`` is false for NaN).  On finite operands the two forms are the same bits.

    ``open_gates=True`` (with ``absolute``): every mask and relu gate open, which bounds sum|terms| under ANY seed."""
    if form not in ("product", "select"):
        raise ValueError(form)
    P, Q, W2, b2, w3, g = (np.asarray(a, dtype=np.float64) for a in (P, Q, W2, b2, w3, g))
    b3 = float(np.asarray(b3, dtype=np.float64).reshape(-1)[0])
    w3 = w3.reshape(-1)
    E = len(src)
    m1, m2 = masks(seed, E, p)
    s = float(scale(p))
    if form == "select":
        gated = lambda x, gate: np.where(gate, x * s, 0.0)  # noqa: E731
    else:
        gated = lambda x, gate: x * (gate * s)  # noqa: E731
    with np.errstate(invalid="ignore"):  # Inf - Inf and 0 * Inf are NaN on purpose
        z1 = P[src] + Q[dst]
        h1 = gated(np.maximum(z1, 0.0), m1)
        z2 = h1 @ W2.T + b2
        gate1, gate2 = m1 & (z1 > 0), m2 & (z2 > 0)
        if open_gates:
            if not absolute:
                raise ValueError("open_gates bounds the absolute form only")
            gate1, gate2, m1, m2 = (np.ones_like(x) for x in (gate1, gate2, m1, m2))
        if absolute:
            P, Q, W2, b2, w3, g, b3 = np.abs(P), np.abs(Q), np.abs(W2), np.abs(b2), np.abs(w3), np.abs(g), abs(b3)
            h1 = gated(P[src] + Q[dst], gate1)
            z2 = h1 @ W2.T + b2
        h2 = gated(z2, gate2) if absolute else gated(np.maximum(z2, 0.0), m2)
        out = {"logit": h2 @ w3 + b3, "z2": z2}
        dz2 = gated(g[:, None] * w3[None, :], gate2)
        dz1 = gated(dz2 @ W2, gate1)
        out["dW2"], out["db2"], out["dw3"], out["db3"] = dz2.T @ h1, dz2.sum(0), (g[:, None] * h2).sum(0), np.array([g.sum()])
    out["dz1"] = dz1
    out["dP"], out["dQ"] = np.zeros_like(P), np.zeros_like(Q)
    np.add.at(out["dP"], src, dz1)
    np.add.at(out["dQ"], dst, dz1)
    return out


GRADS = ("dP", "dQ", "dW2", "db2", "dw3", "db3")
MODULE_GRADS = ("dhd", "dhs", "dW1", "db1")


def ref_of(d, p, seed, g=None, **kw):
    """``reference`` on a design's operands (``g``: another upstream gradient than the design's)."""
    return reference(d["P"], d["Q"], d["W2"], d["b2"], d["w3"], d["b3"], d["src"], d["dst"], p, seed,
                     d["g"] if g is None else g, **kw)


# ---------------------------------------------------------------------------------------------------------------------
# designs
def pair_list(rng, E, n_src, n_dst):
    """A list with a source node that has no pair (1), one that has a quarter of the list, up to 3000 pairs (0), and
    duplicated pairs (the first eighth of the list again at its end)."""
    src = rng.integers(2, n_src, size=E)
    dst = rng.integers(0, n_dst, size=E)
    d = E // 8
    src[rng.permutation(E - d)[:min(E // 4, 3000)]] = 0
    if d:
        src[E - d:], dst[E - d:] = src[:d], dst[:d]
    return src.astype(np.int64), dst.astype(np.int64)


def exact_design(E, seed=0):
    """Integer operands: P, Q in [-3, 3], W2, w3 in [-2, 2], biases in [-2, 2], upstream gradient in [-2, 2].  Layer-1
    unit 5 is never positive and unit 6 always; layer-2 unit 3 is never positive and unit 4 always (zero W2 rows, biases
    -1 / +2).  With p = 0.5 (scale 2) every term and every sum of absolute terms stays below 2^24 (checked by
    ``exact_margin``), so fp32 is exact in any order."""
    rng = np.random.default_rng(1000 + E + seed)
    n_src, n_dst = 37, 29
    P = rng.integers(-3, 4, size=(n_src, H1)).astype(np.float32)
    Q = rng.integers(-3, 4, size=(n_dst, H1)).astype(np.float32)
    P[:, 5], Q[:, 5] = -rng.integers(1, 4, size=n_src), -rng.integers(0, 4, size=n_dst)
    P[:, 6], Q[:, 6] = rng.integers(1, 4, size=n_src), rng.integers(0, 4, size=n_dst)
    W2 = rng.integers(-2, 3, size=(H2, H1)).astype(np.float32)
    b2 = rng.integers(-2, 3, size=H2).astype(np.float32)
    W2[3], W2[4], b2[3], b2[4] = 0, 0, -1, 2
    w3 = rng.integers(-2, 3, size=(1, H2)).astype(np.float32)
    w3[0, 3], w3[0, 4] = 2, -1
    b3 = rng.integers(-2, 3, size=1).astype(np.float32)
    src, dst = pair_list(rng, E, n_src, n_dst)
    g = rng.integers(-2, 3, size=E).astype(np.float32)
    return dict(P=P, Q=Q, W2=W2, b2=b2, w3=w3, b3=b3, src=src, dst=dst, g=g, n_src=n_src, n_dst=n_dst)


def exact_margin(d, p, seed, g=None):
    """The largest sum of absolute terms over all outputs of a design: below 2^24 means exact in fp32, in any order.
    A module design (``module_design``) adds the two ``lin1`` tables and the four gradients behind them.  ``seed=None``:
    with every gate open, a bound for any seed."""
    kw = dict(absolute=True, open_gates=seed is None)
    seed = 0 if seed is None else seed
    if "hd" in d:
        a = module_reference(d, p, seed, g=g, **kw)
        return max(float(np.max(a[k])) for k in ("P", "Q", "logit", "z2") + GRADS + MODULE_GRADS)
    a = ref_of(d, p, seed, g, **kw)
    return max(float(np.max(a[k])) for k in ("logit", "z2") + GRADS)


# ---------------------------------------------------------------------------------------------------------------------
# the module route: P = hd Wa^T + b1, Q = hs Wb^T in front of the fused op
MODULE_F = 8


def module_design(E, seed=0):
    """Integer embeddings ``hd`` (37 x 8), ``hs`` (29 x 8) in [-2, 2], ``lin1.weight`` (128 x 16) in [-1, 1] with
    density 0.4, ``lin1.bias`` in [-1, 1]; ``lin2`` / ``lin3``, the pair list and the upstream gradient as in
    ``exact_design``.  Every operand is a bf16 number, so a GEMM library may round its inputs to bf16 / TF32 and still
    be exact as long as it accumulates in fp32 (the GPU test asserts that on these very operands).  ``P`` / ``Q`` are the
    exact tables."""
    rng = np.random.default_rng(2000 + E + seed)
    d = exact_design(E, seed)
    n_src, n_dst, F = d["n_src"], d["n_dst"], MODULE_F
    d["hd"] = rng.integers(-2, 3, size=(n_src, F)).astype(np.float32)
    d["hs"] = rng.integers(-2, 3, size=(n_dst, F)).astype(np.float32)
    d["W1"] = (rng.integers(-1, 2, size=(H1, 2 * F)) * (rng.random((H1, 2 * F)) < 0.4)).astype(np.float32)
    d["b1"] = rng.integers(-1, 2, size=H1).astype(np.float32)
    P, Q = module_tables(d)
    d["P"], d["Q"] = P.astype(np.float32), Q.astype(np.float32)
    assert np.array_equal(d["P"], P) and np.array_equal(d["Q"], Q)
    return d


def module_tables(d, absolute=False):
    hd, hs, W1, b1 = (np.asarray(d[k], dtype=np.float64) for k in ("hd", "hs", "W1", "b1"))
    if absolute:
        hd, hs, W1, b1 = np.abs(hd), np.abs(hs), np.abs(W1), np.abs(b1)
    F = hd.shape[1]
    return hd @ W1[:, :F].T + b1, hs @ W1[:, F:].T


def module_reference(d, p, seed, absolute=False, g=None, open_gates=False):
    """The float64 restatement of ``MLPDecoder.forward`` on the fused route: the two ``lin1`` tables, ``reference`` on
    them, and the chain rule back to ``hd``, ``hs``, ``lin1.weight`` and ``lin1.bias``.  ``absolute=True``: sum|terms| of
    every stage on the absolute values of ITS operands (the tables' own sums as ``P`` / ``Q``; the gradient stages on
    the absolute-value ``dP`` / ``dQ``, which bound the true ones)."""
    P, Q = module_tables(d)
    r = reference(P, Q, d["W2"], d["b2"], d["w3"], d["b3"], d["src"], d["dst"], p, seed, d["g"] if g is None else g,
                  absolute=absolute, open_gates=open_gates)
    hd, hs, W1 = (np.asarray(d[k], dtype=np.float64) for k in ("hd", "hs", "W1"))
    if absolute:
        hd, hs, W1 = np.abs(hd), np.abs(hs), np.abs(W1)
        r["P"], r["Q"] = module_tables(d, absolute=True)
    F = hd.shape[1]
    r["dhd"], r["dhs"] = r["dP"] @ W1[:, :F], r["dQ"] @ W1[:, F:]
    r["dW1"] = np.concatenate([r["dP"].T @ hd, r["dQ"].T @ hs], 1)
    r["db1"] = r["dP"].sum(0)
    return r


# ---------------------------------------------------------------------------------------------------------------------
# non-finite rows
NONFINITE_E = 129
NF_NAN_ONE, NF_NAN_ROW, NF_NEG_INF = 7, 9, 11   # source nodes: NaN in one column, a row of NaN, -Inf in one column
NF_DST = 4                                      # destination node: +Inf in NF_COL_INF, -Inf in NF_COL_NEG
NF_COL_NAN, NF_COL_INF, NF_COL_NEG = 17, 22, 21


def nonfinite_design(E=NONFINITE_E):
    """``exact_design(E)`` with non-finite rows.  Source node 7 holds a NaN in column 17, source node 9 is all NaN,
    destination node 4 holds +Inf in column 22 and -Inf in column 21, source node 11 holds -Inf in column 22: listed
    against node 4 its column 22 is ``-Inf + Inf = NaN``, against a finite row ``-Inf`` (relu: 0).  Each of them is
    written into the list at several positions of both waves' halves, so that under one mask the non-finite unit is
    kept at some positions and dropped at others (asserted on the host).  ``touch``: the positions that name one of
    these nodes; ``g`` is 0 there.  ``finite``: the same design with the non-finite rows replaced by zeros."""
    d = exact_design(E)
    src, dst = d["src"].copy(), d["dst"].copy()
    dst[dst == NF_DST] = NF_DST + 1
    for s in (NF_NAN_ONE, NF_NAN_ROW, NF_NEG_INF):
        src[src == s] = s + 1
    at = lambda *pos: np.array([q for q in pos if q < E], dtype=np.int64)  # noqa: E731
    src[at(1, 30, 33, 63, 70, 100, 127, 128)] = NF_NAN_ONE
    src[at(2, 34, 90)] = NF_NAN_ROW
    dst[at(3, 31, 35, 64, 65, 96, 110, 120)] = NF_DST
    both = at(5, 40, 66, 97, 111)
    src[both], dst[both] = NF_NEG_INF, NF_DST
    src[at(6, 41)] = NF_NEG_INF
    P, Q = d["P"].copy(), d["Q"].copy()
    rows_p, rows_q = [NF_NAN_ONE, NF_NAN_ROW, NF_NEG_INF], [NF_DST]
    fin = dict(d, src=src, dst=dst, P=P.copy(), Q=Q.copy())
    fin["P"][rows_p], fin["Q"][rows_q] = 0, 0
    P[NF_NAN_ONE, NF_COL_NAN] = np.nan
    P[NF_NAN_ROW] = np.nan
    P[NF_NEG_INF, NF_COL_INF] = -np.inf
    Q[NF_DST, NF_COL_INF], Q[NF_DST, NF_COL_NEG] = np.inf, -np.inf
    touch = np.isin(src, rows_p) | np.isin(dst, rows_q)
    g = np.where(touch, 0, d["g"]).astype(np.float32)
    fin["g"] = g
    return dict(d, P=P, Q=Q, src=src, dst=dst, g=g, touch=touch, finite=fin)


def float_design(E=5000, seed=7, settle=None):
    """Random fp32 operands.  ``settle=(p, mask_seed)``: list positions where some ``|z2|`` is within ``2e-4 sum|terms|``
    of zero under that mask get another pair, until none is left: a relu that float64 and fp32 could take differently
    is a property of the inputs, not an error of either."""
    rng = np.random.default_rng(seed)
    n_src, n_dst = 61, 43
    f = lambda *s: rng.standard_normal(s).astype(np.float32)  # noqa: E731
    src, dst = pair_list(rng, E, n_src, n_dst)
    d = dict(P=f(n_src, H1), Q=f(n_dst, H1), W2=(f(H2, H1) / np.float32(8)), b2=f(H2), w3=f(1, H2), b3=f(1), src=src,
             dst=dst, g=f(E), n_src=n_src, n_dst=n_dst)
    while settle is not None:
        a = (d["P"], d["Q"], d["W2"], d["b2"], d["w3"], d["b3"], d["src"], d["dst"], settle[0], settle[1], d["g"])
        close = np.abs(reference(*a)["z2"]) <= 2e-4 * reference(*a, absolute=True)["z2"]
        bad = np.nonzero(close.any(1))[0]
        if not len(bad):
            break
        d["src"][bad], d["dst"][bad] = rng.integers(2, n_src, len(bad)), rng.integers(0, n_dst, len(bad))
    return d
