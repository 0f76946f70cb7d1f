"""The attention fusion's contract (``include/dgmi_attn.h``) restated in float64 numpy, and the operand designs of its tests.

``reference`` is the contract, line by line.  ``exact_design`` makes operands on which fp32 is exact in ANY order of
summation, so a kernel must EQUAL the restatement rounded to fp32; ``float_design`` draws operands the way the model
meets them, or with scaled weights that saturate ``tanh`` and the softmax; ``block_partials`` is what each block of rows
adds to the three parameter sums; ``poison`` / ``classes`` / ``restate`` are the designs with one non-finite element."""
import numpy as np

HIDDEN = 16
PRE_UNIT = 32     # every pre-activation is a multiple of this: 0, or tanh saturates to +-1 in fp32 AND in float64
SCORE_UNIT = 128  # every s_0 - s_1 is a multiple of this: 0, or the softmax is (1, 0) / (0, 1) in fp32
ACTIVE_ROWS = 30000  # about this many rows of a design carry parameter gradients (keeps every sum exact, see exact_bound)


def reference(A, B, W1, b1, w2, M, g):
    """All seven outputs in float64: out, beta (after the multiplier), dA, dB, dW1, db1, dw2."""
    A, B, W1, b1, w2, g = (np.asarray(t, dtype=np.float64) for t in (A, B, W1, b1, w2, g))
    n = A.shape[0]
    Mx = np.ones((n, 2)) if M is None else np.asarray(M, dtype=np.float64)
    z = np.stack([A, B], 1)                                   # (n, 2, F)
    h = np.tanh(z @ W1.T + b1)                                # (n, 2, 16)
    s = h @ w2.reshape(-1)                                    # (n, 2)
    e = np.exp(s - s.max(1, keepdims=True)) if n else s
    beta = e / e.sum(1, keepdims=True) if n else s
    bp = beta * Mx
    out = bp[:, 0, None] * A + bp[:, 1, None] * B
    dbp = np.einsum("nf,ncf->nc", g, z)
    db = Mx * dbp
    ds = beta * (db - (beta * db).sum(1, keepdims=True))
    dpre = ds[:, :, None] * w2.reshape(1, 1, -1) * (1.0 - h * h)
    dz = bp[:, :, None] * g[:, None, :] + dpre @ W1
    return {"out": out, "beta": bp, "dA": dz[:, 0], "dB": dz[:, 1], "dW1": np.einsum("nch,ncf->hf", dpre, z),
            "db1": dpre.sum((0, 1)), "dw2": np.einsum("nc,nch->h", ds, h)}


OUTPUTS = ("out", "beta", "dA", "dB", "dW1", "db1", "dw2")


def _hidden(z, W1, b1):
    pre = z @ W1.T + b1
    return pre, np.sign(pre)  # tanh of a multiple of PRE_UNIT, in fp32


def exact_design(n_rows, F, mult=False, seed=0):
    """Integer operands ``dict(A, B, W1, b1, w2, M, g)`` (float32 arrays, ``M`` None without ``mult``) with

    * ``W1`` in {0, +-32}, ``b1`` in {0, +-32}, ``A`` / ``B`` in {-1, 0, 1}: every pre-activation is a multiple of 32, so
      ``h`` is 0 or +-1 exactly;
    * ``w2`` = +-128: every ``s_0 - s_1`` is a multiple of 128, so ``beta`` is (1/2, 1/2), (1, 0) or (0, 1) exactly;
    * row ``i`` of class ``i % 3`` (equal / first / second channel); ``M`` cycles (2, 2), (0, 2), (2, 0), (0, 0);
    * gradients reach the parameters only through rows with equal scores, a zero pre-activation and ``h_0 != h_1``;
      about ``ACTIVE_ROWS`` of those (the first and the last ones always) get a one-hot ``g`` on a column where the two
      channels differ, so ``ds`` is a multiple of 1/4 with ``|ds| <= 1``; the other equal-score rows get ``g = 0`` and
      every other row a dense ``g`` in {-1, 0, 1}.
    ``exact_bound`` is the largest sum of absolute terms of any output of the design."""
    rng = np.random.default_rng(1000003 * F + seed)
    k = np.arange(HIDDEN)[:, None]
    f = np.arange(F)[None, :]
    pattern = (f % HIDDEN == k) | (rng.random((HIDDEN, F)) < 0.125)
    W1 = PRE_UNIT * np.where(pattern, rng.choice([-1.0, 1.0], size=(HIDDEN, F)), 0.0)
    b1 = PRE_UNIT * rng.choice([-1.0, 0.0, 1.0], size=HIDDEN)
    w2 = SCORE_UNIT * rng.choice([-1.0, 1.0], size=HIDDEN)

    # a pool of rows, by class
    P = 8192
    z = rng.choice([-1.0, 0.0, 0.0, 1.0], size=(P, 2, F))
    pre, h = _hidden(z, W1, b1)
    s = h @ w2
    differ = (z[:, 0] != z[:, 1]).any(1)
    useful = (s[:, 0] == s[:, 1]) & (pre == 0).any((1, 2)) & (h[:, 0] != h[:, 1]).any(1) & differ
    pools = [np.flatnonzero(useful), np.flatnonzero(s[:, 0] > s[:, 1]), np.flatnonzero(s[:, 0] < s[:, 1])]
    assert all(len(p) > 0 for p in pools), [len(p) for p in pools]

    i = np.arange(n_rows)
    cls = i % 3
    pick = np.empty(n_rows, dtype=np.int64)
    for c in range(3):
        pick[cls == c] = pools[c][(i[cls == c] // 3) % len(pools[c])]
    Z = z[pick]
    A, B = Z[:, 0].copy(), Z[:, 1].copy()

    g = rng.choice([-1.0, 0.0, 1.0], size=(n_rows, F))
    equal = cls == 0
    active = equal & ((rng.random(n_rows) < ACTIVE_ROWS / max(n_rows / 3.0, 1.0)) | (i < 24) | (i >= n_rows - 24))
    g[equal] = 0.0
    for r in np.flatnonzero(active):
        cols = np.flatnonzero(A[r] != B[r])
        g[r, cols[rng.integers(len(cols))]] = rng.choice([-1.0, 1.0])
    M = None
    if mult:
        M = np.array([[2.0, 2.0], [0.0, 2.0], [2.0, 0.0], [0.0, 0.0]])[i % 4]
    f32 = lambda t: None if t is None else np.ascontiguousarray(t, dtype=np.float32)
    return {"A": f32(A), "B": f32(B), "W1": f32(W1), "b1": f32(b1), "w2": f32(w2), "M": f32(M), "g": f32(g)}


def exact_classes(d):
    """``(pre, s)`` of a design in float64: the multiples the design promises."""
    z = np.stack([d["A"], d["B"]], 1).astype(np.float64)
    pre, h = _hidden(z, d["W1"].astype(np.float64), d["b1"].astype(np.float64))
    return pre, h @ d["w2"].astype(np.float64)


def exact_bound(d):
    """The largest sum of ABSOLUTE terms over all sums the contract forms on design ``d`` (so any order and any fused
    multiply-add is exact in fp32 while 8 x this stays below 2^24)."""
    A, B, W1, b1, w2, g = (d[k].astype(np.float64) for k in ("A", "B", "W1", "b1", "w2", "g"))
    n = A.shape[0]
    M = np.ones((n, 2)) if d["M"] is None else d["M"].astype(np.float64)
    z = np.stack([A, B], 1)
    r = reference(A, B, W1, b1, w2, d["M"], g)
    pre_abs = np.abs(z) @ np.abs(W1).T + np.abs(b1)
    h = np.sign(z @ W1.T + b1)
    s_abs = np.abs(h) @ np.abs(w2)
    beta = np.abs(r["beta"])
    out_abs = beta[:, 0, None] * np.abs(A) + beta[:, 1, None] * np.abs(B)
    dbp_abs = np.einsum("nf,ncf->nc", np.abs(g), np.abs(z)) * M
    # ds and dpre from the reference's own values: recompute them
    e = np.exp((h @ w2) - (h @ w2).max(1, keepdims=True))
    b = e / e.sum(1, keepdims=True)
    db = M * np.einsum("nf,ncf->nc", g, z)
    ds = b * (db - (b * db).sum(1, keepdims=True))
    ds[np.abs(ds) < 1e-30] = 0.0
    dpre = np.abs(ds[:, :, None] * w2 * (1.0 - h * h))
    dz_abs = beta[:, :, None] * np.abs(g)[:, None, :] + dpre @ np.abs(W1)
    sums = [pre_abs.max(), s_abs.max(), out_abs.max(), dbp_abs.max() * 2, dz_abs.max(),
            np.einsum("nch,ncf->hf", dpre, np.abs(z)).max(), dpre.sum((0, 1)).max(),
            np.einsum("nc,nch->h", np.abs(ds), np.abs(h)).max()]
    return float(max(sums)) if n else 0.0


def float_design(n_rows, F, seed, w1_scale=1, w2_scale=1):
    """``W1``, ``b1``, ``w2`` as ``nn.Linear`` initialises them (uniform in +-1 / sqrt(fan_in)), ``A ~ N(0, 1)``,
    ``B ~ 0.5 N(0, 1)``, ``g ~ N(0, 1)``, ``M`` a ``p = 0.5`` dropout multiplier (0 or 2).  ``w1_scale`` multiplies
    ``W1`` and ``b1`` and ``w2_scale`` multiplies ``w2`` (the same draws; 1 changes nothing): larger weights leave the
    linear regime, so ``tanh`` and the softmax saturate and the backward's two cancellations carry the error."""
    rng = np.random.default_rng(seed)
    k1, k2 = 1.0 / np.sqrt(F), 1.0 / np.sqrt(HIDDEN)
    f32 = lambda t: np.ascontiguousarray(t, dtype=np.float32)
    return {"A": f32(rng.standard_normal((n_rows, F))), "B": f32(0.5 * rng.standard_normal((n_rows, F))),
            "W1": f32(w1_scale * rng.uniform(-k1, k1, (HIDDEN, F))), "b1": f32(w1_scale * rng.uniform(-k1, k1, HIDDEN)),
            "w2": f32(w2_scale * rng.uniform(-k2, k2, HIDDEN)), "M": f32(2.0 * (rng.random((n_rows, 2)) < 0.5)),
            "g": f32(rng.standard_normal((n_rows, F)))}


def regime(d):
    """Where a float design sits, from the float64 restatement without the multiplier: the share of rows whose smaller
    weight is below 1e-3, the share of hidden units with ``|h| > 0.99``, and the smallest weight rounded to fp32."""
    z = np.stack([d["A"], d["B"]], 1).astype(np.float64)
    h = np.tanh(z @ d["W1"].astype(np.float64).T + d["b1"].astype(np.float64))
    beta = reference(d["A"], d["B"], d["W1"], d["b1"], d["w2"], None, d["g"])["beta"]
    return float((beta.min(1) < 1e-3).mean()), float((np.abs(h) > 0.99).mean()), float(beta.astype(np.float32).min())


BLOCK_ROWS = 64  # DGMI_ATTN_BLOCK_ROWS (test_attention_host.py holds it to the header)


def block_partials(d):
    """The restatement restricted to each block of ``BLOCK_ROWS`` rows, rounded to fp32: ``dW1`` (blocks, 16, F), ``db1``
    and ``dw2`` (blocks, 16), what each block adds to the three parameter sums."""
    n = d["A"].shape[0]
    parts = {"dW1": [], "db1": [], "dw2": []}
    for lo in range(0, n, BLOCK_ROWS):
        rows = slice(lo, min(lo + BLOCK_ROWS, n))
        r = reference(d["A"][rows], d["B"][rows], d["W1"], d["b1"], d["w2"], None if d["M"] is None else d["M"][rows], d["g"][rows])
        for k in parts:
            parts[k].append(r[k].astype(np.float32))
    return {k: np.stack(v) for k, v in parts.items()}


# ---------------------------------------------------------------------------------------------------------------------
# poisoned designs: one element of one operand replaced
FINITE, NAN, POS_INF, NEG_INF = 0, 1, 2, 3


def poison(d, operand, row, col, value):
    """A copy of design ``d`` with ``d[operand][row, col] = value`` (``operand`` one of A, B, g, M)."""
    e = dict(d)
    e[operand] = d[operand].copy()
    e[operand][row, col] = value
    return e


def classes(t):
    """Per element: ``FINITE``, ``NAN``, ``POS_INF`` or ``NEG_INF`` (int8, the shape of ``t``)."""
    t = np.asarray(t)
    c = np.zeros(t.shape, dtype=np.int8)
    c[np.isnan(t)] = NAN
    c[np.isposinf(t)] = POS_INF
    c[np.isneginf(t)] = NEG_INF
    return c


def restate(d, dtype=np.float64, reverse=False):
    """``reference`` on design ``d`` carried out in ``dtype``, with the columns (the index of every sum over the width)
    in reverse order when ``reverse`` is set: the same contract, other roundings and another order of summation."""
    A, B, W1, b1, w2, g = (np.asarray(d[k], dtype=dtype) for k in ("A", "B", "W1", "b1", "w2", "g"))
    if reverse:
        A, B, W1, g = A[:, ::-1], B[:, ::-1], W1[:, ::-1], g[:, ::-1]
    n = A.shape[0]
    Mx = np.ones((n, 2), dtype=dtype) if d["M"] is None else np.asarray(d["M"], dtype=dtype)
    one = dtype(1)
    with np.errstate(all="ignore"):
        z = np.stack([A, B], 1)
        h = np.tanh(np.einsum("ncf,hf->nch", z, W1) + b1)
        s = np.einsum("nch,h->nc", h, w2)
        e = np.exp(s - s.max(1, keepdims=True))
        beta = e / e.sum(1, keepdims=True)
        bp = beta * Mx
        out = bp[:, 0, None] * A + bp[:, 1, None] * B
        db = Mx * np.einsum("nf,ncf->nc", g, z)
        ds = beta * (db - (beta * db).sum(1, keepdims=True))
        dpre = ds[:, :, None] * w2.reshape(1, 1, -1) * (one - h * h)
        dz = bp[:, :, None] * g[:, None, :] + np.einsum("nch,hf->ncf", dpre, W1)
        r = {"out": out, "beta": bp, "dA": dz[:, 0], "dB": dz[:, 1], "dW1": np.einsum("nch,ncf->hf", dpre, z),
             "db1": dpre.sum((0, 1)), "dw2": np.einsum("nc,nch->h", ds, h)}
    if reverse:
        for k in ("out", "dA", "dB", "dW1"):
            r[k] = r[k][:, ::-1]
    return r


POISON_SHAPE = (200, 132, 5)   # rows, width, seed of the unscaled float design: fourth block ragged, last j ragged
POISON_ROWS = (0, 15, 16, 63, 64, 199)
POISON_COLS = {"A": (0, 131), "B": (0, 131), "g": (0, 131), "M": (0, 1)}
POISON_VALUES = {"A": (np.nan, np.inf, -np.inf, 3.0), "B": (np.nan, np.inf, -np.inf, 3.0), "g": (np.nan, np.inf, -np.inf, 3.0),
                 "M": (np.nan, np.inf, -np.inf)}


def poison_cases():
    """``(operand, row, col, value)``: every listed row with every listed column for every operand, the values in turn."""
    out = []
    for operand in ("A", "B", "g", "M"):
        values = POISON_VALUES[operand]
        for ri, row in enumerate(POISON_ROWS):
            for ci, col in enumerate(POISON_COLS[operand]):
                out.append((operand, row, col, values[(2 * ri + ci) % len(values)]))
    return out


#: elements of a poisoned design's outputs whose class depends on rounding or on the order of summation (the three
#: restatements of ``class_disagreements`` differ there): ``{(operand, row, col, repr(value)): {output: [index, ...]}}``.
#: The host test holds this table to what it computes; the GPU test skips exactly these elements in its class check.
POISON_LEFT_OUT = {}


def class_disagreements(d):
    """``{output: boolean mask}`` of the elements where the class map of the float64 restatement differs from that of the
    fp32 restatement or from that of the float64 restatement with the columns reversed."""
    base = restate(d)
    others = (restate(d, np.float32), restate(d, np.float64, reverse=True))
    return {k: np.logical_or.reduce([classes(o[k]) != classes(base[k]) for o in others]) for k in OUTPUTS}
