"""The fused attention fusion where its first suite (``test_gpu_attention.py``) does not look.  Exact cases are ZERO
tolerance against the float64 restatement rounded to fp32, all seven outputs, with and without the multiplier:

1. every width class with live partials: 200 rows (all four blocks add to dW1, db1 and dw2; ``test_attention_host.py``)
   on both sides of each ``by_width`` switch and with a ragged last ``j`` in every instantiation, and R G + 2 R + 3 rows
   at F = 32 and 260, where workgroups 0 to 2 carry their accumulators into a second, contributing block;
2. the reduce kernel at 15, 16, 17, 240, 241, 255, 256, 257 and 1023 partials;
3. the C ABI on buffers the test owns: six different leading dimensions, NaN in every spare column and guard row of the
   inputs, sentinels in every spare column and guard row of the outputs, around the small outputs and behind a workspace
   of exactly ``dgmi_attn_fuse_workspace_bytes``;
4. one poisoned element (NaN, +-Inf, a finite 3.0) in A, B, g or M at tile, block and width edges: every other row keeps
   the BITS of the clean run, the class map is the restatement's;
5. saturating weights (``float_design(..., w1_scale=4, w2_scale=8)``) under the accuracy rule of the first suite;
6. operand forms through ``ops.attention_fuse``: bit-identical to the contiguous call;
7. ``model.Attention`` on the device: the fall-backs take the chain bit for bit, the dropout rate is the module's
   current one, ``p = 1``, ``fuse(x, x)``, ``n = 0``.

Measured on one MI355X (item 5, ``max|T_fused - T_64| / (4 max|T_chain - T_64| + 2^-22 max|T_64|)``, bound 1): between
0.205 and 0.405 over the seven outputs at (763, 128), between 0.219 and 0.689 at (1256, 256), the largest on ``dB``
(``SATURATED_RATIOS`` below, the table in DESIGN.md 4.16); the file prints every ratio (``-s``).  The whole file: 87
cases, 8.0 s."""
import numpy as np
import pytest
import torch

import _attention_cases as K
import test_gpu_attention as T

pytestmark = pytest.mark.gpu

#: item 5 as measured on one MI355X (a record, not a bound): the ratio to the bound of each of the seven outputs
SATURATED_RATIOS = {
    (763, 128): dict(out=0.344, beta=0.405, dA=0.282, dB=0.287, dW1=0.205, db1=0.276, dw2=0.260),
    (1256, 256): dict(out=0.252, beta=0.219, dA=0.429, dB=0.689, dW1=0.270, db1=0.542, dw2=0.281),
}

_cache = {}


def _exact(n_rows, F, mult, seed=0):
    """``(design, restatement rounded to fp32)``; the last few stay cached (the large ones are used twice)."""
    key = (n_rows, F, mult, seed)
    if key not in _cache:
        if len(_cache) >= 6:
            _cache.pop(next(iter(_cache)))
        d = K.exact_design(n_rows, F, mult, seed)
        r = K.reference(d["A"], d["B"], d["W1"], d["b1"], d["w2"], d["M"], d["g"])
        _cache[key] = (d, {k: v.astype(np.float32) for k, v in r.items()})
    return _cache[key]


def _equal(got, want, what=""):
    for k in K.OUTPUTS:
        assert got[k].shape == want[k].shape and got[k].dtype == np.float32, (what, k)
        assert np.array_equal(got[k], want[k]), (what, k, np.abs(got[k] - want[k]).max())


def _bits(x):
    return np.ascontiguousarray(x).view(np.int32)


def _same_bits(got, want, what="", names=K.OUTPUTS):
    for k in names:
        assert got[k].shape == want[k].shape and np.array_equal(_bits(got[k]), _bits(want[k])), (what, k)


# ---------------------------------------------------------------------------------------------------------------------
# 1. widths with live partials
@pytest.mark.parametrize("mult", [False, True])
@pytest.mark.parametrize("F", [4, 12, 20, 28, 32, 36, 124, 132, 252, 260, 508, 512])
def test_every_width_class_with_four_contributing_blocks(dev, F, mult):
    d, want = _exact(200, F, mult)
    for layout in ("contiguous", "stacked_direct"):
        _equal(T._run(d, dev, layout), want, layout)


@pytest.mark.parametrize("mult", [False, True])
@pytest.mark.parametrize("F", [32, 260])
def test_accumulators_carried_into_a_second_contributing_block(dev, F, mult):
    R, G = T._RG()
    d, want = _exact(R * G + 2 * R + 3, F, mult)
    for layout in ("contiguous", "stacked_direct"):
        _equal(T._run(d, dev, layout), want, layout)


# ---------------------------------------------------------------------------------------------------------------------
# 2. partial counts of the reduce kernel
@pytest.mark.parametrize("mult", [False, True])
@pytest.mark.parametrize("k", [15, 16, 17, 240, 241, 255, 256, 257, 1023])
def test_reduce_kernel_at_every_partial_count(dev, k, mult):
    d, want = _exact(T._RG()[0] * k - 3, 16, mult)
    _equal(T._run(d, dev), want)


# ---------------------------------------------------------------------------------------------------------------------
# 3. the C ABI in guarded buffers
SENTINEL = 0x5A5A5A5A   # a finite float (1.5e16) no exact design produces
GUARD_ROWS, PAD = 16, 16


def _table_in(x, ld, dev):
    """``x`` in the first columns and rows of an (n + GUARD_ROWS, ld) buffer that is NaN everywhere else."""
    n, F = x.shape
    buf = torch.full((n + GUARD_ROWS, ld), float("nan"), device=dev)
    buf[:n, :F] = torch.from_numpy(x).to(dev)
    return buf


def _table_out(n, ld, dev):
    return torch.full((n + GUARD_ROWS, ld), SENTINEL, dtype=torch.int32, device=dev)


def _small_out(count, dev):
    return torch.full((PAD + count + PAD,), SENTINEL, dtype=torch.int32, device=dev)


def _check_table(buf, n, F, want, what):
    b = buf.cpu().numpy()
    assert np.array_equal(b[:n, :F].view(np.float32), want), (what, np.abs(b[:n, :F].view(np.float32) - want).max())
    assert np.all(b[:n, F:] == SENTINEL) and np.all(b[n:] == SENTINEL), what


def _check_small(buf, want, what):
    b = buf.cpu().numpy()
    count = want.size
    assert np.array_equal(b[PAD:PAD + count].view(np.float32), want.reshape(-1)), what
    assert np.all(b[:PAD] == SENTINEL) and np.all(b[PAD + count:] == SENTINEL), what


@pytest.mark.parametrize("mult", [False, True])
@pytest.mark.parametrize("F", [20, 36, 132, 260])
@pytest.mark.parametrize("n_rows", [131, 1])
def test_c_abi_keeps_to_its_extents_under_six_leading_dimensions(dev, n_rows, F, mult):
    from dream_gnn_amd import _lib, ops

    L = _lib.lib
    d, want = _exact(n_rows, F, mult)
    n = n_rows
    lda, ldb, ldg, ldo, ld_da, ld_db = (F + 4 * i for i in range(1, 7))
    A, B, g = _table_in(d["A"], lda, dev), _table_in(d["B"], ldb, dev), _table_in(d["g"], ldg, dev)
    W1, b1, w2 = (torch.from_numpy(d[k]).to(dev) for k in ("W1", "b1", "w2"))
    M = torch.from_numpy(d["M"]).to(dev) if mult else None
    out, dA, dB = _table_out(n, ldo, dev), _table_out(n, ld_da, dev), _table_out(n, ld_db, dev)
    beta, dW1, db1, dw2 = _small_out(2 * n, dev), _small_out(16 * F, dev), _small_out(16, dev), _small_out(16, dev)
    wb = L.dgmi_attn_fuse_workspace_bytes(n, F)
    assert wb > 0 and wb % 256 == 0
    ws = torch.full((wb + 4096,), 0xA5, dtype=torch.uint8, device=dev)
    for t in (A, B, g, W1, out, dA, dB, ws):
        assert t.data_ptr() % 16 == 0
    small = lambda t: t.data_ptr() + 4 * PAD
    operands = (A.data_ptr(), lda, B.data_ptr(), ldb, n, F, 16, W1.data_ptr(), b1.data_ptr(), w2.data_ptr(),
                None if M is None else M.data_ptr())
    stream = torch.cuda.current_stream().cuda_stream
    assert L.dgmi_attn_fuse_forward_f32(*operands, out.data_ptr(), ldo, small(beta), stream) == 0
    assert L.dgmi_attn_fuse_backward_f32(*operands, g.data_ptr(), ldg, dA.data_ptr(), ld_da, dB.data_ptr(), ld_db, small(dW1),
                                         small(db1), small(dw2), ws.data_ptr(), wb, stream) == 0
    torch.cuda.synchronize()
    _check_table(out, n, F, want["out"], "out")
    _check_table(dA, n, F, want["dA"], "dA")
    _check_table(dB, n, F, want["dB"], "dB")
    for buf, k in ((beta, "beta"), (dW1, "dW1"), (db1, "db1"), (dw2, "dw2")):
        _check_small(buf, want[k], k)
    assert bool((ws[wb:] == 0xA5).all())
    for buf, k in ((A, "A"), (B, "B"), (g, "g")):                               # the inputs are as they were
        b = buf.cpu().numpy()
        assert np.array_equal(b[:n, :F], d[k]) and np.isnan(b[:n, F:]).all() and np.isnan(b[n:]).all(), k

    # the same operands through ops: a padded by 4, b by 8, the upstream gradient by 12
    a, b = A[:n, :F].requires_grad_(True), B[:n, :F].requires_grad_(True)
    params = [W1.clone().requires_grad_(True), b1.clone().requires_grad_(True), w2.clone().requires_grad_(True)]
    o, bt = ops.attention_fuse(a, b, *params, M)
    grads = torch.autograd.grad(o, [a, b] + params, g[:n, :F])
    got = dict(zip(K.OUTPUTS, (o.detach(), bt) + tuple(grads)))
    _equal({k: v.cpu().numpy().reshape(want[k].shape) for k, v in got.items()}, want, "ops")


# ---------------------------------------------------------------------------------------------------------------------
# 4. row independence by bits
def _float_rule(fused, chain, want, where, what):
    """``max|T_fused - T_64| <= 4 max|T_chain - T_64| + 2^-22 max|T_64|`` over the elements ``where``; a chain that is
    not finite there bounds nothing."""
    if not where.any():
        return
    w = want[where]
    e_f = np.abs(fused[where] - w).max()
    c = chain[where]
    with np.errstate(invalid="ignore"):
        e_c = np.where(np.isfinite(c), np.abs(c - w), np.inf).max()
    bound = 4 * e_c + 2.0 ** -22 * np.abs(w).max()
    assert e_f <= bound, (what, e_f, e_c, bound)


def _poison_clean(dev):
    if "clean" not in _cache:
        d0 = K.float_design(*K.POISON_SHAPE)
        _cache["clean"] = (d0, T._run(d0, dev))
    return _cache["clean"]


@pytest.mark.parametrize("operand", ["A", "B", "g", "M"])
def test_a_poisoned_element_stays_in_its_row_bit_for_bit(dev, operand):
    d0, clean = _poison_clean(dev)
    n = d0["A"].shape[0]
    assert all(np.isfinite(clean[k]).all() for k in K.OUTPUTS)
    for case in [c for c in K.poison_cases() if c[0] == operand]:
        _, row, col, value = case
        d = K.poison(d0, *case)
        got, chain, want = T._run(d, dev), T._chain(d, dev), K.restate(d)
        other = np.arange(n) != row
        for k in ("out", "beta", "dA", "dB"):
            assert np.array_equal(_bits(got[k][other]), _bits(clean[k][other])), (case, k)
        if operand == "g":
            _same_bits(got, clean, case, ("out", "beta"))
        left_out = K.POISON_LEFT_OUT.get((operand, row, col, repr(value)), {})
        for k in K.OUTPUTS:
            keep = np.ones(want[k].shape, dtype=bool)
            for idx in left_out.get(k, ()):
                keep[idx] = False
            assert np.array_equal(K.classes(got[k])[keep], K.classes(want[k])[keep]), (case, k)
            finite = np.isfinite(want[k]) & keep
            if k in ("out", "beta", "dA", "dB"):
                finite[other] = False
            _float_rule(got[k], chain[k], want[k], finite, (case, k))
        if not np.isfinite(value) and operand != "g":
            assert not np.isfinite(got["out"][row]).all() or not np.isfinite(got["beta"][row]).all(), case
        if not np.isfinite(value):
            assert not np.isfinite(got["dA"][row]).all() and not np.isfinite(got["dW1"]).all(), case


# ---------------------------------------------------------------------------------------------------------------------
# 5. saturating weights
@pytest.mark.parametrize("n_rows,F,seed", [(763, 128, 40), (1256, 256, 41)])
def test_saturating_weights_meet_the_accuracy_rule(dev, n_rows, F, seed):
    d = K.float_design(n_rows, F, seed, w1_scale=4, w2_scale=8)
    want = K.reference(d["A"], d["B"], d["W1"], d["b1"], d["w2"], d["M"], d["g"])
    fused, chain = T._run(d, dev), T._chain(d, dev)
    failed = []
    for k in K.OUTPUTS:
        e_f, e_c = np.abs(fused[k] - want[k]).max(), np.abs(chain[k] - want[k]).max()
        bound = 4 * e_c + 2.0 ** -22 * np.abs(want[k]).max()
        print("attention_fuse saturated (%d, %d) %-4s fused %.3e chain %.3e ratio to bound %.3f" % (n_rows, F, k, e_f, e_c, e_f / bound))
        if not e_f <= bound:
            failed.append(k)
    assert not failed, failed


# ---------------------------------------------------------------------------------------------------------------------
# 6. operand forms through ops
FORMS_SHAPE = (131, 128)


def _form_operands(dev):
    d, want = _exact(*FORMS_SHAPE, True)
    t = {k: torch.from_numpy(d[k]).to(dev) for k in ("A", "B", "W1", "b1", "w2", "M", "g")}
    return d, want, t


def _call(t, a=None, b="given", W1=None, b1=None, w2=None, M="given", g=None, grad=(True,) * 5):
    """One forward and ``backward`` of ``ops.attention_fuse``: the tensors of ``t`` unless an operand is given; returns
    ``(out, beta, leaves)`` with the gradients on the leaves."""
    from dream_gnn_amd import ops

    leaf = lambda x, need: x.clone().requires_grad_(need)
    a = leaf(t["A"], grad[0]) if a is None else a
    b = leaf(t["B"], grad[1]) if isinstance(b, str) else b
    W1 = leaf(t["W1"], grad[2]) if W1 is None else W1
    b1 = leaf(t["b1"], grad[3]) if b1 is None else b1
    w2 = leaf(t["w2"], grad[4]) if w2 is None else w2
    M = t["M"] if isinstance(M, str) else M
    out, beta = ops.attention_fuse(a, b, W1, b1, w2, M)
    out.backward(t["g"] if g is None else g)
    return out.detach(), beta, (a, b, W1, b1, w2)


def _np(out, beta, grads):
    got = dict(zip(K.OUTPUTS, (out, beta) + tuple(grads)))
    return {k: v.detach().cpu().numpy().reshape(-1) if k in ("db1", "dw2") else v.detach().cpu().numpy() for k, v in got.items()}


def _base(dev):
    """The contiguous call on the exact design: equal to the restatement; every form below must have its bits."""
    d, want, t = _form_operands(dev)
    out, beta, leaves = _call(t)
    got = _np(out, beta, [x.grad for x in leaves])
    _equal(got, want, "contiguous")
    return t, got


def _misaligned(x):
    """A copy of ``x`` whose storage starts one float off a 16-byte boundary (a leaf view)."""
    buf = torch.empty(x.numel() + 1, device=x.device)
    v = buf[1:].view(x.shape)
    v.copy_(x)
    assert v.data_ptr() % 16 == 4
    return v


def test_upstream_gradient_forms(dev):
    from dream_gnn_amd import ops

    t, base = _base(dev)
    n, F = FORMS_SHAPE
    padded = torch.zeros(n, F + 4, device=dev)
    padded[:, :F] = t["g"]
    strided = t["g"].t().contiguous().t()
    assert strided.stride() == (1, n) and padded[:, :F].stride() == (F + 4, 1)
    for what, g in (("padded", padded[:, :F]), ("column-strided", strided)):
        out, beta, leaves = _call(t, g=g)
        _same_bits(_np(out, beta, [x.grad for x in leaves]), base, what)
    # a stride-0 gradient (out.sum().backward()) against the same gradient materialised
    runs = []
    for expanded in (True, False):
        leaves = [t[k].clone().requires_grad_(True) for k in ("A", "B", "W1", "b1", "w2")]
        out, beta = ops.attention_fuse(*leaves, t["M"])
        if expanded:
            (out * 1).sum().backward()
        else:
            out.backward(torch.ones(n, F, device=dev))
        runs.append(_np(out, beta, [x.grad for x in leaves]))
    _same_bits(runs[0], runs[1], "expanded")
    assert runs[0]["dW1"].any() and runs[0]["dA"].any()


def test_tables_off_a_16_byte_boundary(dev):
    from dream_gnn_amd import ops

    t, base = _base(dev)
    n, F = FORMS_SHAPE
    for what, which in (("a", (True, False)), ("b", (False, True)), ("a and b", (True, True))):
        a = _misaligned(t["A"]).requires_grad_(True) if which[0] else None
        b = _misaligned(t["B"]).requires_grad_(True) if which[1] else "given"
        out, beta, leaves = _call(t, a=a, b=b)
        _same_bits(_np(out, beta, [x.grad for x in leaves]), base, what)
    z = _misaligned(torch.stack([t["A"], t["B"]], 1)).requires_grad_(True)
    params = [t[k].clone().requires_grad_(True) for k in ("W1", "b1", "w2")]
    out, beta = ops.attention_fuse(z, None, *params, t["M"])
    out.backward(t["g"])
    assert z.grad.shape == (n, 2, F)
    _same_bits(_np(out, beta, [z.grad[:, 0], z.grad[:, 1]] + [p.grad for p in params]), base, "stacked")


def test_parameter_and_multiplier_forms(dev):
    t, base = _base(dev)
    n, F = FORMS_SHAPE
    Wt = t["W1"].t().contiguous().requires_grad_(True)                          # an (F, 16) leaf
    assert not Wt.t().is_contiguous()
    out, beta, leaves = _call(t, W1=Wt.t())
    assert Wt.grad.shape == (F, 16) and Wt.grad.stride() == Wt.stride()         # the gradient in the leaf's layout
    got = _np(out, beta, [leaves[0].grad, leaves[1].grad, Wt.grad.t(), leaves[3].grad, leaves[4].grad])
    _same_bits(got, base, "W1 transposed")
    M4 = torch.full((n, 4), 7.0, device=dev)
    M4[:, 1:3] = t["M"]
    assert not M4[:, 1:3].is_contiguous()
    out, beta, leaves = _call(t, M=M4[:, 1:3])
    _same_bits(_np(out, beta, [x.grad for x in leaves]), base, "mult a column slice")
    Mg = t["M"].clone().requires_grad_(True)
    out, beta, leaves = _call(t, M=Mg)
    assert Mg.grad is None and not beta.requires_grad
    _same_bits(_np(out, beta, [x.grad for x in leaves]), base, "mult requires grad")
    for what, shape1, shape2 in (("b1 (1, 16), w2 (1, 16)", (1, 16), (1, 16)), ("w2 (16, 1)", (16,), (16, 1))):
        b1, w2 = t["b1"].clone().view(shape1).requires_grad_(True), t["w2"].clone().view(shape2).requires_grad_(True)
        out, beta, leaves = _call(t, b1=b1, w2=w2)
        assert b1.grad.shape == shape1 and w2.grad.shape == shape2
        _same_bits(_np(out, beta, [x.grad for x in leaves]), base, what)
    wide = [torch.zeros(16, 2, device=dev) for _ in range(2)]                    # b1 and w2 as every second float
    wide[0][:, 0], wide[1][:, 0] = t["b1"], t["w2"]
    b1, w2 = (x.requires_grad_(True) for x in wide)
    out, beta, leaves = _call(t, b1=b1[:, 0], w2=w2[:, 0])
    got = _np(out, beta, [leaves[0].grad, leaves[1].grad, leaves[2].grad, b1.grad[:, 0], w2.grad[:, 0]])
    assert not b1.grad[:, 1].any() and not w2.grad[:, 1].any()
    _same_bits(got, base, "b1 and w2 strided")


def test_one_leaf_passed_twice_gets_the_sum_of_both_gradients(dev):
    d, _, t = _form_operands(dev)
    separate = dict(t, B=t["A"])
    out0, beta0, leaves0 = _call(separate)
    x = t["A"].clone().requires_grad_(True)
    out, beta, leaves = _call(t, a=x, b=x)
    assert torch.equal(out, out0) and torch.equal(beta, beta0)
    assert torch.equal(x.grad, leaves0[0].grad + leaves0[1].grad) and x.grad.any()
    for u, v in zip(leaves[2:], leaves0[2:]):
        assert torch.equal(u.grad, v.grad)


def test_requires_grad_subsets(dev):
    t, base = _base(dev)
    names = K.OUTPUTS[2:]
    for need in ((False, False, True, True, True), (True, False, False, False, False), (False, True, False, False, True)):
        out, beta, leaves = _call(t, grad=need)
        assert np.array_equal(_bits(out.cpu().numpy()), _bits(base["out"])), need
        for k, x, wanted in zip(names, leaves, need):
            if wanted:
                assert np.array_equal(_bits(x.grad.cpu().numpy().reshape(base[k].shape)), _bits(base[k])), (need, k)
            else:
                assert x.grad is None, (need, k)


def test_a_second_backward(dev):
    from dream_gnn_amd import ops

    t, base = _base(dev)
    leaves = [t[k].clone().requires_grad_(True) for k in ("A", "B", "W1", "b1", "w2")]
    out, beta = ops.attention_fuse(*leaves, t["M"])
    first = torch.autograd.grad(out, leaves, t["g"], retain_graph=True)
    second = torch.autograd.grad(out, leaves, t["g"])
    for run in (first, second):
        _same_bits(_np(out, beta, run), base, "retain_graph")
    with pytest.raises(RuntimeError, match="backward through the graph a second time"):
        torch.autograd.grad(out, leaves, t["g"])


def test_a_side_stream_gives_the_default_streams_bits(dev):
    t, base = _base(dev)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        out, beta, leaves = _call(t)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    _same_bits(_np(out, beta, [x.grad for x in leaves]), base, "side stream")


def test_a_small_call_after_a_large_one_reads_no_stale_partials(dev):
    R, G = T._RG()
    big, want_big = _exact(R * G + 65, 128, True)
    small, want_small = _exact(3, 128, True)
    first = T._run(big, dev)
    middle = T._run(small, dev)
    third = T._run(big, dev)
    _equal(first, want_big, "large")
    _equal(middle, want_small, "3 rows after the large call")
    _same_bits(third, first, "large again")


# ---------------------------------------------------------------------------------------------------------------------
# 7. the module on the device
def _module_pair(make, dev, seed=5):
    atts = []
    for fused in (False, True):
        torch.manual_seed(seed)
        att = make().to(dev).train()
        att.fused = fused
        atts.append(att)
    return atts


def _module_step(att, inputs, g, route):
    leaves = [x.detach().requires_grad_(True) for x in inputs]                  # the same storage: an offset stays an offset
    att.zero_grad(set_to_none=True)
    torch.manual_seed(11)
    out, beta = att.fuse(*leaves) if route == "fuse" else att(*leaves)
    out.backward(g)
    return (out.detach(), beta, [x.grad for x in leaves] + [p.grad for p in att.parameters()], torch.cuda.get_rng_state())


def _with_biased_output():
    from dream_gnn_amd import model as M

    att = M.Attention(64, dropout_rate=0.5)
    att.project[2] = torch.nn.Linear(16, 1, bias=True)
    return att


def _fallback_cases(dev):
    from dream_gnn_amd import model as M

    r = lambda *s, **kw: torch.randn(*s, device=dev, **kw)
    off = torch.empty(301 * 64 + 1, device=dev)[1:].view(301, 64).copy_(r(301, 64))
    return {
        "F = 6": (lambda: M.Attention(6, dropout_rate=0.5), (r(301, 2, 6),), r(301, 6), "forward"),
        "F = 6, fuse": (lambda: M.Attention(6, dropout_rate=0.5), (r(301, 6), r(301, 6)), r(301, 6), "fuse"),
        "hidden 8": (lambda: M.Attention(64, hidden_size=8, dropout_rate=0.5), (r(301, 2, 64),), r(301, 64), "forward"),
        "three channels": (lambda: M.Attention(64, dropout_rate=0.5), (r(301, 3, 64),), r(301, 64), "forward"),
        "float64": (lambda: M.Attention(64, dropout_rate=0.5).double(), (r(301, 2, 64, dtype=torch.float64),),
                    r(301, 64, dtype=torch.float64), "forward"),
        "output bias": (_with_biased_output, (r(301, 2, 64),), r(301, 64), "forward"),
        "rows off 16 bytes": (lambda: M.Attention(64, dropout_rate=0.5), (off, r(301, 64)), r(301, 64), "fuse"),
    }


@pytest.mark.parametrize("case", ["F = 6", "F = 6, fuse", "hidden 8", "three channels", "float64", "output bias", "rows off 16 bytes"])
def test_module_falls_back_to_the_chain_bit_for_bit(dev, case):
    torch.manual_seed(2)
    make, inputs, g, route = _fallback_cases(dev)[case]
    if case == "rows off 16 bytes":
        assert inputs[0].data_ptr() % 16 == 4
    plain, flagged = _module_pair(make, dev)
    assert flagged.fused is True and plain.fused is False
    want, got = _module_step(plain, inputs, g, route), _module_step(flagged, inputs, g, route)
    assert got[1].requires_grad and want[1].requires_grad                      # the chain's beta carries gradient
    assert (want[1] == 0).any()                                                # dropout was drawn
    assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1]) and torch.equal(got[3], want[3])
    assert len(got[2]) == len(want[2])
    for u, v in zip(got[2], want[2]):
        assert u is not None and torch.equal(u, v)


def test_module_uses_the_rate_its_dropout_holds_now(dev):
    from dream_gnn_amd import model as M

    torch.manual_seed(2)
    n = 2001
    x, y, g = torch.randn(n, 64, device=dev), 0.5 * torch.randn(n, 64, device=dev), torch.randn(n, 64, device=dev)
    plain, flagged = _module_pair(lambda: M.Attention(64, dropout_rate=0.1), dev)
    for att in (plain, flagged):
        att.dropout.p = 0.5
    want, got = _module_step(plain, (x, y), g, "fuse"), _module_step(flagged, (x, y), g, "fuse")
    assert not got[1].requires_grad and got[1].shape == (n, 2, 1)              # the fused route ran
    share = float((got[1] == 0).float().mean())
    assert abs(share - 0.5) < 0.05, share                                       # 0.5, not the constructor's 0.1 (sigma 0.008)
    assert torch.equal(got[3], want[3])
    T._within_module_bar((got[0], got[1].detach(), got[2]), (want[0], want[1].detach(), want[2]))


def test_module_with_dropout_one_returns_exact_zeros_on_both_routes(dev):
    from dream_gnn_amd import model as M

    torch.manual_seed(2)
    x, y, g = torch.randn(301, 64, device=dev), 0.5 * torch.randn(301, 64, device=dev), torch.randn(301, 64, device=dev)
    plain, flagged = _module_pair(lambda: M.Attention(64, dropout_rate=0.5), dev)
    states = []
    for att in (plain, flagged):
        att.dropout.p = 1.0
        for route, inputs in (("fuse", (x, y)), ("forward", (torch.stack([x, y], 1),))):
            out, beta, grads, state = _module_step(att, inputs, g, route)
            assert beta.requires_grad == (att is plain)
            assert not out.any() and not beta.any() and out.shape == (301, 64) and beta.shape == (301, 2, 1)
            assert all(u is not None and not u.any() for u in grads), (att.fused, route)
            states.append(state)
    assert all(torch.equal(s, states[0]) for s in states)


def test_module_fuse_of_one_tensor_with_itself(dev):
    from dream_gnn_amd import model as M

    torch.manual_seed(2)
    x, g = torch.randn(301, 64, device=dev), torch.randn(301, 64, device=dev)
    plain, flagged = _module_pair(lambda: M.Attention(64, dropout_rate=0.5), dev)
    runs = []
    for att in (plain, flagged):
        att.eval()
        leaf = x.clone().requires_grad_(True)
        att.zero_grad(set_to_none=True)
        out, beta = att.fuse(leaf, leaf)
        out.backward(g)
        runs.append((out.detach(), beta.detach(), [leaf.grad] + [p.grad for p in att.parameters()]))
        assert beta.requires_grad == (att is plain)
    T._within_module_bar(runs[1], runs[0])


def test_module_on_empty_tables_returns_the_chains_shapes(dev):
    from dream_gnn_amd import model as M

    plain, flagged = _module_pair(lambda: M.Attention(64, dropout_rate=0.5), dev)
    e = torch.zeros(0, 64, device=dev)
    for route, inputs in (("fuse", (e, e.clone())), ("forward", (torch.zeros(0, 2, 64, device=dev),))):
        want = _module_step(plain, inputs, torch.zeros(0, 64, device=dev), route)
        got = _module_step(flagged, inputs, torch.zeros(0, 64, device=dev), route)
        assert got[0].shape == want[0].shape == (0, 64) and got[1].shape == want[1].shape == (0, 2, 1)
        for u, v in zip(got[2], want[2]):
            assert u is not None and v is not None and u.shape == v.shape and not u.any()
