"""The fused attention fusion, host side (no GPU): include/dgmi_attn.h declares exactly the three entry points, the library
exports them and ``ATTN_SIGNATURES`` matches type for type; argument validation and workspace sizing return codes before
any launch; the ops are registered for the device only; the module flag is opt-in and falls back to the chain on CPU
tensors; the float64 restatement agrees with float64 autograd of the module's expression; the exact designs keep their
margins, classes and bound; and what ``test_gpu_attention_forms.py`` relies on: every block of its exact designs adds to
all three parameter sums (the first suite's width shapes do not), the scaled float design saturates, and the poisoned
designs have one class map in any precision and order of summation."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import _attention_cases as K

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY_POINTS = ["dgmi_attn_fuse_backward_f32", "dgmi_attn_fuse_forward_f32", "dgmi_attn_fuse_workspace_bytes"]
CTYPE = {"const float*": ctypes.c_void_p, "float*": ctypes.c_void_p, "void*": ctypes.c_void_p,
         "dgmi_stream_t": ctypes.c_void_p, "int64_t": ctypes.c_int64, "int32_t": ctypes.c_int32,
         "size_t": ctypes.c_size_t, "int": ctypes.c_int}


def _text():
    return open(os.path.join(ROOT, "include", "dgmi_attn.h")).read()


def _prototypes():
    """name -> (return type, [parameter types]) as the header spells them."""
    out = {}
    for ret, name, params in re.findall(r"DGMI_API\s+([\w\s\*]+?)\s*\b(dgmi_\w+)\s*\(([^)]*)\)\s*;", _text()):
        types = [re.sub(r"\s*\w+$", "", " ".join(q.split())).replace(" *", "*") for q in params.split(",")]
        out[name] = (ret.strip(), types)
    return out


def _constant(name):
    return int(re.search(r"#define\s+%s\s+(\d+)" % name, _text()).group(1))


def test_header_declares_exactly_the_three_entry_points():
    assert sorted(_prototypes()) == ENTRY_POINTS
    assert '#include "dgmi.h"' in _text()
    dgmi = open(os.path.join(ROOT, "include", "dgmi.h")).read()
    assert "#define DGMI_ABI_VERSION 20" in dgmi and "attn" not in dgmi


def test_table_matches_the_header_type_for_type_and_the_library_exports_it():
    from dream_gnn_amd import _lib

    protos = _prototypes()
    assert sorted(_lib.ATTN_SIGNATURES) == ENTRY_POINTS
    for name, (res, args) in _lib.ATTN_SIGNATURES.items():
        ret, types = protos[name]
        assert CTYPE[ret] is res, name
        assert [CTYPE[t] for t in types] == args, name
        fn = getattr(_lib.lib, name)
        assert fn.restype is res and list(fn.argtypes) == args, name
    for other in (_lib.SIGNATURES, _lib.PAIR_SIGNATURES, _lib.RANK_SIGNATURES, _lib.ABOVE_SIGNATURES, _lib.BF16_SIGNATURES,
                  _lib.GIVEN_SIGNATURES, _lib.CURVE_SIGNATURES, _lib.LAYOUT_SIGNATURES, _lib.TRAIN_SIGNATURES):
        assert not set(_lib.ATTN_SIGNATURES) & set(other)


def test_python_mirrors_the_header_constants():
    from dream_gnn_amd import ops

    assert ops.ATTN_FUSE_BLOCK_ROWS == _constant("DGMI_ATTN_BLOCK_ROWS")
    assert ops.ATTN_FUSE_MAX_WORKGROUPS == _constant("DGMI_ATTN_MAX_WORKGROUPS")


# fake device addresses, 16-byte aligned and far apart: every call below must return before anything is launched
_BASE = dict(A=0x100000, lda=128, B=0x200000, ldb=128, n_rows=40, F=128, H=16, W1=0x300000, b1=0x310000, w2=0x320000, M=None,
             out=0x400000, ldo=128, beta=0x500000, dout=0x600000, ldg=128, dA=0x700000, ld_da=128, dB=0x800000, ld_db=128,
             dW1=0x900000, db1=0x910000, dw2=0x920000, ws=0xA00000, wsb=1 << 40, stream=None)


def _operands(a):
    return [a[k] for k in ("A", "lda", "B", "ldb", "n_rows", "F", "H", "W1", "b1", "w2", "M")]


def _forward(L, **kw):
    a = dict(_BASE)
    a.update(kw)
    return L.dgmi_attn_fuse_forward_f32(*_operands(a), a["out"], a["ldo"], a["beta"], a["stream"])


def _backward(L, **kw):
    a = dict(_BASE)
    a.update(kw)
    return L.dgmi_attn_fuse_backward_f32(*_operands(a), a["dout"], a["ldg"], a["dA"], a["ld_da"], a["dB"], a["ld_db"], a["dW1"],
                                         a["db1"], a["dw2"], a["ws"], a["wsb"], a["stream"])


@pytest.mark.parametrize("call", [_forward, _backward])
def test_argument_validation_returns_codes_without_a_gpu(call):
    from dream_gnn_amd import _lib

    L = _lib.lib
    assert call(L, H=8) == -1 and call(L, H=32) == -1                            # only hidden size 16
    for F in (0, 2, 6, 130, 516, 1024, -4):
        assert call(L, F=F, lda=1024, ldb=1024, ldo=1024, ldg=1024, ld_da=1024, ld_db=1024) == -1, F
    assert call(L, lda=124) == -1 and call(L, ldb=64) == -1 and call(L, lda=130) == -1 and call(L, ldb=134) == -1
    for name in ("A", "B", "W1", "b1", "w2"):                                    # null pointers (M may be null)
        assert call(L, **{name: None}) == -1, name
    assert call(L, A=0x100004) == -1 and call(L, B=0x200008) == -1 and call(L, W1=0x300004) == -1   # not 16-B aligned
    assert call(L, n_rows=2 ** 31) == -1 and call(L, n_rows=-1) == -1
    assert call(L, n_rows=0, H=8) == -1 and call(L, n_rows=0, F=6) == -1 and call(L, n_rows=0, A=None) == -1
    assert call(L, n_rows=0, lda=64) == -1                                      # an empty call excuses no bad argument


def test_forward_and_backward_own_arguments():
    from dream_gnn_amd import _lib

    L = _lib.lib
    assert _forward(L, n_rows=0) == 0                                            # writes nothing, launches nothing
    assert _forward(L, out=None) == -1 and _forward(L, beta=None) == -1
    assert _forward(L, ldo=124) == -1 and _forward(L, ldo=130) == -1 and _forward(L, out=0x400008) == -1
    assert _forward(L, out=_BASE["A"]) == -1 and _forward(L, out=_BASE["B"]) == -1              # out overlapping A or B
    assert _forward(L, out=_BASE["A"] + 16 * 128) == -1 and _forward(L, out=_BASE["B"] - 16) == -1
    assert _forward(L, n_rows=0, out=_BASE["A"]) == -1 and _forward(L, n_rows=0, out=None) == -1
    for name in ("dout", "dA", "dB", "dW1", "db1", "dw2"):
        assert _backward(L, **{name: None}) == -1, name
        assert _backward(L, n_rows=0, **{name: None}) == -1, name
    assert _backward(L, ldg=124) == -1 and _backward(L, ld_da=130) == -1 and _backward(L, ld_db=64) == -1
    assert _backward(L, dout=0x600004) == -1 and _backward(L, dA=0x700008) == -1 and _backward(L, dB=0x800004) == -1
    assert _backward(L, ws=None) == -3 and _backward(L, wsb=64) == -3            # workspace missing / short
    assert _backward(L, wsb=L.dgmi_attn_fuse_workspace_bytes(40, 128) - 1) == -3


def test_workspace_formula():
    from dream_gnn_amd import _lib

    W = _lib.lib.dgmi_attn_fuse_workspace_bytes
    R, G = _constant("DGMI_ATTN_BLOCK_ROWS"), _constant("DGMI_ATTN_MAX_WORKGROUPS")
    for F in (4, 128, 132, 512):
        def want(n):
            if n <= 0 or n > 2 ** 31 - 1:
                return 0
            groups = min(-(-n // R), G)
            return -(-(groups * (16 * F + 32) * 4) // 256) * 256

        ns = [0, -1, 2 ** 31, 1, R - 1, R, R + 1, R * G, R * G + 1, 2 ** 31 - 1]
        assert [W(n, F) for n in ns] == [want(n) for n in ns], F
        sizes = [W(n, F) for n in sorted(n for n in ns if 0 < n < 2 ** 31)]
        assert sizes == sorted(sizes) and all(s % 256 == 0 and s > 0 for s in sizes)
    assert W(100, 6) == 0 and W(100, 516) == 0 and W(100, 0) == 0


def test_torch_ops_are_registered_for_the_device_only():
    from dream_gnn_amd import _lib  # noqa: F401

    ns = torch.ops.dreamgnn_mi
    fwd, bwd = ns.attn_fuse_forward.default._schema, ns.attn_fuse_backward.default._schema
    assert str(fwd) == ("dreamgnn_mi::attn_fuse_forward(Tensor A, Tensor B, Tensor? M, Tensor W1, Tensor b1, Tensor w2) "
                        "-> (Tensor, Tensor)")
    assert str(bwd) == ("dreamgnn_mi::attn_fuse_backward(Tensor A, Tensor B, Tensor? M, Tensor W1, Tensor b1, Tensor w2, "
                        "Tensor dout) -> (Tensor, Tensor, Tensor, Tensor, Tensor)")
    z = (torch.zeros(2, 8), torch.zeros(2, 8), None, torch.zeros(16, 8), torch.zeros(16), torch.zeros(16))
    with pytest.raises(NotImplementedError):  # no CPU kernel
        ns.attn_fuse_forward(*z)
    with pytest.raises(NotImplementedError):
        ns.attn_fuse_backward(*z, torch.zeros(2, 8))


def test_ops_refuse_cpu_tensors():
    from dream_gnn_amd import ops

    z = (torch.zeros(2, 8), torch.zeros(2, 8), torch.zeros(16, 8), torch.zeros(16), torch.zeros(16))
    with pytest.raises(RuntimeError, match="MI355X only"):
        ops.attention_fuse(*z)


def test_module_flag_is_opt_in_and_keeps_rng_and_state_dict():
    from dream_gnn_amd import model as M

    assert M.Attention.fused is False
    torch.manual_seed(0)
    a = M.Attention(8, dropout_rate=0.1)
    state_a = torch.get_rng_state()
    torch.manual_seed(0)
    b = M.Attention(8, dropout_rate=0.1, fused=True)
    assert torch.equal(state_a, torch.get_rng_state())
    assert a.fused is False and b.fused is True and "fused" not in vars(a)
    sa, sb = a.state_dict(), b.state_dict()
    assert list(sa) == list(sb) == ["project.0.weight", "project.0.bias", "project.2.weight"]
    assert all(torch.equal(sa[k], sb[k]) for k in sa)


@pytest.mark.parametrize("training", [True, False])
def test_flag_falls_back_to_the_chain_on_cpu_tensors_bit_for_bit(training):
    from dream_gnn_amd import model as M

    torch.manual_seed(1)
    att = M.Attention(8, dropout_rate=0.5)
    att.train(training)
    x, y = torch.randn(13, 8), torch.randn(13, 8)
    z = torch.stack([x, y], 1)
    runs = []
    for fused, route in ((False, "forward"), (True, "forward"), (False, "fuse"), (True, "fuse")):
        att.fused = fused
        torch.manual_seed(7)
        out, beta = att(z) if route == "forward" else att.fuse(x, y)
        runs.append((out, beta, torch.get_rng_state()))
    for out, beta, state in runs[1:]:
        assert torch.equal(out, runs[0][0]) and torch.equal(beta, runs[0][1]) and torch.equal(state, runs[0][2])
    assert runs[0][1].shape == (13, 2, 1)


@pytest.mark.parametrize("n_rows,F,seed", [(37, 8, 0), (19, 128, 1), (5, 132, 2)])
def test_restatement_agrees_with_float64_autograd_of_the_module_expression(n_rows, F, seed):
    d = K.float_design(n_rows, F, seed)
    t = {k: (None if v is None else torch.tensor(v, dtype=torch.float64)) for k, v in d.items()}
    for with_mult in (False, True):
        leaves = [t[k].clone().requires_grad_(True) for k in ("A", "B", "W1", "b1", "w2")]
        A, B, W1, b1, w2 = leaves
        z = torch.stack([A, B], 1)
        # model.Attention.forward with nn.Dropout replaced by the given multiplier
        project = torch.tanh(z @ W1.t() + b1) @ w2.reshape(16, 1)
        beta = torch.softmax(project, dim=1)
        if with_mult:
            beta = beta * t["M"].unsqueeze(-1)
        out = (beta * z).sum(1)
        grads = torch.autograd.grad(out, leaves, t["g"])
        want = dict(zip(K.OUTPUTS, [out.detach(), beta.detach().squeeze(-1)] + [g for g in grads]))
        got = K.reference(d["A"], d["B"], d["W1"], d["b1"], d["w2"], d["M"] if with_mult else None, d["g"])
        for name in K.OUTPUTS:
            w = want[name].numpy()
            assert np.abs(got[name] - w).max() <= 1e-12 * np.abs(w).max(), name


def test_fp32_saturates_at_the_margins_of_the_exact_designs():
    assert torch.tanh(torch.tensor([16.0, -16.0, 0.0])).tolist() == [1.0, -1.0, 0.0]
    assert torch.softmax(torch.tensor([128.0, 0.0]), 0).tolist() == [1.0, 0.0]
    assert torch.softmax(torch.tensor([-384.0, -384.0]), 0).tolist() == [0.5, 0.5]
    assert K.PRE_UNIT >= 16 and K.SCORE_UNIT >= 128
    assert np.tanh(np.float64(K.PRE_UNIT)) == 1.0    # the float64 restatement saturates too


@pytest.mark.parametrize("mult", [False, True])
@pytest.mark.parametrize("n_rows,F", [(1, 128), (2, 128), (65, 4), (65, 8), (65, 132), (131, 128), (65, 512), (65537, 128)])
def test_exact_designs_keep_their_margins_classes_and_bound(n_rows, F, mult):
    d = K.exact_design(n_rows, F, mult)
    pre, s = K.exact_classes(d)
    assert np.all((pre == 0) | (np.abs(pre) >= 16)) and np.all(pre == np.round(pre))
    diff = s[:, 0] - s[:, 1]
    assert np.all((diff == 0) | (np.abs(diff) >= 128))
    for k in ("A", "B", "g", "W1", "b1", "w2"):
        assert np.all(d[k] == np.round(d[k])), k
    assert 8 * K.exact_bound(d) < 2 ** 24
    r = K.reference(d["A"], d["B"], d["W1"], d["b1"], d["w2"], d["M"], d["g"])
    r32 = {k: v.astype(np.float32) for k, v in r.items()}
    beta = r32["beta"] if d["M"] is None else r32["beta"] / np.where(d["M"] == 0, 1, d["M"]) * (d["M"] != 0)
    assert set(np.unique(beta)) <= {0.0, 0.5, 1.0}
    # the restatement rounded to fp32 is a multiple of 1 / 4 everywhere: nothing of it depends on a rounding
    for k in K.OUTPUTS:
        assert np.all(r32[k] * 4 == np.round(r32[k] * 4)), k
    for k in ("dW1", "db1", "dw2"):
        assert np.any(r32[k] != 0), k
    if n_rows >= 12:
        classes = {(float(a), float(b)) for a, b in K.reference(d["A"], d["B"], d["W1"], d["b1"], d["w2"], None, d["g"])["beta"]
                   .astype(np.float32)}
        assert classes == {(0.5, 0.5), (1.0, 0.0), (0.0, 1.0)}
        if mult:
            assert np.any((d["M"] == 0).all(1))
            assert np.any(r32["dA"][(d["M"] == 0).all(1)] == 0)


# ---------------------------------------------------------------------------------------------------------------------
# the designs of test_gpu_attention_forms.py do what that file relies on
FORMS_WIDTHS = (4, 12, 20, 28, 32, 36, 124, 132, 252, 260, 508, 512)
FORMS_PART_COUNTS = (15, 16, 17, 240, 241, 255, 256, 257, 1023)


def _forms_exact_cases():
    R, G = K.BLOCK_ROWS, _constant("DGMI_ATTN_MAX_WORKGROUPS")
    return ([(200, F) for F in FORMS_WIDTHS] + [(R * G + 2 * R + 3, 32), (R * G + 2 * R + 3, 260)]
            + [(R * k - 3, 16) for k in FORMS_PART_COUNTS])


def _every_block_contributes(d):
    p = K.block_partials(d)
    assert all(v.dtype == np.float32 and v.shape[0] == -(-d["A"].shape[0] // K.BLOCK_ROWS) for v in p.values())
    return {k: bool(np.all(np.any(v.reshape(v.shape[0], -1) != 0, axis=1))) for k, v in p.items()}


def test_block_rows_mirror_the_header():
    assert K.BLOCK_ROWS == _constant("DGMI_ATTN_BLOCK_ROWS")


@pytest.mark.parametrize("mult", [False, True])
@pytest.mark.parametrize("n_rows,F", _forms_exact_cases())
def test_every_block_of_the_forms_designs_adds_to_all_three_sums(n_rows, F, mult):
    """The width and partial-count cases of the forms file: fp32 is exact in any order, and EVERY block's partial of
    dW1, db1 and dw2 is non-zero after rounding, so a sum carried across blocks or across partials is a sum of non-zero
    terms.  The partials add up to the restatement's sums."""
    d = K.exact_design(n_rows, F, mult)
    assert 8 * K.exact_bound(d) < 2 ** 24
    assert _every_block_contributes(d) == {"dW1": True, "db1": True, "dw2": True}
    p = K.block_partials(d)
    r = K.reference(d["A"], d["B"], d["W1"], d["b1"], d["w2"], d["M"], d["g"])
    for k in p:
        assert np.array_equal(p[k].astype(np.float64).sum(0).astype(np.float32), r[k].astype(np.float32)), k


@pytest.mark.parametrize("mult", [False, True])
@pytest.mark.parametrize("n_rows,F", [(65, 16), (65, 128), (65, 512), (65537, 128)])
def test_the_first_suites_width_shapes_carry_no_second_partial(n_rows, F, mult):
    """Why the forms file has shapes of its own: at R + 1 and R G + 1 rows the lone row of the last block is of class 1
    (saturated softmax, ds = 0), so that block's partial of all three sums is exactly zero."""
    p = K.block_partials(K.exact_design(n_rows, F, mult))
    for k, v in p.items():
        assert not v[-1].any() and v[0].any(), k


def test_scaled_float_design_keeps_the_default_and_reaches_saturation():
    for shape in ((763, 128, 40), (1256, 256, 41)):
        plain, one = K.float_design(*shape), K.float_design(*shape, w1_scale=1, w2_scale=1)
        assert all(np.array_equal(plain[k], one[k]) and plain[k].dtype == np.float32 for k in plain)
        small, sat, least = K.regime(plain)
        assert small == 0.0 and sat < 1e-3 and least > 0.2                    # the linear regime of the first suite
        d = K.float_design(*shape, w1_scale=4, w2_scale=8)
        for k in ("A", "B", "g", "M"):
            assert np.array_equal(d[k], plain[k]), k
        assert np.array_equal(d["W1"], (4 * plain["W1"].astype(np.float64)).astype(np.float32))
        small, sat, least = K.regime(d)
        print("float_design%s x (4, 8): weight < 1e-3 in %.1f %% of rows, |h| > 0.99 in %.1f %% of units, least fp32 weight %.3g"
              % (shape, 100 * small, 100 * sat, least))
        assert small >= 0.15 and sat >= 0.10 and least > 0.0


def test_poison_and_classes():
    d = K.float_design(5, 8, 0)
    e = K.poison(d, "B", 3, 7, -np.inf)
    assert e["B"][3, 7] == -np.inf and np.isfinite(d["B"]).all() and e["A"] is d["A"] and e["B"] is not d["B"]
    c = K.classes(np.array([[1.0, np.nan], [np.inf, -np.inf]], dtype=np.float32))
    assert c.tolist() == [[K.FINITE, K.NAN], [K.POS_INF, K.NEG_INF]]
    cases = K.poison_cases()
    for operand in ("A", "B", "g", "M"):
        mine = [c for c in cases if c[0] == operand]
        assert {(c[1], c[2]) for c in mine} == {(r, col) for r in K.POISON_ROWS for col in K.POISON_COLS[operand]}
        assert {repr(c[3]) for c in mine} == {repr(v) for v in K.POISON_VALUES[operand]}


def test_poisoned_designs_have_one_class_map_in_any_precision_and_order():
    """For every poisoned design of the forms file: NaN / +Inf / -Inf / finite per element of the float64 restatement is
    also what the restatement gives in fp32 and with the columns reversed, except at the elements ``POISON_LEFT_OUT``
    names (at most 1 % of an output); the poisoned row is not finite unless the value is, and the restatement keeps a
    poisoned row out of every other row."""
    d0 = K.float_design(*K.POISON_SHAPE)
    assert K.regime(d0)[2] > 0.2                                                 # no weight underflows on this design
    clean = K.restate(d0)
    named = {}
    for case in K.poison_cases():
        operand, row, col, value = case
        d = K.poison(d0, *case)
        diff = K.class_disagreements(d)
        where = {k: [tuple(int(i) for i in idx) for idx in np.argwhere(v)] for k, v in diff.items() if v.any()}
        if where:
            named[(operand, row, col, repr(value))] = where
        for k, v in diff.items():
            assert v.sum() <= 0.01 * v.size, (case, k)
        r = K.restate(d)
        other = np.arange(d0["A"].shape[0]) != row
        for k in ("out", "beta", "dA", "dB"):
            assert np.array_equal(r[k][other], clean[k][other]), (case, k)
        if operand == "g":
            assert np.array_equal(r["out"], clean["out"]) and np.array_equal(r["beta"], clean["beta"])
        if not np.isfinite(value):
            assert not np.isfinite(r["dA"][row]).all() and not np.isfinite(r["dW1"]).all(), case
        else:
            assert all(np.isfinite(r[k]).all() for k in K.OUTPUTS), case
    assert named == K.POISON_LEFT_OUT
