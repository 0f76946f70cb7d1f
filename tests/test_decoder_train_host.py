"""The fused training decoder, host side (no GPU): include/dgmi_train.h declares exactly the new entry points, the
library exports them and ``TRAIN_SIGNATURES`` matches type for type; argument validation and workspace sizing return
codes before any launch; the numpy restatement of the dropout mask has the statistics a mask needs (share, independence
of the layers, of sequential seeds and of translated seeds); the exact designs are exact; the ``select`` form of the
restatement is the product form's bits on finite designs; the module design is exact under every seed; the non-finite
design keeps and drops its units under the test mask; the mask's extremes (p next to 0 and next to 1, negative seeds)."""
import ctypes
import math
import os
import re

import numpy as np
import pytest
import torch

import _decoder_train_cases as K

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY_POINTS = ["dgmi_pair_mlp_train_backward_f32", "dgmi_pair_mlp_train_forward_f32", "dgmi_pair_mlp_train_workspace_bytes"]
CTYPE = {"const float*": ctypes.c_void_p, "float*": ctypes.c_void_p, "const int32_t*": ctypes.c_void_p,
         "int32_t*": ctypes.c_void_p, "const int64_t*": ctypes.c_void_p, "void*": ctypes.c_void_p,
         "dgmi_stream_t": ctypes.c_void_p, "int64_t": ctypes.c_int64, "int32_t": ctypes.c_int32, "float": ctypes.c_float,
         "size_t": ctypes.c_size_t, "int": ctypes.c_int}


def _text():
    return open(os.path.join(ROOT, "include", "dgmi_train.h")).read()


def _prototypes():
    """name -> (return type, [parameter types]) as the header spells them."""
    out = {}
    for ret, name, params in re.findall(r"DGMI_API\s+([\w\s\*]+?)\s*\b(dgmi_\w+)\s*\(([^)]*)\)\s*;", _text()):
        types = [re.sub(r"\s*\w+$", "", " ".join(q.split())).replace(" *", "*") for q in params.split(",")]
        out[name] = (ret.strip(), types)
    return out


def test_header_declares_exactly_the_train_entry_points():
    assert sorted(_prototypes()) == ENTRY_POINTS
    assert '#include "dgmi.h"' in _text()


def test_table_matches_the_header_type_for_type_and_the_library_exports_it():
    from dream_gnn_amd import _lib

    protos = _prototypes()
    assert sorted(_lib.TRAIN_SIGNATURES) == ENTRY_POINTS
    for name, (res, args) in _lib.TRAIN_SIGNATURES.items():
        ret, types = protos[name]
        assert CTYPE[ret] is res, name
        assert [CTYPE[t] for t in types] == args, name
        fn = getattr(_lib.lib, name)
        assert fn.restype is res and list(fn.argtypes) == args, name
    for other in (_lib.SIGNATURES, _lib.PAIR_SIGNATURES, _lib.RANK_SIGNATURES, _lib.ABOVE_SIGNATURES, _lib.BF16_SIGNATURES,
                  _lib.GIVEN_SIGNATURES, _lib.CURVE_SIGNATURES, _lib.LAYOUT_SIGNATURES):
        assert not set(_lib.TRAIN_SIGNATURES) & set(other)


_BASE = dict(X=16, ldx=128, n_query=100, C=16, ldc=128, n_cand=50, h1=128, h2=64, W2=16, b2=16, w3=16, b3=16, pq=16, pc=16,
             n_pairs=40, p=0.25, seed=16, ol=16, oi=16, dl=16, dz1=16, ld=128, dW2=16, db2=16, dw3=16, db3=16, ws=16,
             wsb=1 << 40, stream=None)


def _operands(a):
    return [a[k] for k in ("X", "ldx", "n_query", "C", "ldc", "n_cand", "h1", "h2", "W2", "b2", "w3", "b3", "pq", "pc", "n_pairs",
                           "p", "seed")]


def _forward(L, **kw):
    a = dict(_BASE)
    a.update(kw)
    return L.dgmi_pair_mlp_train_forward_f32(*_operands(a), a["ol"], a["oi"], a["stream"])


def _backward(L, **kw):
    a = dict(_BASE)
    a.update(kw)
    return L.dgmi_pair_mlp_train_backward_f32(*_operands(a), a["dl"], a["dz1"], a["ld"], a["dW2"], a["db2"], a["dw3"], a["db3"],
                                              a["oi"], a["ws"], a["wsb"], a["stream"])


@pytest.mark.parametrize("call", [_forward, _backward])
def test_argument_validation_returns_codes_without_a_gpu(call):
    from dream_gnn_amd import _lib

    L = _lib.lib
    assert call(L, h1=256) == -1 and call(L, h2=32) == -1                       # only the reference's widths
    assert call(L, ldx=127) == -1 and call(L, ldc=64) == -1 and call(L, ldx=130) == -1 and call(L, ldc=134) == -1
    for name in ("X", "C", "W2", "b2", "w3", "b3", "pq", "pc", "seed", "oi"):    # null pointers
        assert call(L, **{name: None}) == -1, name
    assert call(L, X=20) == -1 and call(L, C=24) == -1 and call(L, W2=8) == -1   # not 16-B aligned
    for p in (-0.01, 1.0, 1.5, float("nan"), float("inf")):
        assert call(L, p=p) == -1, p
    assert call(L, n_query=2 ** 31) == -1 and call(L, n_cand=2 ** 31) == -1 and call(L, n_pairs=2 ** 31) == -1
    assert call(L, n_query=-1) == -1 and call(L, n_cand=-1) == -1 and call(L, n_pairs=-1) == -1
    assert call(L, n_pairs=0, p=1.0) == -1 and call(L, n_pairs=0, h1=64) == -1   # an empty list excuses no bad argument


def test_forward_and_backward_own_arguments():
    from dream_gnn_amd import _lib

    L = _lib.lib
    assert _forward(L, n_pairs=0) == 0 and _forward(L, n_pairs=0, X=None, C=None, pq=None, pc=None, ol=None) == 0
    assert _forward(L, ol=None) == -1
    for name in ("dl", "dz1", "dW2", "db2", "dw3", "db3"):
        assert _backward(L, **{name: None}) == -1, name
    assert _backward(L, n_pairs=0, dW2=None) == -1                               # they are written even then
    assert _backward(L, ld=127) == -1 and _backward(L, ld=130) == -1 and _backward(L, dz1=24) == -1
    assert _backward(L, ws=None) == -3 and _backward(L, wsb=64) == -3            # workspace missing / short
    assert _backward(L, wsb=L.dgmi_pair_mlp_train_workspace_bytes(40) - 1) == -3


def test_workspace_sizing_is_monotone_host_arithmetic():
    from dream_gnn_amd import _lib

    W = _lib.lib.dgmi_pair_mlp_train_workspace_bytes
    assert W(0) == 0 and W(-1) == 0 and W(2 ** 31) == 0 and W(-2 ** 40) == 0
    ns = [1, 2, 127, 128, 129, 1000, 32_768, 32_769, 40_000, 467_643, 816_000, 2 ** 31 - 1]
    sizes = [W(n) for n in ns]
    assert sizes[0] > 0 and sizes == sorted(sizes) and sizes[3] < sizes[4]
    assert all(s % 256 == 0 for s in sizes)
    # dZ2 (n x 64 fp32) plus one 64 x 128 partial and one small partial per workgroup, at most 256 workgroups
    assert W(467_643) <= 467_643 * 256 + 256 * (8192 + 132) * 4 + 3 * 256


def test_torch_ops_are_registered():
    from dream_gnn_amd import _lib  # noqa: F401

    ns = torch.ops.dreamgnn_mi
    names = ["X", "C", "W2", "b2", "w3", "b3", "pair_query", "pair_cand", "p", "seed"]
    assert [a.name for a in ns.pair_mlp_train_forward.default._schema.arguments] == names
    assert [a.name for a in ns.pair_mlp_train_backward.default._schema.arguments] == names + ["dlogit"]
    assert len(ns.pair_mlp_train_forward.default._schema.returns) == 2
    assert len(ns.pair_mlp_train_backward.default._schema.returns) == 6
    z = (torch.zeros(2, 128), torch.zeros(2, 128), torch.zeros(64, 128), torch.zeros(64), torch.zeros(64), torch.zeros(1),
         torch.zeros(1, dtype=torch.int32), torch.zeros(1, dtype=torch.int32), 0.5, torch.zeros(1, dtype=torch.int64))
    with pytest.raises(NotImplementedError):  # no CPU kernel
        ns.pair_mlp_train_forward(*z)
    with pytest.raises(NotImplementedError):
        ns.pair_mlp_train_backward(*z, torch.zeros(1))


def test_module_flag_is_opt_in_and_keeps_the_state_dict():
    from dream_gnn_amd import model as M

    assert M.MLPDecoder.fused_training is False
    torch.manual_seed(0)
    a = M.MLPDecoder(8, 0.1)
    torch.manual_seed(0)
    b = M.MLPDecoder(8, 0.1, fused_training=True)
    assert a.fused_training is False and b.fused_training is True
    assert list(a.state_dict()) == list(b.state_dict())
    assert all(torch.equal(x, y) for x, y in zip(a.state_dict().values(), b.state_dict().values()))  # same RNG consumption


# ---------------------------------------------------------------------------------------------------------------------
# the mask function, restated
P_DROP, N_E = 0.3, 4096
SEED = 0x1234_5678_9ABC_DEF1


def _within(share, expect, n):
    """|share - expect| <= 5 sigma of a Bernoulli(expect) mean over n elements."""
    return abs(share - expect) <= 5.0 * math.sqrt(expect * (1.0 - expect) / n)


def test_kept_share_matches_one_minus_p():
    m1, m2 = K.masks(SEED, N_E, P_DROP)
    assert m1.shape == (N_E, 128) and m2.shape == (N_E, 64)
    assert _within(m1.mean(), 0.7, m1.size)                    # sigma = sqrt(0.21 / n)
    assert _within(m2.mean(), 0.7, m2.size)
    # no unit and no pair is special
    assert np.all(np.abs(m1.mean(0) - 0.7) <= 5 * math.sqrt(0.21 / N_E))
    assert np.all(np.abs(m1.mean(1) - 0.7) <= 5.5 * math.sqrt(0.21 / 128))


def test_layers_seeds_and_translates_are_independent():
    agree = P_DROP ** 2 + (1 - P_DROP) ** 2
    m1, m2 = K.masks(SEED, N_E, P_DROP)
    assert _within((m1[:, :64] == m2).mean(), agree, m2.size)  # layer 1 against layer 2 on the units they share
    n1, n2 = K.masks(SEED + 1, N_E, P_DROP)                      # sequential seeds
    assert _within((m1 == n1).mean(), agree, m1.size) and _within((m2 == n2).mean(), agree, m2.size)
    # seed s against s ^ 3 at element i ^ 3: an element hash that XORs the raw seed into the index makes these EQUAL
    e, j1, j2 = np.arange(N_E)[:, None], np.arange(128)[None, :], np.arange(64)[None, :]
    for layer, j, m in ((1, j1, m1), (2, j2, m2)):
        assert _within((m == K.keep(SEED ^ 3, layer, e ^ 3, j, P_DROP)).mean(), agree, m.size)
        assert _within((m == K.keep(SEED ^ 3, layer, e, j ^ 3, P_DROP)).mean(), agree, m.size)
        flat = e * m.shape[1] + j                                # ... and with i the flat index of the E x H tensor
        ft = flat ^ 3
        assert _within((m == K.keep(SEED ^ 3, layer, ft // m.shape[1], ft % m.shape[1], P_DROP)).mean(), agree, m.size)


def test_p_zero_keeps_all_and_scales_are_rounded_once():
    m1, m2 = K.masks(SEED, 257, 0.0)
    assert m1.all() and m2.all()
    assert K.threshold(0.0) == 2 ** 32 and K.scale(0.0) == np.float32(1.0)
    assert K.scale(0.5) == np.float32(2.0) and K.threshold(0.5) == 2 ** 31
    assert K.threshold(0.3) == math.floor((1.0 - float(np.float32(0.3))) * 2 ** 32)
    assert K.scale(0.3).dtype == np.float32


def test_mask_is_keyed_by_position_not_by_pair():
    m1, _ = K.masks(SEED, 64, 0.5)
    assert not np.array_equal(m1[0], m1[1])  # two positions of (what may be) one pair


@pytest.mark.parametrize("E", K.EXACT_SIZES)
def test_exact_designs_are_exact_and_have_their_special_nodes_and_units(E):
    d = K.exact_design(E)
    for p in (0.5, 0.0):
        assert K.exact_margin(d, p, SEED) < 2 ** 24
    src, dst = d["src"], d["dst"]
    assert not np.any(src == 1)                                                      # a node with no pair
    z1 = d["P"][src] + d["Q"][dst]
    assert np.all(z1[:, 5] < 0) and np.all(z1[:, 6] > 0)                             # never / always positive
    r = K.reference(d["P"], d["Q"], d["W2"], d["b2"], d["w3"], d["b3"], src, dst, 0.5, SEED, d["g"])
    assert np.all(r["z2"][:, 3] < 0) and np.all(r["z2"][:, 4] > 0)
    if E >= 129:
        assert np.sum(src == 0) >= min(E // 4, 3000)                                 # a node with (up to) thousands
        pairs = np.stack([src, dst], 1)
        assert len(np.unique(pairs, axis=0)) < E                                     # duplicated pairs
    if E == 40_000:
        assert np.sum(src == 0) >= 3000


# ---------------------------------------------------------------------------------------------------------------------
# the two forms of the restatement, the module design, the non-finite design, the mask's extremes
def _same(a, b, keys):
    for k in keys:
        assert a[k].dtype == b[k].dtype and np.array_equal(a[k], b[k]), k


OUTPUTS = ("logit", "z2", "dz1") + K.GRADS


@pytest.mark.parametrize("E", K.EXACT_SIZES)
def test_select_and_product_forms_are_the_same_bits_on_the_integer_designs(E):
    d = K.exact_design(E)
    for p in (0.5, 0.0):
        for absolute in (False, True):
            _same(K.ref_of(d, p, SEED, form="select", absolute=absolute), K.ref_of(d, p, SEED, absolute=absolute), OUTPUTS)


@pytest.mark.parametrize("design", ["float-5000-settled", "float-129", "float-40000", "module-33", "module-385"])
def test_select_and_product_forms_are_the_same_bits_on_the_other_finite_designs(design):
    kind, E = design.split("-")[0], int(design.split("-")[1])
    p = 0.3 if kind == "float" else 0.5
    if kind == "module":
        d = K.module_design(E)
    else:
        d = K.float_design(E, settle=(p, SEED)) if design.endswith("settled") else K.float_design(E, seed=21 if E > 129 else E)
    for absolute in (False, True):
        _same(K.ref_of(d, p, SEED, form="select", absolute=absolute), K.ref_of(d, p, SEED, absolute=absolute), OUTPUTS)


@pytest.mark.parametrize("E", [33, 385])
def test_module_designs_are_exact_under_every_seed(E):
    """The condition of the exact module test: sum|terms| of the two lin1 tables, of every output of the fused op and of
    the four gradients behind the tables, with EVERY gate open (the GPU test draws its seed on the device)."""
    d = K.module_design(E)
    for p in (0.5, 0.0):
        assert K.exact_margin(d, p, None) < 2 ** 24
        assert K.exact_margin(d, p, SEED) <= K.exact_margin(d, p, None)
    for k in ("hd", "hs", "W1", "b1", "W2", "b2", "w3", "b3", "g"):   # bf16 numbers: a GEMM may round its inputs
        t = torch.from_numpy(d[k])
        assert torch.equal(t.bfloat16().float(), t), k
    r, P = K.module_reference(d, 0.5, SEED), K.module_tables(d)
    assert np.array_equal(d["P"], P[0]) and np.array_equal(d["Q"], P[1]) and d["P"].dtype == np.float32
    assert r["dW1"].shape == d["W1"].shape and r["db1"].shape == d["b1"].shape and r["dhd"].shape == d["hd"].shape
    assert all(np.any(r[k]) for k in K.MODULE_GRADS) or E < 33
    # the chain rule against float64 autograd of the same expression
    t = {k: torch.from_numpy(d[k]).double().requires_grad_(k in ("hd", "hs", "W1", "b1")) for k in ("hd", "hs", "W1", "b1")}
    Pt = t["hd"] @ t["W1"][:, :K.MODULE_F].t() + t["b1"]
    Qt = t["hs"] @ t["W1"][:, K.MODULE_F:].t()
    (Pt * torch.from_numpy(r["dP"])).sum().backward(retain_graph=True)
    (Qt * torch.from_numpy(r["dQ"])).sum().backward()
    for k, name in (("hd", "dhd"), ("hs", "dhs"), ("W1", "dW1"), ("b1", "db1")):
        assert np.array_equal(t[k].grad.numpy(), r[name]), name
    src = d["src"]
    assert not np.any(src == 1) and np.sum(src == 0) >= E // 4 and len(np.unique(np.stack([src, d["dst"]], 1), axis=0)) < E


def test_upstream_gradient_of_ones_keeps_the_integer_design_exact():
    d = K.exact_design(385)
    assert K.exact_margin(d, 0.5, SEED, g=np.ones(385)) < 2 ** 24


def test_nonfinite_design_keeps_and_drops_its_units_under_the_test_mask():
    d = K.nonfinite_design()
    E, src, dst, touch = K.NONFINITE_E, d["src"], d["dst"], d["touch"]
    m1, _ = K.masks(SEED, E, 0.5)
    one = np.nonzero(src == K.NF_NAN_ONE)[0]
    row = np.nonzero(src == K.NF_NAN_ROW)[0]
    inf = np.nonzero((dst == K.NF_DST) & (src != K.NF_NEG_INF))[0]
    clash = np.nonzero((dst == K.NF_DST) & (src == K.NF_NEG_INF))[0]
    low = np.nonzero((dst != K.NF_DST) & (src == K.NF_NEG_INF))[0]
    assert len(one) >= 8 and len(row) >= 3 and len(inf) >= 8 and len(clash) >= 5 and len(low) >= 2
    assert np.isnan(d["P"][K.NF_NAN_ONE]).sum() == 1 and np.isnan(d["P"][K.NF_NAN_ROW]).all()
    assert d["Q"][K.NF_DST, K.NF_COL_INF] == np.inf and d["Q"][K.NF_DST, K.NF_COL_NEG] == -np.inf
    assert np.isfinite(d["Q"]).sum() == d["Q"].size - 2 and d["P"][K.NF_NEG_INF, K.NF_COL_INF] == -np.inf
    assert touch.sum() == len(one) + len(row) + len(inf) + len(clash) + len(low) and not d["g"][touch].any()
    assert d["g"][~touch].any() and np.isfinite(d["finite"]["P"]).all() and np.isfinite(d["finite"]["Q"]).all()
    assert K.exact_margin(d["finite"], 0.5, SEED) < 2 ** 24 and K.exact_margin(d["finite"], 0.0, SEED) < 2 ** 24
    # kept at some positions, dropped at others
    for pos, col in ((one, K.NF_COL_NAN), (inf, K.NF_COL_INF), (clash, K.NF_COL_INF)):
        assert m1[pos, col].any() and not m1[pos, col].all(), (pos, col)
    r = K.ref_of(d, 0.5, SEED, form="select")
    logit = r["logit"]
    assert np.array_equal(np.isnan(logit[one]), m1[one, K.NF_COL_NAN])         # finite exactly where the NaN is dropped
    assert np.array_equal(np.isfinite(logit[inf]), ~m1[inf, K.NF_COL_INF])    # kept +Inf: 0 * Inf or Inf - Inf in z2
    assert np.array_equal(np.isnan(logit[clash]), m1[clash, K.NF_COL_INF])    # Inf - Inf = NaN in z1 itself
    assert np.isnan(logit[row]).all() and np.isfinite(logit[low]).all()       # relu(-Inf + finite) = 0
    assert np.isfinite(logit[~touch]).all()
    # a pair of two finite nodes: the bits of the design with the non-finite rows zeroed; dz1 is finite everywhere
    f = K.ref_of(d["finite"], 0.5, SEED, form="select")
    assert np.array_equal(logit[~touch], f["logit"][~touch]) and np.array_equal(r["dz1"], f["dz1"])
    assert np.isfinite(r["dz1"]).all() and not r["dz1"][touch].any()
    for k in ("dP", "dQ", "db2", "db3"):
        assert np.array_equal(r[k], f[k]), k
    # numpy's product does what the contract says of the sums: 0 * NaN is NaN (column k of dW2, entry h of dw3)
    with np.errstate(invalid="ignore"):
        s, g = 2.0, d["g"].astype(np.float64)
        z1 = d["P"].astype(np.float64)[src] + d["Q"].astype(np.float64)[dst]
        h1 = np.where(m1, np.maximum(z1, 0.0) * s, 0.0)
    bad_k = ~np.isfinite(h1).all(0)
    assert bad_k[K.NF_COL_NAN] and bad_k[K.NF_COL_INF] and not bad_k.all()  # the all-NaN row is dropped in some columns
    assert np.array_equal(np.isnan(r["dW2"]), np.broadcast_to(bad_k, (64, 128)))
    _, m2 = K.masks(SEED, E, 0.5)
    with np.errstate(invalid="ignore"):
        bad_h = ~np.isfinite(np.where(m2, np.maximum(r["z2"], 0.0) * s, 0.0)).all(0)
    assert bad_h.any() and np.array_equal(np.isnan(r["dw3"]), bad_h) and g[~touch].any()
    print("dW2 columns NaN: %d of 128, dw3 entries NaN: %d of 64" % (bad_k.sum(), bad_h.sum()))
    # the product form, which is the torch chain's, differs: a dropped NaN stays NaN
    prod = K.ref_of(d, 0.5, SEED)["logit"]
    assert np.isnan(prod[one]).all() and not np.array_equal(np.isnan(prod), np.isnan(logit))


def test_mask_extremes_on_the_host():
    E = 129
    # p = 2^-24: thr = 0xFFFFFF00, scale 1 + 2^-23; p = 1e-12 and p just below 2^-33: thr = 2^32 - 1 (NOT 2^32: only a unit
    # whose hash is 0xFFFFFFFF goes), scale exactly 1, and under the test seed every unit of 129 pairs is kept
    assert K.threshold(2.0 ** -24) == 0xFFFFFF00 and K.scale(2.0 ** -24) == np.float32(1.0 + 2.0 ** -23)
    for p in (1e-12, float(np.nextafter(np.float32(2.0 ** -33), np.float32(0)))):
        assert K.threshold(p) == 2 ** 32 - 1 and K.scale(p) == np.float32(1.0)
        assert all(m.all() for m in K.masks(SEED, E, p))
    assert K.threshold(2.0 ** -60) == 2 ** 32                    # 1 - p is 1.0 in double: the "keep all" branch
    m1, m2 = K.masks(SEED, E, 2.0 ** -24)
    assert m1.all() and m2.all()                                 # 256 / 2^32 per unit: nothing goes at this size either
    # p = 0.999 and p = 1 - 2^-10 (scale exactly 1024): most pairs lose a whole layer
    assert K.scale(1.0 - 2.0 ** -10) == np.float32(1024.0) and K.threshold(1.0 - 2.0 ** -10) == 2 ** 22
    assert float(np.float32(1.0 - 2.0 ** -10)) == 1.0 - 2.0 ** -10
    assert K.scale(0.999) != np.float32(1000.0)
    for p in (0.999, 1.0 - 2.0 ** -10):
        for n, both in ((129, 0), (385, 1)):
            m1, m2 = K.masks(SEED, n, p)
            assert (~m2.any(1)).sum() >= 1 and (~m1.any(1)).sum() >= 1
            # at 129 pairs NO position keeps a unit in both layers under this seed (expected: 0.97 positions); at 385 one does
            assert (m1.any(1) & m2.any(1)).sum() == both, (p, n)
            assert m1.any() and m2.any()
    for n in (129, 385):                                         # the integer design at scale 1024, under the test seed
        assert K.exact_margin(K.exact_design(n), 1.0 - 2.0 ** -10, SEED) < 2 ** 24


def test_negative_seeds_are_their_two_complement_cast():
    """``(uint64_t)seed`` of the kernels: -1 is 2^64 - 1, -2^63 is 2^63; the five seeds of the device probes give five
    different masks with the share a mask needs."""
    for layer in (1, 2):
        assert K.layer_key(-1, layer) == K.layer_key(2 ** 64 - 1, layer) == K.mix64((K.mix64(2 ** 64 - 1) + layer) & K.M64)
        assert K.layer_key(-2 ** 63, layer) == K.layer_key(2 ** 63, layer)
        assert K.layer_key(0, layer) == K.mix64((K.mix64(0) + layer) & K.M64)
        assert len({K.layer_key(s, layer) for s in (SEED, 0, -1, -2 ** 63, 2 ** 63 - 1)}) == 5
    seen = []
    for s in (SEED, 0, -1, -2 ** 63, 2 ** 63 - 1):
        m1, m2 = K.masks(s, 129, 0.3)
        assert _within(m1.mean(), 0.7, m1.size) and _within(m2.mean(), 0.7, m2.size)
        assert m2.any(1).all()
        seen.append(m1)
    agree = P_DROP ** 2 + (1 - P_DROP) ** 2
    for i in range(5):
        for j in range(i):
            assert _within((seen[i] == seen[j]).mean(), agree, seen[i].size)
