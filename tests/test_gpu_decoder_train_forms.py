"""The fused training decoder where its first suite does not look, at ZERO tolerance unless a test says otherwise: the
module route with dropout (the rate ``MLPDecoder.forward`` hands to the op, the seed it draws, the gradients behind the
split ``lin1``), ids out of range through the registered ops (``EdgePairs`` refuses them earlier), non-finite rows under
the contract of include/dgmi_train.h (a dropped unit is exactly 0, a kept one follows IEEE), operand and gradient forms
(row-strided and misaligned tables with gradients, stride-0 and strided upstream gradients, ``requires_grad`` subsets, a
second backward, a side stream, a large list before a small one) and the largest dropout rates.

Every expected value comes from ``_decoder_train_cases.reference`` (float64, masks restated from the seed) on integer
designs whose sum|terms| stays below 2^24 (``test_decoder_train_host.py``), so fp32 equals it in any order."""
import numpy as np
import pytest
import torch

import _decoder_train_cases as K

pytestmark = pytest.mark.gpu

SEED = 0x1234_5678_9ABC_DEF1 % (1 << 62)
OPERANDS = ("P", "Q", "W2", "b2", "w3", "b3")


def _seed(dev, value=SEED):
    return torch.tensor([value], dtype=torch.int64, device=dev)


def _tensors(d, dev, grad=False):
    return [torch.from_numpy(d[k]).to(dev).requires_grad_(grad) for k in OPERANDS]


def _pairs(d, dev):
    from dream_gnn_amd import ops

    return ops.EdgePairs(torch.from_numpy(d["src"]).to(dev), torch.from_numpy(d["dst"]).to(dev), d["n_src"], d["n_dst"])


def _ids(a, dev):
    return torch.from_numpy(np.asarray(a).astype(np.int32)).to(dev)


def _raw(t, src, dst, p, seed, g):
    """The two registered ops on int32 id tensors that nothing has range-checked: dict of numpy outputs, both ``info``."""
    T = torch.ops.dreamgnn_mi
    args = (t[0], t[1], t[2], t[3].reshape(-1), t[4].reshape(-1), t[5].reshape(-1), src, dst, p, seed)
    logit, info_f = T.pair_mlp_train_forward(*args)
    dz1, dW2, db2, dw3, db3, info_b = T.pair_mlp_train_backward(*args, g)
    out = dict(logit=logit, dz1=dz1, dW2=dW2, db2=db2, dw3=dw3, db3=db3)
    return {k: v.cpu().numpy() for k, v in out.items()}, info_f.tolist(), info_b.tolist()


def _run(t, pairs, p, seed, g):
    """``ops.pair_mlp_train`` forward + ``backward(g)`` on leaves ``t``: dict of numpy outputs named as the restatement's."""
    from dream_gnn_amd import ops

    logit = ops.pair_mlp_train(*t, pairs, p, seed=seed)
    logit.backward(g)
    out = {"logit": logit.detach().cpu().numpy()}
    for name, x in zip(K.GRADS, t):
        out[name] = x.grad.cpu().numpy().reshape(-1) if name in ("dw3", "db3") else x.grad.cpu().numpy()
    return out


def _same(got, want, names, what=""):
    for name in names:
        assert got[name].dtype == np.float32, (what, name)
        want64 = np.asarray(want[name], dtype=np.float64)
        assert np.array_equal(got[name].astype(np.float64), want64, equal_nan=True), (what, name)


ALL = ("logit",) + K.GRADS


# ---------------------------------------------------------------------------------------------------------------------
# A. the module route with dropout
class _Graph:
    def __init__(self, pairs):
        self._pairs = pairs

    def edge_pairs(self):
        return self._pairs


def _decoder(d, dev, rate=0.5):
    from dream_gnn_amd import model as M

    dec = M.MLPDecoder(K.MODULE_F, rate, fused_training=True)
    with torch.no_grad():
        for prm, k in ((dec.lin1.weight, "W1"), (dec.lin1.bias, "b1"), (dec.lin2.weight, "W2"), (dec.lin2.bias, "b2"),
                       (dec.lin3.weight, "w3"), (dec.lin3.bias, "b3")):
            prm.copy_(torch.from_numpy(d[k]).reshape(prm.shape))
    return dec.to(dev)


def _module_step(dec, graph, d, dev, backward=True):
    """One forward (+ backward) of the module: numpy outputs named as ``module_reference``'s, and the seed it drew."""
    from dream_gnn_amd import ops

    hd, hs = (torch.from_numpy(d[k]).to(dev).requires_grad_(backward) for k in ("hd", "hs"))
    dec.zero_grad(set_to_none=True)
    ops.pair_mlp_train.last_seed = None
    y = dec(graph, hd, hs)
    assert y.shape == (len(d["src"]), 1) and y.dtype == torch.float32
    seed = None if ops.pair_mlp_train.last_seed is None else int(ops.pair_mlp_train.last_seed)
    out = {"logit": y.detach().squeeze(-1).cpu().numpy()}
    if backward:
        y.backward(torch.from_numpy(d["g"]).to(dev).unsqueeze(-1))
        grads = dict(dhd=hd.grad, dhs=hs.grad, dW1=dec.lin1.weight.grad, db1=dec.lin1.bias.grad, dW2=dec.lin2.weight.grad,
                     db2=dec.lin2.bias.grad, dw3=dec.lin3.weight.grad.reshape(-1), db3=dec.lin3.bias.grad)
        out.update({k: v.cpu().numpy() for k, v in grads.items()})
    return out, seed


MODULE_OUT = ("logit", "dhd", "dhs", "dW1", "db1", "dW2", "db2", "dw3", "db3")


@pytest.mark.parametrize("E", [33, 385])
def test_module_route_with_dropout_equals_the_float64_module(dev, E):
    """``MLPDecoder(F, 0.5, fused_training=True).train()``: logits, both embedding gradients and all six parameter
    gradients EQUAL the float64 restatement of the module with p = 0.5 and the seed the forward drew.  No dropout, another
    rate or torch's dropout on top of the kernel's cannot pass; nor can a wrong gradient behind the split ``lin1``."""
    d = K.module_design(E)
    assert K.exact_margin(d, 0.5, None) < 2 ** 24  # every gate open: exact under whatever seed is drawn
    dec, graph = _decoder(d, dev).train(), _Graph(_pairs(d, dev))
    F = K.MODULE_F
    # premise: the GEMM library is exact on these operands, forward and backward (a failure here is about the library)
    hd, hs, W1, b1 = (torch.from_numpy(d[k]).to(dev) for k in ("hd", "hs", "W1", "b1"))
    assert torch.equal(torch.addmm(b1, hd, W1[:, :F].t()).cpu(), torch.from_numpy(d["P"]))
    assert torch.equal((hs @ W1[:, F:].t()).cpu(), torch.from_numpy(d["Q"]))
    r0 = K.module_reference(d, 0.5, SEED)
    for tab, x, w, dx, dw in (("dP", hd, W1[:, :F], "dhd", r0["dW1"][:, :F]), ("dQ", hs, W1[:, F:], "dhs", r0["dW1"][:, F:])):
        up = torch.from_numpy(r0[tab]).float().to(dev)
        assert torch.equal(up.cpu().double(), torch.from_numpy(r0[tab]))
        assert torch.equal((up @ w).cpu().double(), torch.from_numpy(r0[dx]))
        assert torch.equal((x.t() @ up).cpu().double(), torch.from_numpy(dw).t())
        assert torch.equal(up.sum(0).cpu().double(), torch.from_numpy(r0[tab].sum(0)))

    got, seed = _module_step(dec, graph, d, dev)
    assert seed is not None and 0 <= seed < 2 ** 62
    _same(got, K.module_reference(d, 0.5, seed), MODULE_OUT, "train")
    m1, m2 = K.masks(seed, E, 0.5)
    assert not m1.all() and not m2.all()
    again, seed2 = _module_step(dec, graph, d, dev)  # one forward draws one seed; the next one another
    assert seed2 != seed
    _same(again, K.module_reference(d, 0.5, seed2), MODULE_OUT, "second draw")

    # train() under no_grad still draws masks
    with torch.no_grad():
        got, seed3 = _module_step(dec, graph, d, dev, backward=False)
    assert seed3 not in (None, seed, seed2)
    _same(got, K.module_reference(d, 0.5, seed3), ("logit",), "train, no_grad")

    # eval() with grad: the training kernels without dropout; under no_grad: the list scorer, bit for bit
    dec.eval()
    got, seed4 = _module_step(dec, graph, d, dev)
    assert seed4 is not None
    _same(got, K.module_reference(d, 0.0, seed4), MODULE_OUT, "eval")
    with torch.no_grad():
        got_ng, none = _module_step(dec, graph, d, dev, backward=False)
        assert none is None  # the fused op did not run
        hd, hs = torch.from_numpy(d["hd"]).to(dev), torch.from_numpy(d["hs"]).to(dev)
        want = dec.score_pairs(hd, hs, torch.from_numpy(d["src"]).to(dev), torch.from_numpy(d["dst"]).to(dev))
    assert np.array_equal(got_ng["logit"], want.cpu().numpy()) and np.array_equal(got_ng["logit"], got["logit"])


def test_module_uses_the_rate_its_dropout_holds_now(dev):
    """``dec.dropout.p = 0.25`` after construction is the rate used: scale 4/3 rounded once, so the logits are compared
    under the elementwise bar 1e-5 x sum|terms|.  The gradients are not: with a scale that is no power of two a ``z2``
    that is exactly 0 in float64 is a rounding residue in fp32, and its relu gate is a property of the inputs (what
    ``float_design(settle=...)`` removes); they are pinned exactly at p = 0.5 above."""
    E = 385
    d = K.module_design(E)
    dec, graph = _decoder(d, dev, rate=0.5).train(), _Graph(_pairs(d, dev))
    dec.dropout.p = 0.25
    got, seed = _module_step(dec, graph, d, dev)
    ref, mag = K.module_reference(d, 0.25, seed), K.module_reference(d, 0.25, seed, absolute=True)
    err, bar = np.abs(got["logit"].astype(np.float64) - ref["logit"]), 1e-5 * mag["logit"]
    print("dropout.p = 0.25, worst logit |err| / (1e-5 sum|terms|): %.4f" % float(np.max(err / bar)))
    assert np.all(bar > 0) and np.all(err <= bar), float(np.max(err / bar))
    m1, m2 = K.masks(seed, E, 0.25)
    assert not m1.all() and not m2.all()
    # and it is not the constructor's rate: the p = 0.5 module under the same seed is far outside the bar
    other = K.module_reference(d, 0.5, seed)["logit"]
    assert np.mean(np.abs(other - ref["logit"]) > bar) > 0.5


def test_whole_model_gradients_agree_with_the_flag_on_and_off(dev):
    """``dropout = attention_dropout = 0``, one eager ``forward_loss`` + backward from one ``state_dict``: every
    parameter gradient within 1e-4 max|g| of the torch chain's, tensor by tensor, the loss within 1e-5 relative."""
    from dream_gnn_amd import harness as H, model as M, ops
    from test_gpu_training import _problem

    batch, labels, args = _problem(dev)
    args.dropout, args.attention_dropout = 0.0, 0.0
    torch.manual_seed(1)
    nets = [M.Net(args).to(dev).train() for _ in range(2)]
    nets[1].load_state_dict(nets[0].state_dict())
    nets[1].decoder.fused_training = True
    res = []
    for net in nets:
        ops.pair_mlp_train.last_seed = None
        loss, _ = H.forward_loss(net, batch, labels, 0.1)
        loss.backward()
        assert (ops.pair_mlp_train.last_seed is not None) == net.decoder.fused_training  # the route that was asked for
        res.append((float(loss.detach()), {k: q.grad for k, q in net.named_parameters() if q.grad is not None}))
    (l0, g0), (l1, g1) = res
    assert abs(l1 - l0) <= 1e-5 * abs(l0), (l0, l1)
    assert list(g0) == list(g1) and any(k.startswith("decoder.lin1") for k in g0)
    for k in g0:
        top = float(g0[k].abs().max())
        assert g1[k].shape == g0[k].shape and float((g1[k] - g0[k]).abs().max()) <= 1e-4 * top, k


# ---------------------------------------------------------------------------------------------------------------------
# B. ids out of range
GUARD, MAGNET = 2, 100.0


def _guarded(x, dev):
    """``x`` as a row range inside a larger tensor the test owns, with finite magnet rows before and after it."""
    buf = torch.full((x.shape[0] + 2 * GUARD, x.shape[1]), MAGNET, device=dev)
    buf[GUARD:GUARD + x.shape[0]] = torch.from_numpy(x).to(dev)
    return buf, buf[GUARD:GUARD + x.shape[0]]


def test_ids_out_of_range_are_flagged_zeroed_and_never_read(dev):
    """E = 129, p = 0.5, ids -1 / n one row off either end of tables that lie inside owned buffers: positions 0 (first
    lane), 31 (wave edge), 32 (second wave), 64 and 128 (the lone pair of the last block); query side only, candidate
    side only, both."""
    from dream_gnn_amd import _lib

    E, p = 129, 0.5
    d = K.exact_design(E)
    nq, nc = d["n_src"], d["n_dst"]
    t = _tensors(d, dev)
    (bufP, t[0]), (bufQ, t[1]) = _guarded(d["P"], dev), _guarded(d["Q"], dev)
    assert t[0].is_contiguous() and t[0].data_ptr() == bufP.data_ptr() + GUARD * 128 * 4
    bad = {0: (-1, None), 31: (None, nc), 32: (nq, -1), 64: (nq, None), 128: (None, -1)}
    src, dst = d["src"].copy(), d["dst"].copy()
    for e, (q, c) in bad.items():
        src[e], dst[e] = (src[e] if q is None else q), (dst[e] if c is None else c)
    pos = np.array(sorted(bad))
    g = d["g"].copy()
    g[pos] = 2.0  # a gradient arrives at the bad positions and must go nowhere
    gz = g.copy()
    gz[pos] = 0.0
    seed = _seed(dev)
    got, info_f, info_b = _raw(t, _ids(src, dev), _ids(dst, dev), p, seed, torch.from_numpy(g).to(dev))
    clean, cinfo_f, cinfo_b = _raw(t, _ids(d["src"], dev), _ids(d["dst"], dev), p, seed, torch.from_numpy(gz).to(dev))
    assert info_f == [1, 0] and info_b == [1, 0] and cinfo_f == [0, 0] and cinfo_b == [0, 0]
    ok = np.ones(E, bool)
    ok[pos] = False
    assert np.isnan(got["logit"][pos]).all() and not np.isnan(got["logit"][ok]).any()
    assert np.array_equal(got["logit"][ok], clean["logit"][ok])
    assert not got["dz1"][pos].any() and np.array_equal(got["dz1"], clean["dz1"])
    for k in ("dW2", "db2", "dw3", "db3"):
        assert np.array_equal(got[k], clean[k]), k
    # ... and the clean list is right: the float64 restatement with the gradient zeroed there
    ref = K.ref_of(d, p, SEED, g=gz)
    _same(clean, ref, ("logit", "dz1", "dW2", "db2", "dw3", "db3"), "clean list")
    assert ref["dz1"][ok].any() and ref["dW2"].any()
    # the same backward through the C ABI into a strided buffer the test owns: guard rows and spare columns stay
    L = _lib.lib
    ld, fill = 132, -7.0
    out = torch.full((E + 2 * GUARD, ld), fill, device=dev)
    small = [torch.full((n + 8,), fill, device=dev) for n in (64 * 128, 64, 64, 1)]
    info = torch.full((2 + 8,), -7, dtype=torch.int32, device=dev)
    wb = L.dgmi_pair_mlp_train_workspace_bytes(E)
    ws = torch.full((wb + 4096,), 0xA5, dtype=torch.uint8, device=dev)
    pq, pc, gt = _ids(src, dev), _ids(dst, dev), torch.from_numpy(g).to(dev)
    b2, w3, b3 = (x.reshape(-1).contiguous() for x in t[3:])
    _lib.check(L.dgmi_pair_mlp_train_backward_f32(
        t[0].data_ptr(), 128, nq, t[1].data_ptr(), 128, nc, 128, 64, t[2].data_ptr(), b2.data_ptr(), w3.data_ptr(), b3.data_ptr(),
        pq.data_ptr(), pc.data_ptr(), E, p, seed.data_ptr(), gt.data_ptr(), out[GUARD].data_ptr(), ld, small[0].data_ptr(),
        small[1].data_ptr(), small[2].data_ptr(), small[3].data_ptr(), info.data_ptr(), ws.data_ptr(), wb,
        torch.cuda.current_stream().cuda_stream), "dgmi_pair_mlp_train_backward_f32")
    torch.cuda.synchronize()
    out, info = out.cpu().numpy(), info.cpu().numpy()
    assert np.array_equal(out[GUARD:GUARD + E, :128], got["dz1"])
    assert np.all(out[:GUARD] == fill) and np.all(out[GUARD + E:] == fill) and np.all(out[:, 128:] == fill)
    assert info[:2].tolist() == [1, 0] and np.all(info[2:] == -7)
    for x, k, n in zip(small, ("dW2", "db2", "dw3", "db3"), (64 * 128, 64, 64, 1)):
        x = x.cpu().numpy()
        assert np.array_equal(x[:n], got[k].reshape(-1)) and np.all(x[n:] == fill), k
    assert bool((ws[wb:] == 0xA5).all())
    # nothing wrote to the tables or their guard rows
    for buf, x in ((bufP, d["P"]), (bufQ, d["Q"])):
        b = buf.cpu().numpy()
        assert np.all(b[:GUARD] == MAGNET) and np.all(b[-GUARD:] == MAGNET) and np.array_equal(b[GUARD:-GUARD], x)


# ---------------------------------------------------------------------------------------------------------------------
# C. non-finite rows
def test_nonfinite_rows_follow_the_select_contract(dev):
    """A dropped unit is exactly 0 whatever lies under it, a kept unit follows IEEE (include/dgmi_train.h): NaN in one
    column, a row of NaN, +Inf / -Inf against finite rows and against each other, each kept at some positions and
    dropped at others (host test).  Logits NaN by position and finite bits equal; a pair of two finite nodes has the
    bits of the run with the non-finite rows zeroed; with ``dlogit = 0`` at every pair that names such a node, dZ1, dP,
    dQ, db2, db3 are exact and dW2 / dw3 are NaN exactly where the restatement's ``0 * NaN`` is."""
    E, p = K.NONFINITE_E, 0.5
    d = K.nonfinite_design(E)
    fin, touch = d["finite"], d["touch"]
    assert K.exact_margin(fin, p, SEED) < 2 ** 24
    ref = K.ref_of(d, p, SEED, form="select")
    seed, g = _seed(dev), torch.from_numpy(d["g"]).to(dev)
    got, info_f, info_b = _raw(_tensors(d, dev), _ids(d["src"], dev), _ids(d["dst"], dev), p, seed, g)
    assert info_f == [0, 0] and info_b == [0, 0]
    nan = np.isnan(ref["logit"])
    assert nan[touch].any() and np.isfinite(ref["logit"][touch]).any() and not nan[~touch].any()
    _same(got, ref, ("logit", "dz1", "dW2", "db2", "dw3", "db3"), "select reference")
    assert np.isfinite(got["dz1"]).all() and not got["dz1"][touch].any()
    assert np.isnan(got["dW2"]).any() and np.isfinite(got["dW2"]).any() and np.isnan(got["dw3"]).any()
    # one pair's column never leaks into another's: the finite pairs are those of the run without the non-finite rows
    zeroed, _, _ = _raw(_tensors(fin, dev), _ids(fin["src"], dev), _ids(fin["dst"], dev), p, seed, g)
    assert np.array_equal(got["logit"][~touch], zeroed["logit"][~touch]) and np.array_equal(got["dz1"], zeroed["dz1"])
    assert np.array_equal(got["db2"], zeroed["db2"]) and np.array_equal(got["db3"], zeroed["db3"])
    # the public op: the segment sums of dZ1 are finite and exact for every node
    out = _run(_tensors(d, dev, grad=True), _pairs(d, dev), p, seed, g)
    _same(out, ref, ALL, "ops.pair_mlp_train")
    assert np.isfinite(out["dP"]).all() and np.isfinite(out["dQ"]).all() and out["dP"].any()
    # p = 0 keeps every unit: the list scorer's bits, NaN by position
    from dream_gnn_amd import ops

    t = _tensors(d, dev)
    with torch.no_grad():
        a = ops.pair_mlp_train(*t, _pairs(d, dev), 0.0, seed=seed).cpu().numpy()
    b = torch.ops.dreamgnn_mi.pair_mlp_score_list(t[0], t[1], t[2], t[3].reshape(-1), t[4].reshape(-1), t[5].reshape(-1),
                                                  _ids(d["src"], dev), _ids(d["dst"], dev))[0].cpu().numpy()
    assert np.array_equal(a, b, equal_nan=True) and np.isnan(a[touch]).any()
    _same({"logit": a}, K.ref_of(d, 0.0, SEED, form="select"), ("logit",), "p = 0")


# ---------------------------------------------------------------------------------------------------------------------
# D. operand and gradient forms (E = 385, exact design, p = 0.5)
E_FORMS, P_FORMS = 385, 0.5


@pytest.fixture(scope="module")
def forms():
    """The design, its float64 restatement (computed once, never modified) and the restatement for ``g = 1``."""
    d = K.exact_design(E_FORMS)
    ref, ones = K.ref_of(d, P_FORMS, SEED), K.ref_of(d, P_FORMS, SEED, g=np.ones(E_FORMS))
    for r in (ref, ones):
        for v in r.values():
            v.setflags(write=False)
    return d, ref, ones


def _strided(x, dev):
    wide = torch.full((x.shape[0], 132), float("nan"), device=dev)
    wide[:, :128] = torch.from_numpy(x).to(dev)
    view = wide[:, :128].detach().requires_grad_(True)
    assert view.stride(0) == 132 and not view.is_contiguous() and view.data_ptr() == wide.data_ptr()
    return wide, view


def _offset(x, dev):
    flat = torch.zeros(x.size + 1, device=dev)
    flat[1:] = torch.from_numpy(x).to(dev).reshape(-1)
    view = flat[1:].view(x.shape).detach().requires_grad_(True)
    assert view.data_ptr() % 16 == 4 and view.is_contiguous()
    return flat, view


@pytest.mark.parametrize("form", ["row-strided", "off-16-bytes"])
def test_table_forms_with_gradients_equal_the_contiguous_run(dev, forms, form):
    d, ref, _ = forms
    pairs, g, seed = _pairs(d, dev), torch.from_numpy(d["g"]).to(dev), _seed(dev)
    base = _run(_tensors(d, dev, grad=True), pairs, P_FORMS, seed, g)
    _same(base, ref, ALL, "contiguous")
    t = _tensors(d, dev, grad=True)
    make = _strided if form == "row-strided" else _offset
    (ownP, t[0]), (ownQ, t[1]) = make(d["P"], dev), make(d["Q"], dev)
    got = _run(t, pairs, P_FORMS, seed, g)
    for name in ALL:
        assert np.array_equal(got[name], base[name]), name
    assert t[0].grad.shape == t[0].shape == (d["n_src"], 128) and t[1].grad.shape == (d["n_dst"], 128)
    if form == "row-strided":  # the spare columns: NaN before and after, the tables unchanged
        for own, x in ((ownP, d["P"]), (ownQ, d["Q"])):
            assert bool(torch.isnan(own[:, 128:]).all()) and np.array_equal(own[:, :128].cpu().numpy(), x)
    else:
        for own, x in ((ownP, d["P"]), (ownQ, d["Q"])):
            assert float(own[0]) == 0.0 and np.array_equal(own[1:].cpu().numpy(), x.reshape(-1))


def test_upstream_gradient_forms(dev, forms):
    """``sum().backward()`` (a stride-0 gradient), ``(logit * g).sum()``, and a gradient that is every second element of
    a 2E vector: the backward makes them contiguous, and every gradient equals the restatement."""
    from dream_gnn_amd import ops

    d, ref, ones = forms
    pairs, g, seed = _pairs(d, dev), torch.from_numpy(d["g"]).to(dev), _seed(dev)

    def grads(t):
        out = {}
        for name, x in zip(K.GRADS, t):
            out[name] = x.grad.cpu().numpy().reshape(-1) if name in ("dw3", "db3") else x.grad.cpu().numpy()
        return out

    t = _tensors(d, dev, grad=True)
    ops.pair_mlp_train(*t, pairs, P_FORMS, seed=seed).sum().backward()
    _same(grads(t), ones, K.GRADS, "sum().backward()")
    assert not np.array_equal(ones["dW2"], ref["dW2"])
    t = _tensors(d, dev, grad=True)
    (ops.pair_mlp_train(*t, pairs, P_FORMS, seed=seed) * g).sum().backward()
    _same(grads(t), ref, K.GRADS, "(logit * g).sum()")
    t = _tensors(d, dev, grad=True)
    two = torch.full((2 * E_FORMS,), float("nan"), device=dev)
    two[::2] = g
    assert two[::2].stride(0) == 2
    ops.pair_mlp_train(*t, pairs, P_FORMS, seed=seed).backward(two[::2])
    _same(grads(t), ref, K.GRADS, "every second element")


@pytest.mark.parametrize("wanted", [("W2", "b2", "w3", "b3"), ("P",), ("Q", "w3")], ids="+".join)
def test_requires_grad_subsets(dev, forms, wanted):
    from dream_gnn_amd import ops

    d, ref, _ = forms
    t = [torch.from_numpy(d[k]).to(dev).requires_grad_(k in wanted) for k in OPERANDS]
    logit = ops.pair_mlp_train(*t, _pairs(d, dev), P_FORMS, seed=_seed(dev))
    logit.backward(torch.from_numpy(d["g"]).to(dev))
    assert np.array_equal(logit.detach().cpu().numpy().astype(np.float64), ref["logit"])
    for k, name, x in zip(OPERANDS, K.GRADS, t):
        if k in wanted:
            assert x.grad is not None and x.grad.shape == x.shape
            assert np.array_equal(x.grad.cpu().numpy().astype(np.float64).reshape(ref[name].shape), ref[name]), k
        else:
            assert x.grad is None, k


def test_second_backward_raises(dev, forms):
    """The op is once-differentiable: differentiating its backward is an error, never a silent zero.  With an upstream
    gradient that is a constant the first-order gradient simply carries no graph; with one that depends on the logits
    (any real loss) autograd names the reason."""
    from dream_gnn_amd import ops

    d, ref, _ = forms
    t = _tensors(d, dev, grad=True)
    logit = ops.pair_mlp_train(*t, _pairs(d, dev), P_FORMS, seed=_seed(dev))
    (dP,) = torch.autograd.grad(logit, t[0], torch.from_numpy(d["g"]).to(dev), create_graph=True)
    assert np.array_equal(dP.detach().cpu().numpy().astype(np.float64), ref["dP"])
    assert not dP.requires_grad
    with pytest.raises(RuntimeError, match="does not require grad"):
        dP.sum().backward()
    logit = ops.pair_mlp_train(*t, _pairs(d, dev), P_FORMS, seed=_seed(dev))
    (dP,) = torch.autograd.grad((logit * logit).sum(), t[0], create_graph=True)
    assert dP.requires_grad
    with pytest.raises(RuntimeError, match="once_differentiable"):
        dP.sum().backward()


def test_side_stream_gives_the_default_streams_bits(dev, forms):
    """The backward's workspace is the per-(device, stream) scratch: a side stream has its own."""
    d, ref, _ = forms
    pairs, g, seed = _pairs(d, dev), torch.from_numpy(d["g"]).to(dev), _seed(dev)
    base = _run(_tensors(d, dev, grad=True), pairs, P_FORMS, seed, g)
    t = _tensors(d, dev, grad=True)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        got = _run(t, pairs, P_FORMS, seed, g)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    for name in ALL:
        assert np.array_equal(got[name], base[name]), name
    _same(got, ref, ALL, "side stream")


def test_large_list_then_small_list_on_one_stream(dev, forms):
    """The scratch grown for 40 000 pairs serves the next, smaller calls: all exact."""
    seed = _seed(dev)
    for E in (40_000, 33, E_FORMS):
        d = K.exact_design(E)
        got = _run(_tensors(d, dev, grad=True), _pairs(d, dev), P_FORMS, seed, torch.from_numpy(d["g"]).to(dev))
        _same(got, forms[1] if E == E_FORMS else K.ref_of(d, P_FORMS, SEED), ALL, "E = %d" % E)


# ---------------------------------------------------------------------------------------------------------------------
# E. the largest rates, on the integer design
@pytest.mark.parametrize("E", [129, 385])
def test_p_close_to_one_is_exact_and_a_pair_without_layer_two_is_the_bias(dev, E):
    """p = 1 - 2^-10: threshold 2^22, scale exactly 1024, and the integer design stays below 2^24 under the test seed (host
    test).  Most positions lose all of layer 2: their logit is exactly b3 and their dZ1 row exactly zero."""
    p = 1.0 - 2.0 ** -10
    d = K.exact_design(E)
    assert K.exact_margin(d, p, SEED) < 2 ** 24 and K.scale(p) == np.float32(1024.0)
    ref = K.ref_of(d, p, SEED)
    g = torch.from_numpy(d["g"]).to(dev)
    got, info_f, info_b = _raw(_tensors(d, dev), _ids(d["src"], dev), _ids(d["dst"], dev), p, _seed(dev), g)
    assert info_f == [0, 0] and info_b == [0, 0]
    _same(got, ref, ("logit", "dz1", "dW2", "db2", "dw3", "db3"), "p = 1 - 2^-10")
    _, m2 = K.masks(SEED, E, p)
    gone = ~m2.any(1)
    assert gone.any() and not gone.all()
    assert np.all(got["logit"][gone] == d["b3"][0]) and not got["dz1"][gone].any()
    assert np.any(got["logit"][~gone] != d["b3"][0])
    out = _run(_tensors(d, dev, grad=True), _pairs(d, dev), p, _seed(dev), torch.from_numpy(d["g"]).to(dev))
    _same(out, ref, ALL, "ops.pair_mlp_train")


def test_p_0999_meets_the_elementwise_bar(dev):
    """p = 0.999: the scale float32(1 / (1 - float32(0.999))) is no integer, so the bar is 1e-5 x sum|terms|; the positions
    without a layer-2 unit are still exactly b3."""
    E, p = 385, 0.999
    d = K.exact_design(E)
    ref, mag = K.ref_of(d, p, SEED), K.ref_of(d, p, SEED, absolute=True)
    got = _run(_tensors(d, dev, grad=True), _pairs(d, dev), p, _seed(dev), torch.from_numpy(d["g"]).to(dev))
    for name in ALL:
        err, bar = np.abs(got[name].astype(np.float64) - ref[name]), 1e-5 * mag[name]
        assert np.all(err <= bar), (name, float(np.max(err - bar)))
    _, m2 = K.masks(SEED, E, p)
    assert np.all(got["logit"][~m2.any(1)] == d["b3"][0])
