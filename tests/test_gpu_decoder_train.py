"""The fused training decoder on the device (``ops.pair_mlp_train``, ``MLPDecoder.fused_training``): the device mask is
the restated one; with p = 0 the logits are the list scorer's bits; on integer designs every output EQUALS the float64
restatement; random operands meet the elementwise bar; the module route matches the torch chain; gradients are the same
bits from run to run; autograd keeps nothing per pair; empty and bad input; HIP-graph capture draws a new mask per replay.
The module route WITH dropout, ids out of range, non-finite rows and the operand / gradient forms:
``test_gpu_decoder_train_forms.py``.

Measured on an MI355X (float parity, E = 5000, p = 0.3), worst |err| / (1e-5 sum|terms|): see DESIGN.md 4.15."""
import numpy as np
import pytest
import torch

import _decoder_train_cases as K

pytestmark = pytest.mark.gpu

SEED = 0x1234_5678_9ABC_DEF1 % (1 << 62)


def _dev(d, dev, grad=False):
    """The design's operands on the device: the six float operands (leaves when ``grad``), the pair list, the gradient."""
    from dream_gnn_amd import ops

    t = [torch.from_numpy(d[k]).to(dev).requires_grad_(grad) for k in ("P", "Q", "W2", "b2", "w3", "b3")]
    pairs = ops.EdgePairs(torch.from_numpy(d["src"]).to(dev), torch.from_numpy(d["dst"]).to(dev), d["n_src"], d["n_dst"])
    return t, pairs, torch.from_numpy(d["g"]).to(dev)


def _seed(dev, value=SEED):
    return torch.tensor([value], dtype=torch.int64, device=dev)


def _run(d, dev, p, seed):
    """Forward + backward of a design: dict of numpy outputs named as the restatement's."""
    from dream_gnn_amd import ops

    t, pairs, g = _dev(d, dev, grad=True)
    logit = ops.pair_mlp_train(*t, pairs, p, seed=seed)
    logit.backward(g)
    out = {"logit": logit.detach().cpu().numpy()}
    for name, x in zip(K.GRADS, t):
        out[name] = x.grad.cpu().numpy().reshape(-1) if name in ("dw3", "db3") else x.grad.cpu().numpy()
    return out


# ---------------------------------------------------------------------------------------------------------------------
# mask and p = 0 identity
MASK_CASES = [(0.3, SEED, 129), (0.999, SEED, 129), (2.0 ** -24, SEED, 129), (1e-12, SEED, 129), (0.3, 0, 129), (0.3, -1, 129),
              (0.3, -2 ** 63, 129), (0.3, 2 ** 63 - 1, 129), (0.999, SEED, 385)]


@pytest.mark.parametrize("p,seed_value,E", MASK_CASES, ids=lambda v: "%g" % v if isinstance(v, float) else str(v))
def test_device_mask_equals_the_restatement(dev, p, seed_value, E):
    """One-hot operands: with W2 = 0, b2 = 1, w3 = e_h the logit is scale * m2[e, h]; with P = 1, Q = 0, W2[:, k] = 1
    (other columns 0), b2 = 0, w3 = 1 it is scale^2 * m1[e, k] * (kept layer-2 units of e).  E = 129, p = 0.3 under five
    seeds (0, negative ones and both ends of int64: the kernels cast to uint64); under the first seed also p = 0.999
    (most pairs lose a whole layer; at 385 pairs one keeps a unit in both, at 129 none does: test_decoder_train_host.py),
    p = 2^-24 (thr = 0xFFFFFF00, scale 1 + 2^-23) and p = 1e-12 (thr = 2^32 - 1, scale 1: every unit kept)."""
    from dream_gnn_amd import ops

    rng = np.random.default_rng(3)
    src, dst = torch.from_numpy(rng.integers(0, 5, E)).to(dev), torch.from_numpy(rng.integers(0, 4, E)).to(dev)
    pairs = ops.EdgePairs(src, dst, 5, 4)
    seed = _seed(dev, seed_value)
    m1, m2 = K.masks(seed_value, E, p)
    s = float(K.scale(p))
    P, Q = torch.ones(5, 128, device=dev), torch.zeros(4, 128, device=dev)
    zero, one = torch.zeros(64, device=dev), torch.ones(64, device=dev)
    b3 = torch.zeros(1, device=dev)
    with torch.no_grad():
        got2 = torch.stack([ops.pair_mlp_train(P, Q, torch.zeros(64, 128, device=dev), one, torch.eye(64, device=dev)[h], b3,
                                               pairs, p, seed=seed) for h in range(64)], 1).cpu().numpy()
        cols = torch.eye(128, device=dev)
        got1 = torch.stack([ops.pair_mlp_train(P, Q, cols[k].expand(64, 128).contiguous(), zero, one, b3, pairs, p, seed=seed)
                            for k in range(128)], 1).cpu().numpy()
    assert np.array_equal(got2, m2 * np.float32(s))
    shows = m2.any(1)  # a pair that keeps a layer-2 unit shows its layer 1
    if p <= 0.3:
        assert shows.all()
    assert np.array_equal(got1 != 0, m1 & shows[:, None]) and np.all(got1 >= 0)
    if p == 0.3:
        assert not m1.all() and not m2.all() and m1.any() and m2.any()
    elif p < 0.3:
        assert m1.all() and m2.all()
        if s == 1.0:
            assert np.all(got1 == 64.0)
    else:
        assert (~shows).any() and (~m1.any(1)).any() and m1.any() and m2.any()
        assert bool((m1.any(1) & shows).any()) == (E == 385)


def test_p_one_hash_step_above_zero_is_the_p_zero_bits(dev):
    """p = 1e-12: every unit of the 129 pairs is kept (host test) and the scale is exactly 1, through the masked path."""
    from dream_gnn_amd import ops

    d = K.float_design(129, seed=129)
    t, pairs, _ = _dev(d, dev)
    assert all(m.all() for m in K.masks(SEED, 129, 1e-12)) and K.scale(1e-12) == np.float32(1.0) and K.threshold(1e-12) < 2 ** 32
    with torch.no_grad():
        got = ops.pair_mlp_train(*t, pairs, 1e-12, seed=_seed(dev))
        assert torch.equal(got, ops.pair_mlp_train(*t, pairs, 0.0, seed=_seed(dev)))
    assert torch.equal(got, ops.pair_mlp_score_list(*t, pairs.src, pairs.dst))


@pytest.mark.parametrize("E", [1, 31, 32, 33, 127, 128, 129, 385, 40_000])
def test_p_zero_logits_are_the_list_scorers_bits(dev, E):
    """Duplicates in the list, row-strided tables (ld = 132); 40 000 pairs are more list blocks than workgroups."""
    from dream_gnn_amd import ops

    d = K.float_design(E, seed=E)
    t, pairs, _ = _dev(d, dev)
    wide = [torch.zeros(x.shape[0], 132, device=dev) for x in t[:2]]
    for w, x in zip(wide, t[:2]):
        w[:, :128] = x
    P, Q = wide[0][:, :128], wide[1][:, :128]
    assert P.stride(0) == 132 and not P.is_contiguous()
    want = ops.pair_mlp_score_list(P, Q, *t[2:], pairs.src, pairs.dst)
    with torch.no_grad():
        got = ops.pair_mlp_train(P, Q, *t[2:], pairs, 0.0, seed=_seed(dev))
    assert got.shape == (E,) and torch.equal(got, want)
    assert torch.equal(got, ops.pair_mlp_train(t[0], t[1], *t[2:], pairs, 0.0, seed=_seed(dev, 99)).detach())  # any seed, any ld


# ---------------------------------------------------------------------------------------------------------------------
# exact gradients
@pytest.mark.parametrize("E,p", [(1, 0.5), (33, 0.5), (129, 0.5), (385, 0.5), (40_000, 0.5), (385, 0.0), (40_000, 0.0)])
def test_integer_designs_equal_the_float64_restatement(dev, E, p):
    d = K.exact_design(E)
    ref = K.reference(d["P"], d["Q"], d["W2"], d["b2"], d["w3"], d["b3"], d["src"], d["dst"], p, SEED, d["g"])
    got = _run(d, dev, p, _seed(dev))
    for name in ("logit",) + K.GRADS:
        assert got[name].dtype == np.float32
        assert np.array_equal(got[name].astype(np.float64), ref[name]), name
    assert not got["dP"][1].any() and got["dP"][0].any() == (E > 4)  # the node without a pair, the node with many
    assert not got["dW2"][3].any() and not got["dW2"][:, 5].any()   # the units that are never positive


# ---------------------------------------------------------------------------------------------------------------------
# float parity
def test_random_operands_meet_the_elementwise_bar(dev):
    """|err| <= 1e-5 x the same expression in float64 on the absolute values of every operand, for every output."""
    p = 0.3
    d = K.float_design(5000, settle=(p, SEED))
    a = (d["P"], d["Q"], d["W2"], d["b2"], d["w3"], d["b3"], d["src"], d["dst"], p, SEED, d["g"])
    ref, mag = K.reference(*a), K.reference(*a, absolute=True)
    # the design keeps every z2 ten bars away from 0, so fp32 and float64 take the same relu branches
    assert np.all(np.abs(ref["z2"]) > 1e-4 * mag["z2"])
    got = _run(d, dev, p, _seed(dev))
    worst = {}
    for name in ("logit",) + K.GRADS:
        err, bar = np.abs(got[name].astype(np.float64) - ref[name]), 1e-5 * mag[name]
        worst[name] = float(np.max(np.where(bar > 0, err / np.where(bar > 0, bar, 1.0), np.where(err > 0, np.inf, 0.0))))
    print("worst |err| / (1e-5 sum|terms|):", {k: round(v, 4) for k, v in worst.items()})
    for name, w in worst.items():
        assert w <= 1.0, (name, w)


# ---------------------------------------------------------------------------------------------------------------------
# module
class _Graph:
    def __init__(self, pairs):
        self._pairs = pairs

    def edge_pairs(self):
        return self._pairs


def _decoder_inputs(dev, E=3000, F=24):
    from dream_gnn_amd import ops

    rng = np.random.default_rng(11)
    src, dst = K.pair_list(rng, E, 50, 40)
    pairs = ops.EdgePairs(torch.from_numpy(src).to(dev), torch.from_numpy(dst).to(dev), 50, 40)
    g = torch.Generator().manual_seed(5)
    return _Graph(pairs), torch.randn(50, F, generator=g).to(dev), torch.randn(40, F, generator=g).to(dev)


def test_module_route_matches_the_torch_chain(dev):
    from dream_gnn_amd import model as M

    graph, hd, hs = _decoder_inputs(dev)
    torch.manual_seed(2)
    old = M.MLPDecoder(24, 0.0).to(dev).train()
    new = M.MLPDecoder(24, 0.0, fused_training=True).to(dev).train()
    new.load_state_dict(old.state_dict())
    assert list(new.state_dict()) == list(old.state_dict())
    dy = torch.randn(graph.edge_pairs().E, 1, device=dev)
    res = []
    for dec in (old, new):
        a, b = hd.clone().requires_grad_(True), hs.clone().requires_grad_(True)
        y = dec(graph, a, b)
        y.backward(dy)
        res.append((y.detach(), [a.grad, b.grad] + [q.grad for q in dec.parameters()]))
    (y0, g0), (y1, g1) = res
    assert y1.shape == y0.shape == (graph.edge_pairs().E, 1)
    assert float((y1 - y0).abs().max()) <= 1e-5 * float(y0.abs().max())
    for u, v in zip(g0, g1):
        assert v.shape == u.shape and float((v - u).abs().max()) <= 1e-4 * float(u.abs().max())
    # eval without grad: the list scorer; eval with grad: the training kernels without dropout: the same bits
    new.eval()
    with torch.no_grad():
        y_eval = new(graph, hd, hs)
    assert y_eval.shape == y0.shape and torch.equal(y_eval, new(graph, hd, hs).detach())
    assert torch.equal(y_eval.squeeze(-1), new.score_pairs(hd, hs, graph.edge_pairs().src.long(), graph.edge_pairs().dst.long()))


def test_flag_off_is_the_existing_path_bit_for_bit(dev):
    from dream_gnn_amd import model as M
    from dream_gnn_amd import ops

    graph, hd, hs = _decoder_inputs(dev)
    torch.manual_seed(2)
    dec = M.MLPDecoder(24, 0.2).to(dev).train()
    assert dec.fused_training is False
    torch.manual_seed(9)
    y = dec(graph, hd, hs)
    # the existing forward, statement for statement
    torch.manual_seed(9)
    w = dec.lin1.weight
    out = ops.gather_add_relu_dropout(graph.edge_pairs(), hd @ w[:, :24].t(), hs @ w[:, 24:].t(), dec.lin1.bias, dec.dropout.p)
    out = M._edge_linear_relu_dropout(dec.lin2, dec.dropout, out)
    assert torch.equal(y, M._edge_linear(dec.lin3, out))
    dec.fused_training = True   # and switching it on changes the stream, as documented
    torch.manual_seed(9)
    assert not torch.equal(dec(graph, hd, hs), y)


# ---------------------------------------------------------------------------------------------------------------------
# determinism
def test_gradients_are_the_same_bits_from_run_to_run(dev):
    d = K.float_design(40_000, seed=21)
    a, b = _run(d, dev, 0.3, _seed(dev)), _run(d, dev, 0.3, _seed(dev))
    for name in ("logit",) + K.GRADS:
        assert np.array_equal(a[name], b[name]), name
    c = _run(d, dev, 0.3, _seed(dev, SEED + 1))
    assert not np.array_equal(a["logit"], c["logit"])


# ---------------------------------------------------------------------------------------------------------------------
# memory
def _saved(fn, seen):
    if fn is None or fn in seen:
        return
    seen.add(fn)
    for name in dir(fn):
        if name.startswith("_saved_"):
            v = getattr(fn, name)
            for x in (v if isinstance(v, (tuple, list)) else (v,)):
                if isinstance(x, torch.Tensor):
                    yield x
    for x in getattr(fn, "saved_tensors", ()):
        yield x
    for nxt, _ in fn.next_functions:
        yield from _saved(nxt, seen)


def test_autograd_keeps_nothing_per_pair_and_the_peak_is_lower(dev):
    from dream_gnn_amd import _lib
    from dream_gnn_amd import model as M

    E = 40_000
    graph, hd, hs = _decoder_inputs(dev, E=E)
    torch.manual_seed(2)
    old = M.MLPDecoder(24, 0.1).to(dev).train()
    new = M.MLPDecoder(24, 0.1, fused_training=True).to(dev).train()
    dy = torch.randn(E, 1, device=dev)

    y = new(graph, hd.clone().requires_grad_(True), hs.clone().requires_grad_(True))
    sizes = [t.numel() for t in _saved(y.grad_fn, set())]
    assert sizes and max(sizes) < E * 64
    y_old = old(graph, hd.clone().requires_grad_(True), hs.clone().requires_grad_(True))
    assert max(t.numel() for t in _saved(y_old.grad_fn, set())) >= E * 64  # the walk sees what the torch chain keeps
    del y, y_old

    def peak(dec):
        a, b = hd.clone().requires_grad_(True), hs.clone().requires_grad_(True)
        dec(graph, a, b).backward(dy)  # builds the lazily made layouts and the kernel scratch
        dec.zero_grad(set_to_none=True)
        a.grad = b.grad = None
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        dec(graph, a, b).backward(dy)
        torch.cuda.synchronize()
        return torch.cuda.max_memory_allocated() - base

    # the fused backward's workspace lives in the kernel scratch across calls: count it in full
    fused = peak(new) + _lib.lib.dgmi_pair_mlp_train_workspace_bytes(E)
    chain = peak(old)
    print("peak bytes: fused %d (workspace included), torch chain %d" % (fused, chain))
    assert fused < chain


# ---------------------------------------------------------------------------------------------------------------------
# empty and bad input
def test_empty_list_and_bad_input(dev):
    from dream_gnn_amd import ops

    d = K.exact_design(33)
    t, _, _ = _dev(d, dev, grad=True)
    none = torch.zeros(0, dtype=torch.int64, device=dev)
    logit = ops.pair_mlp_train(*t, ops.EdgePairs(none, none, d["n_src"], d["n_dst"]), 0.5)
    assert logit.shape == (0,) and logit.dtype == torch.float32
    logit.sum().backward()
    for x in t:
        assert x.grad is not None and x.grad.shape == x.shape and not x.grad.any()
    with pytest.raises(RuntimeError, match="out of range"):
        ops.EdgePairs(torch.tensor([0, d["n_src"]], device=dev), torch.tensor([0, 0], device=dev), d["n_src"], d["n_dst"])
    t, pairs, _ = _dev(d, dev)
    with pytest.raises(RuntimeError, match="MI355X only"):
        ops.pair_mlp_train(t[0].cpu(), *t[1:], pairs, 0.5)
    with pytest.raises(ValueError, match="p must be"):
        ops.pair_mlp_train(*t, pairs, 1.0)
    with pytest.raises(ValueError, match="seed"):
        ops.pair_mlp_train(*t, pairs, 0.5, seed=torch.zeros(2, dtype=torch.int64, device=dev))
    with pytest.raises(RuntimeError, match="source feature table"):
        ops.pair_mlp_train(t[0][:5], *t[1:], pairs, 0.5)


# ---------------------------------------------------------------------------------------------------------------------
# HIP-graph capture
def test_captured_step_draws_a_new_mask_per_replay(dev):
    from dream_gnn_amd import ops

    d = K.float_design(3000, seed=31)
    t, pairs, g = _dev(d, dev, grad=True)

    def step():
        logit = ops.pair_mlp_train(*t, pairs, 0.3)  # seed=None: drawn on the device
        return (ops.pair_mlp_train.last_seed, logit) + torch.autograd.grad(logit, t, g)

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):  # the lazily built layouts and the kernel scratch exist before the recording
        step()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        outs = step()
    seeds = []
    for _ in range(2):
        graph.replay()
        torch.cuda.synchronize()
        got = [o.clone() for o in outs]
        seeds.append(int(got[0]))
        t2, _, _ = _dev(d, dev, grad=True)
        logit = ops.pair_mlp_train(*t2, pairs, 0.3, seed=got[0])
        want = (logit,) + torch.autograd.grad(logit, t2, g)
        for u, v in zip(got[1:], want):
            assert torch.equal(u, v.detach())
    assert seeds[0] != seeds[1]


def test_whole_model_trains_through_the_captured_step_with_the_flag_set(dev):
    """``net.decoder.fused_training = True`` and nothing else: ``harness.CapturedTrainStep`` records the iteration
    (augmentation, dropout 0.1) with the fused decoder in it, every replay draws new masks, and the model trains."""
    from dream_gnn_amd import harness as H, model as M
    from test_gpu_training import _problem

    batch, labels, args = _problem(dev)
    args.dropout, args.attention_dropout = 0.1, 0.1
    torch.manual_seed(1)
    net = M.Net(args).to(dev)
    net.decoder.fused_training = True
    opt = torch.optim.Adam(net.parameters(), lr=2e-3, weight_decay=1e-5, capturable=True)
    net.eval()
    with torch.no_grad():
        untrained = float(H.forward_loss(net, batch, labels, 0.1)[0])
    step = H.CapturedTrainStep(net, opt, batch, labels, beta=0.1)
    losses = [float(step()) for _ in range(40)]
    assert all(np.isfinite(losses)) and len(set(round(x, 7) for x in losses)) > 30
    assert np.mean(losses[-10:]) < 0.8 * untrained, (untrained, losses[-10:])
