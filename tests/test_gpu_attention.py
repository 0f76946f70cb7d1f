"""The fused attention fusion on the GPU (``ops.attention_fuse``, ``model.Attention.fused``): exact designs
EQUAL the float64 restatement at every block and width edge and in every operand form; float designs meet the accuracy
bars against float64 and against the torch chain; the module and ``Net`` routes draw the chain's masks; sums are
deterministic; non-finite rows stay in their row; autograd keeps the inputs only; both routes can be captured.

Measured on one MI355X (float designs, ``max|T_fused - T_64| / (4 max|T_chain - T_64| + 2^-22 max|T_64|)``; the bound
is 1): between 0.038 and 0.226 over the seven outputs and the three shapes, the largest on ``out`` at (1256, 256); ``out``
elementwise at 0.012 - 0.014 of its bar.  The file prints every ratio (``-s``); the table is in DESIGN.md 4.16."""
import functools

import numpy as np
import pytest
import torch

import _attention_cases as K

pytestmark = pytest.mark.gpu

NAMES = ("A", "B", "W1", "b1", "w2")


def _RG():
    from dream_gnn_amd import ops

    return ops.ATTN_FUSE_BLOCK_ROWS, ops.ATTN_FUSE_MAX_WORKGROUPS


@functools.lru_cache(maxsize=4)
def _exact(n_rows, F, mult):
    d = K.exact_design(n_rows, F, mult)
    r = K.reference(d["A"], d["B"], d["W1"], d["b1"], d["w2"], d["M"], d["g"])
    return d, {k: v.astype(np.float32) for k, v in r.items()}


@functools.lru_cache(maxsize=4)
def _float(n_rows, F, seed):
    d = K.float_design(n_rows, F, seed)
    return d, K.reference(d["A"], d["B"], d["W1"], d["b1"], d["w2"], d["M"], d["g"])


def _run(d, dev, layout="contiguous", mult=True):
    """All seven outputs of ``ops.attention_fuse`` on design ``d`` (numpy), the tables placed by ``layout``:
    contiguous, stacked (views of one (n, 2, F) leaf), stacked_direct (``b=None``), padded (ld = F + 4)."""
    from dream_gnn_amd import ops

    t = {k: torch.from_numpy(d[k]).to(dev) for k in NAMES + ("g",)}
    M = torch.from_numpy(d["M"]).to(dev) if (mult and d["M"] is not None) else None
    n, F = d["A"].shape
    params = [t[k].clone().requires_grad_(True) for k in ("W1", "b1", "w2")]
    if layout.startswith("stacked"):
        z = torch.stack([t["A"], t["B"]], 1).requires_grad_(True)
        leaves = [z]
        a, b = (z, None) if layout == "stacked_direct" else (z[:, 0], z[:, 1])
    elif layout == "padded":
        bufs = [torch.zeros(n, F + 4, device=dev) for _ in range(2)]
        bufs[0][:, :F], bufs[1][:, :F] = t["A"], t["B"]
        leaves = [x.requires_grad_(True) for x in bufs]
        a, b = leaves[0][:, :F], leaves[1][:, :F]
    else:
        leaves = [t["A"].clone().requires_grad_(True), t["B"].clone().requires_grad_(True)]
        a, b = leaves
    out, beta = ops.attention_fuse(a, b, *params, M)
    assert not beta.requires_grad and out.shape == (n, F) and beta.shape == (n, 2)
    grads = torch.autograd.grad(out, leaves + params, t["g"])
    if layout.startswith("stacked"):
        dA, dB = grads[0][:, 0], grads[0][:, 1]
        rest = grads[1:]
    elif layout == "padded":
        assert not grads[0][:, F:].any() and not grads[1][:, F:].any()
        dA, dB = grads[0][:, :F], grads[1][:, :F]
        rest = grads[2:]
    else:
        dA, dB = grads[0], grads[1]
        rest = grads[2:]
    got = dict(zip(K.OUTPUTS, (out.detach(), beta, dA, dB) + tuple(rest)))
    return {k: v.cpu().numpy().reshape(-1) if k in ("db1", "dw2") else v.cpu().numpy() for k, v in got.items()}


LAYOUTS = ("contiguous", "stacked", "stacked_direct", "padded")


def _exact_case(dev, n_rows, F, mult):
    d, want = _exact(n_rows, F, mult)
    for layout in LAYOUTS:
        got = _run(d, dev, layout)
        for k in K.OUTPUTS:
            assert np.array_equal(got[k], want[k]), (layout, k, np.abs(got[k] - want[k]).max())


# ---------------------------------------------------------------------------------------------------------------------
# 1. exact designs
@pytest.mark.parametrize("mult", [False, True])
@pytest.mark.parametrize("which", range(8))
def test_exact_designs_equal_the_restatement_at_every_block_edge(dev, which, mult):
    R, G = _RG()
    n_rows = [1, 2, R - 1, R, R + 1, 2 * R + 3, R * G + 1, 2 * R * G + R + 5][which]
    _exact_case(dev, n_rows, 128, mult)


@pytest.mark.parametrize("mult", [False, True])
@pytest.mark.parametrize("F", [4, 8, 16, 64, 132, 256, 512])
def test_exact_designs_equal_the_restatement_at_every_width(dev, F, mult):
    _exact_case(dev, _RG()[0] + 1, F, mult)


# ---------------------------------------------------------------------------------------------------------------------
# 2. float designs
class _Mult(torch.nn.Module):
    """Stands where ``nn.Dropout`` stands in ``model.Attention``: the given multiplier on beta (n, 2, 1)."""

    def __init__(self, M):
        super().__init__()
        self.M = M

    def forward(self, beta):
        return beta * self.M.unsqueeze(-1)


def _chain(d, dev):
    """``model.Attention`` with the flag off on design ``d`` (the parent's code), the dropout replaced by ``d['M']``."""
    from dream_gnn_amd import model as M

    n, F = d["A"].shape
    att = M.Attention(F).to(dev)
    with torch.no_grad():
        att.project[0].weight.copy_(torch.from_numpy(d["W1"]))
        att.project[0].bias.copy_(torch.from_numpy(d["b1"]))
        att.project[2].weight.copy_(torch.from_numpy(d["w2"]).view(1, 16))
    att.dropout = _Mult(torch.from_numpy(d["M"]).to(dev))
    a, b = (torch.from_numpy(d[k]).to(dev).requires_grad_(True) for k in ("A", "B"))
    out, beta = att(torch.stack([a, b], 1))
    p = [att.project[0].weight, att.project[0].bias, att.project[2].weight]
    grads = torch.autograd.grad(out, [a, b] + p, torch.from_numpy(d["g"]).to(dev))
    got = dict(zip(K.OUTPUTS, (out.detach(), beta.detach().view(n, 2)) + tuple(grads)))
    return {k: v.cpu().numpy().reshape(-1) if k in ("db1", "dw2") else v.cpu().numpy() for k, v in got.items()}


@pytest.mark.parametrize("which", range(3))
def test_float_designs_meet_the_accuracy_bars(dev, which):
    R, G = _RG()
    n_rows, F = [(763, 128), (1256, 256), (R * G + R + 1, 128)][which]
    d, want = _float(n_rows, F, 40 + which)
    fused, chain = _run(d, dev), _chain(d, dev)
    # out, elementwise: the bar of DESIGN 3 on the sum's absolute terms; exactly 0 where both factors are 0
    bar = 1e-5 * (d["M"][:, 0, None] * np.abs(d["A"]) + d["M"][:, 1, None] * np.abs(d["B"])).astype(np.float64)
    err = np.abs(fused["out"] - want["out"])
    print("attention_fuse (%d, %d): out err / bar max %.4f" % (n_rows, F, (err[bar > 0] / bar[bar > 0]).max()))
    assert np.all(err <= bar)
    assert not fused["out"][(d["M"] == 0).all(1)].any()
    for k in K.OUTPUTS:
        e_f, e_c = np.abs(fused[k] - want[k]).max(), np.abs(chain[k] - want[k]).max()
        bound = 4 * e_c + 2.0 ** -22 * np.abs(want[k]).max()
        print("attention_fuse (%d, %d) %-4s fused %.3e chain %.3e ratio to bound %.3f" % (n_rows, F, k, e_f, e_c, e_f / bound))
        assert e_f <= bound, k


# ---------------------------------------------------------------------------------------------------------------------
# 3. module route
def _module_run(att, x, y, g, route, seed):
    a, b = x.clone().requires_grad_(True), y.clone().requires_grad_(True)
    att.zero_grad()
    before = torch.cuda.get_rng_state()
    if seed is not None:
        torch.manual_seed(seed)
        before = torch.cuda.get_rng_state()
    out, beta = att(torch.stack([a, b], 1)) if route == "forward" else att.fuse(a, b)
    out.backward(g)
    grads = [a.grad, b.grad] + [p.grad.clone() for p in att.parameters()]
    return out.detach(), beta.detach(), grads, before, torch.cuda.get_rng_state()


def _within_module_bar(got, want):
    out, beta, grads = got[:3]
    assert (out - want[0]).abs().max() <= 1e-5 * want[0].abs().max()
    assert beta.shape == want[1].shape and torch.equal(beta == 0, want[1] == 0)
    assert (beta - want[1]).abs().max() <= 1e-5 * want[1].abs().max()
    for u, v in zip(grads, want[2]):
        assert u.shape == v.shape and (u - v).abs().max() <= 1e-4 * v.abs().max()


@pytest.mark.parametrize("p", [0.1, 0.5])
def test_module_route_draws_the_chains_masks_in_training(dev, p):
    from dream_gnn_amd import model as M

    torch.manual_seed(3)
    att = M.Attention(64, dropout_rate=p).to(dev).train()
    x, y, g = torch.randn(301, 64, device=dev), 0.5 * torch.randn(301, 64, device=dev), torch.randn(301, 64, device=dev)
    att.fused = False
    want = _module_run(att, x, y, g, "forward", 11)
    assert (want[1] == 0).any() and not torch.equal(want[3], want[4])
    att.fused = True
    runs = [_module_run(att, x, y, g, route, 11) for route in ("forward", "fuse")]
    for got in runs:
        assert got[1].shape == (301, 2, 1) and not got[1].requires_grad
        assert torch.equal(got[4], want[4])                      # the generator is left where the chain leaves it
        _within_module_bar(got, want)
    for u, v in zip([runs[0][0], runs[0][1]] + runs[0][2], [runs[1][0], runs[1][1]] + runs[1][2]):
        assert torch.equal(u, v)                                 # forward(stacked z) and fuse(a, b): the same bits


def test_module_route_in_eval_mode_consumes_no_rng(dev):
    from dream_gnn_amd import model as M

    torch.manual_seed(3)
    att = M.Attention(64, dropout_rate=0.5).to(dev).eval()
    x, y, g = torch.randn(301, 64, device=dev), 0.5 * torch.randn(301, 64, device=dev), torch.randn(301, 64, device=dev)
    att.fused = False
    want = _module_run(att, x, y, g, "forward", None)
    att.fused = True
    for route in ("forward", "fuse"):
        got = _module_run(att, x, y, g, route, None)
        assert torch.equal(got[3], got[4])
        _within_module_bar(got, want)
    att.train()
    att.dropout.p = 0.0                                           # training without dropout: no multiplier, no draw
    got = _module_run(att, x, y, g, "fuse", None)
    assert torch.equal(got[3], got[4])
    _within_module_bar(got, want)


# ---------------------------------------------------------------------------------------------------------------------
# 4. Net route
def test_net_route_matches_the_chain_from_the_same_seed(dev):
    from dream_gnn_amd import model as M
    from test_gpu_training import _problem

    batch, labels, args = _problem(dev)
    args.dropout, args.attention_dropout = 0.1, 0.1
    torch.manual_seed(1)
    net = M.Net(args).to(dev).train()
    w = torch.randn(labels.numel(), device=dev)
    runs = []
    for fused in (False, True):
        net.attention.fused = fused
        net.zero_grad()
        torch.manual_seed(17)
        pred = net(batch["enc_graph"], batch["dec_graph"], batch["drug_graph"], batch["drug_sim_feat"], batch["drug_feat"],
                   batch["disease_graph"], batch["disease_sim_feat"], batch["disease_feat"],
                   batch.get("drug_feature_graph"), batch.get("disease_feature_graph"), False)[0]
        (pred.view(-1) * w).sum().backward()
        runs.append((pred.detach(), {k: p.grad.clone() for k, p in net.named_parameters() if p.grad is not None},
                     torch.cuda.get_rng_state()))
    (pred0, grads0, state0), (pred1, grads1, state1) = runs
    assert torch.equal(state0, state1) and sorted(grads0) == sorted(grads1) and "attention.project.0.weight" in grads1
    assert (pred1 - pred0).abs().max() <= 1e-5 * pred0.abs().max()
    for k in grads0:
        assert (grads1[k] - grads0[k]).abs().max() <= 1e-4 * grads0[k].abs().max(), k


# ---------------------------------------------------------------------------------------------------------------------
# 5. determinism, 6. non-finite operands
def test_two_runs_give_the_same_bits(dev):
    R, G = _RG()
    d, _ = _float(R * G + R + 1, 128, 42)
    first, second = _run(d, dev), _run(d, dev)
    for k in K.OUTPUTS:
        assert np.array_equal(first[k], second[k]), k


@pytest.mark.parametrize("mult", [False, True])
def test_a_nan_row_stays_in_its_row(dev, mult):
    d = dict(K.float_design(200, 128, 5))
    d["A"] = d["A"].copy()
    d["A"][77, 5] = np.nan
    if mult:
        d["M"] = d["M"].copy()
        d["M"][77] = 0.0                                         # a product: NaN * 0 = NaN
    got = _run(d, dev, mult=mult)
    other = np.arange(200) != 77
    for k in ("out", "beta", "dA", "dB"):
        assert np.isfinite(got[k][other]).all(), k
        assert np.isnan(got[k][77]).all(), k
    for k in ("dW1", "db1", "dw2"):
        assert np.isnan(got[k]).all(), k


# ---------------------------------------------------------------------------------------------------------------------
# 7. empty and bad input
def test_empty_tables(dev):
    d = K.float_design(0, 128, 1)
    for layout in ("contiguous", "stacked_direct"):
        got = _run(d, dev, layout, mult=False)
        assert got["out"].shape == (0, 128) and got["beta"].shape == (0, 2) and got["dA"].shape == (0, 128)
        assert got["dW1"].shape == (16, 128) and not got["dW1"].any() and not got["db1"].any() and not got["dw2"].any()
        assert got["db1"].shape == (16,) and got["dw2"].shape == (16,)


def test_bad_input_is_refused(dev):
    from dream_gnn_amd import ops

    z = lambda *s: torch.zeros(*s, device=dev)
    with pytest.raises(RuntimeError, match="MI355X only"):
        ops.attention_fuse(torch.zeros(3, 8), torch.zeros(3, 8), torch.zeros(16, 8), torch.zeros(16), torch.zeros(16))
    with pytest.raises(RuntimeError, match="MI355X only"):
        ops.attention_fuse(z(3, 8), z(3, 8), z(16, 8), z(16), z(16), torch.zeros(3, 2))
    for F in (6, 516):
        with pytest.raises(ValueError):
            ops.attention_fuse(z(3, F), z(3, F), z(16, F), z(16), z(16))
    with pytest.raises(ValueError):
        ops.attention_fuse(z(3, 8), z(3, 8), z(8, 8), z(8), z(8))              # hidden size 8
    with pytest.raises(ValueError):
        ops.attention_fuse(z(3, 8), z(4, 8), z(16, 8), z(16), z(16))
    with pytest.raises(ValueError):
        ops.attention_fuse(z(3, 8), z(3, 8), z(16, 8), z(16), z(16), z(3, 3))
    with pytest.raises(ValueError):
        ops.attention_fuse(z(3, 8).double(), z(3, 8).double(), z(16, 8), z(16), z(16))


# ---------------------------------------------------------------------------------------------------------------------
# 8. autograd keeps the inputs only
def test_autograd_saves_only_the_ops_inputs(dev):
    from dream_gnn_amd import ops

    d = K.float_design(1000, 128, 9)
    t = [torch.from_numpy(d[k]).to(dev).requires_grad_(True) for k in NAMES]
    M = torch.from_numpy(d["M"]).to(dev)
    saved = {}

    def pack(x):
        saved[x.untyped_storage().data_ptr()] = x.untyped_storage().nbytes()
        return x

    with torch.autograd.graph.saved_tensors_hooks(pack, lambda x: x):
        out, _ = ops.attention_fuse(*t, M)
    inputs = {x.untyped_storage().data_ptr(): x.untyped_storage().nbytes() for x in t + [M]}
    assert saved and set(saved) <= set(inputs)
    assert sum(saved.values()) <= sum(inputs.values())
    out.backward(torch.from_numpy(d["g"]).to(dev))
    assert all(x.grad is not None for x in t)


# ---------------------------------------------------------------------------------------------------------------------
# 9. HIP-graph capture
def test_captured_call_replays_to_the_bits_of_an_eager_call(dev):
    from dream_gnn_amd import ops

    d = K.float_design(1500, 128, 21)
    t = [torch.from_numpy(d[k]).to(dev).requires_grad_(True) for k in NAMES]
    M, g = torch.from_numpy(d["M"]).to(dev), torch.from_numpy(d["g"]).to(dev)

    def step():
        out, beta = ops.attention_fuse(*t, M)
        return (out, beta) + torch.autograd.grad(out, t, g)

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):  # the kernel scratch exists before the recording
        step()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        outs = step()
    want = [o.detach().clone() for o in step()]
    for _ in range(2):
        graph.replay()
        torch.cuda.synchronize()
        for u, v in zip(outs, want):
            assert torch.equal(u.detach(), v)
    with torch.no_grad():                                        # refreshed operands: the replay follows them
        t[0].mul_(0.5)
    graph.replay()
    torch.cuda.synchronize()
    for u, v in zip(outs, step()):
        assert torch.equal(u.detach(), v.detach())


def test_whole_model_trains_through_the_captured_step_with_the_flag_set(dev):
    """``net.attention.fused = True`` and nothing else: ``harness.CapturedTrainStep`` records the iteration (augmentation,
    dropout 0.1 on the attention weights) with the fused attention in it, and the model trains."""
    from dream_gnn_amd import harness as H, model as M
    from test_gpu_training import _problem

    batch, labels, args = _problem(dev)
    args.dropout, args.attention_dropout = 0.1, 0.1
    torch.manual_seed(1)
    net = M.Net(args).to(dev)
    net.attention.fused = True
    opt = torch.optim.Adam(net.parameters(), lr=2e-3, weight_decay=1e-5, capturable=True)
    net.eval()
    with torch.no_grad():
        untrained = float(H.forward_loss(net, batch, labels, 0.1)[0])
    step = H.CapturedTrainStep(net, opt, batch, labels, beta=0.1)
    losses = [float(step()) for _ in range(40)]
    assert all(np.isfinite(losses)) and len(set(round(x, 7) for x in losses)) > 30
    assert np.mean(losses[-10:]) < 0.8 * untrained, (untrained, losses[-10:])
