"""Attention fusion forward + backward of BOTH node types, fused (``Attention.fused``: ``ops.attention_fuse``) against the
torch chain, in one process, eager, timed with HIP events: an lrssl shape (763 + 681 rows, F = 128), a C+G shape
(1256 + 722 rows, F = 256) and a config-4 scale (100 000 + 50 000 rows, F = 128), dropout 0.1.  Both modules hold the same
parameters and see the same inputs; the two paths alternate, three rounds of ``--iters`` iterations each after a warm-up.
Also the peak allocated bytes of one iteration of each path (the fused path's persistent kernel scratch counted in full),
and an lrssl-shaped ``harness.CapturedTrainStep`` with the flag off and on, replayed alternately (three rounds of
``--replays`` replays).

    python tools/attention_fuse_bench.py [--iters 30] [--replays 200] [--out profiles/attention_fuse/attention_fuse_bench.json]
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/attention_fuse_bench.py --pieces

Prints one JSON document; needs the MI355X (no fallback).  ``--pieces``: instead, the two ops alone at every shape, 23
calls each with HIP events around the last 20: a run to put under a kernel trace."""
import argparse
import json
import os
import sys
import types

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import __graft_entry__  # noqa: E402

__graft_entry__.ensure_built()  # before the GPU is touched

import torch  # noqa: E402

from dream_gnn_amd import _lib, graph as G, harness as H, model as M, synth  # noqa: E402

SHAPES = (("lrssl-shape", 763, 681, 128), ("C+G-shape", 1256, 722, 256), ("config-4 scale", 100_000, 50_000, 128))
ROUNDS = 3
DROPOUT = 0.1


def tables(nd, ns, F, dev):
    g = torch.Generator().manual_seed(nd * 1000 + ns)
    r = lambda n: torch.randn(n, F, generator=g).to(dev)  # noqa: E731
    return [r(nd), 0.5 * r(nd), r(ns), 0.5 * r(ns)], [r(nd), r(ns)]


def pieces(dev):
    T = _lib.torch_ops
    for tag, nd, ns, F in SHAPES:
        g = torch.Generator().manual_seed(1)
        r = lambda *s: torch.randn(*s, generator=g).to(dev)  # noqa: E731
        for n in (nd, ns):
            A, B, W1, b1, w2, dout = r(n, F), r(n, F), r(16, F) / F ** 0.5, r(16) / 4, r(16) / 4, r(n, F)
            mult = torch.nn.functional.dropout(torch.ones(n, 2, device=dev), DROPOUT, True)
            for name, fn in (("forward", lambda: T.attn_fuse_forward(A, B, mult, W1, b1, w2)),
                             ("backward", lambda: T.attn_fuse_backward(A, B, mult, W1, b1, w2, dout))):
                for _ in range(3):
                    fn()
                t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                t0.record()
                for _ in range(20):
                    fn()
                t1.record()
                t1.synchronize()
                print("%-16s n=%-7d F=%-4d %-9s %.4f ms" % (tag, n, F, name, t0.elapsed_time(t1) / 20), flush=True)


def summary(ms, a, b):
    spread = max(max(v) - min(v) for v in ms.values())
    gain = min(ms[a]) - max(ms[b])  # the least the fused path saves over the three rounds
    return {a + "_ms": [round(x, 4) for x in ms[a]], b + "_ms": [round(x, 4) for x in ms[b]],
            "widest_spread_ms": round(spread, 4), "least_gain_ms": round(gain, 4), "fused_wins_beyond_spread": bool(gain > spread)}


def modules(dev, iters):
    out = {}
    for tag, nd, ns, F in SHAPES:
        z, dy = tables(nd, ns, F, dev)
        torch.manual_seed(0)
        chain = M.Attention(F, dropout_rate=DROPOUT).to(dev).train()
        fused = M.Attention(F, dropout_rate=DROPOUT, fused=True).to(dev).train()
        fused.load_state_dict(chain.state_dict())
        for t in z:
            t.requires_grad_(True)

        def step(att):
            att.zero_grad(set_to_none=True)
            for t in z:
                t.grad = None
            drug, _ = att.fuse(z[0], z[1])
            dis, _ = att.fuse(z[2], z[3])
            torch.autograd.backward([drug, dis], dy)

        def timed(att):
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record()
            for _ in range(iters):
                step(att)
            t1.record()
            t1.synchronize()
            return t0.elapsed_time(t1) / iters

        def peak(att):
            step(att)
            att.zero_grad(set_to_none=True)
            for t in z:
                t.grad = None
            torch.cuda.synchronize()
            torch.cuda.reset_peak_memory_stats()
            base = torch.cuda.memory_allocated()
            step(att)
            torch.cuda.synchronize()
            return torch.cuda.max_memory_allocated() - base

        for att in (chain, fused):
            for _ in range(5):
                step(att)
        torch.cuda.synchronize()
        ms = {"chain": [], "fused": []}
        for _ in range(ROUNDS):
            ms["chain"].append(timed(chain))
            ms["fused"].append(timed(fused))
        entry = {"rows": [nd, ns], "width": F}
        entry.update(summary(ms, "chain", "fused"))
        entry["peak_bytes_chain"] = peak(chain)
        entry["peak_bytes_fused"] = peak(fused) + int(_lib.lib.dgmi_attn_fuse_workspace_bytes(max(nd, ns), F))
        out[tag] = entry
        print(tag, json.dumps(entry), flush=True)
        del z, dy
        torch.cuda.empty_cache()
    return out


def recorded_step(dev, replays):
    """An lrssl-shaped training iteration as bench.py builds it, recorded with the flag off and on."""
    drug, dis, labels, nd, ns = synth.dataset_shaped_pairs([synth.DATASET_SHAPES["lrssl"]])
    batch = {"enc_graph": G.build_enc_graph(drug, dis, labels, nd, ns, device=dev).int(),
             "dec_graph": G.build_dec_graph(drug, dis, nd, ns, device=dev).int()}
    for key, n, seed in (("drug", nd, 1), ("disease", ns, 2)):
        batch[key + "_sim_feat"] = torch.rand(n, n, device=dev)
        batch[key + "_feat"] = torch.nn.functional.normalize(torch.randn(n, 768, device=dev))
        for gname, s2 in ((key + "_graph", 0), (key + "_feature_graph", 10)):
            r, c, v = synth.knn_sim_graph(n, 4, seed + s2, dev)
            batch[gname] = torch.sparse_coo_tensor(torch.stack([r.long(), c.long()]), v, (n, n))
    args = types.SimpleNamespace(rating_vals=[0, 1], src_in_units=768, dst_in_units=768, gcn_agg_units=1024, gcn_out_units=128,
                                 dropout=0.3, gcn_agg_accum="sum", model_activation="leaky", share_param=True, device=None,
                                 layers=3, fdim_drug=nd, fdim_disease=ns, nhid1=768, nhid2=128, attention_dropout=0.5)
    y = labels.to(dev).float()
    steps = {}
    for name, flag in (("chain", False), ("fused", True)):
        torch.manual_seed(0)
        net = M.Net(args).to(dev)
        net.attention.fused = flag
        opt = torch.optim.Adam(net.parameters(), lr=2e-3, weight_decay=1e-5, capturable=True)
        steps[name] = H.CapturedTrainStep(net, opt, batch, y)

    def timed(step):
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        for _ in range(replays):
            step()
        t1.record()
        t1.synchronize()
        return t0.elapsed_time(t1) / replays

    for step in steps.values():
        for _ in range(20):
            step()
    torch.cuda.synchronize()
    ms = {"chain": [], "fused": []}
    for _ in range(ROUNDS):
        ms["chain"].append(timed(steps["chain"]))
        ms["fused"].append(timed(steps["fused"]))
    entry = {"nodes": "%dx%d" % (nd, ns), "train_pairs": int(drug.numel()), "replays_per_round": replays}
    entry.update(summary(ms, "chain", "fused"))
    print("recorded step", json.dumps(entry), flush=True)
    return entry


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--replays", type=int, default=200)
    ap.add_argument("--out", default=None)
    ap.add_argument("--pieces", action="store_true")
    ap.add_argument("--no-step", action="store_true", help="skip the recorded training step")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("attention_fuse_bench needs the MI355X: nothing is measured without it")
    dev = torch.device("cuda:0")
    if a.pieces:
        return pieces(dev)
    doc = {"device": torch.cuda.get_device_name(0), "iters_per_round": a.iters, "rounds": ROUNDS, "dropout": DROPOUT,
           "shapes": modules(dev, a.iters)}
    if not a.no_step:
        doc["recorded_lrssl_step"] = recorded_step(dev, a.replays)
    text = json.dumps(doc, indent=1)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
