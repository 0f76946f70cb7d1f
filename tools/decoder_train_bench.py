"""Decoder forward + backward on the training pair list, fused (``MLPDecoder.fused_training``: ``ops.pair_mlp_train``)
against the existing torch chain, in one process: an lrssl-shaped list (763 x 681, 467 643 pairs, 128-d embeddings) and a
C+G-shaped one (1256 x 722, 816 148 pairs, 256-d).  Both modules hold the same parameters and see the same inputs; the two
paths alternate, three rounds of ``--iters`` iterations each, timed with HIP events around the whole round (forward,
backward of every parameter and of both embedding tables).  Also the peak allocated bytes of one iteration of each path
(the fused path's persistent kernel scratch counted in full).

    python tools/decoder_train_bench.py [--iters 30] [--out profiles/decoder_train/decoder_train_bench.json]
    rocprofv3 --kernel-trace --stats -d DIR -- python tools/decoder_train_bench.py --pieces

Prints one JSON document; needs the MI355X (no fallback).  ``--pieces``: instead, the ops of the fused step one by one
on the lrssl-shaped list (list scorer, training forward and backward at p = 0 and 0.1, the two segment sums), 23 calls
each with HIP events around the last 20: a run to put under a kernel trace."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import __graft_entry__  # noqa: E402

__graft_entry__.ensure_built()  # before the GPU is touched

import torch  # noqa: E402

from dream_gnn_amd import _lib, model as M, ops  # noqa: E402

SHAPES = (("lrssl-shape", 763, 681, 128), ("C+G-shape", 1256, 722, 256))
ROUNDS = 3


class _Graph:
    def __init__(self, pairs):
        self._pairs = pairs

    def edge_pairs(self):
        return self._pairs


def problem(nd, ns, F, dev):
    g = torch.Generator().manual_seed(nd * 1000 + ns)
    cells = torch.randperm(nd * ns, generator=g)[: round(nd * ns * 0.9)]  # 90 % of all cells train, as a fold does
    src, dst = (cells // ns).to(dev), (cells % ns).to(dev)
    pairs = ops.EdgePairs(src, dst, nd, ns)
    hd, hs = torch.randn(nd, F, generator=g).to(dev), torch.randn(ns, F, generator=g).to(dev)
    dy = torch.randn(pairs.E, 1, generator=g).to(dev)
    return _Graph(pairs), hd, hs, dy


def pieces(dev):
    T = _lib.torch_ops
    _, nd, ns, _ = SHAPES[0]
    graph, _, _, dy = problem(nd, ns, 128, dev)
    pairs = graph.edge_pairs()
    g = torch.Generator().manual_seed(1)
    r = lambda *s: torch.randn(*s, generator=g).to(dev)  # noqa: E731
    P, Q, W2, b2, w3, b3 = r(nd, 128), r(ns, 128), r(64, 128) / 8, r(64), r(64), r(1)
    seed = torch.tensor([5], dtype=torch.int64, device=dev)
    dl, dz1 = dy.reshape(-1).contiguous(), r(pairs.E, 128)
    ids = (pairs.src, pairs.dst)

    def timed(name, fn):
        for _ in range(3):
            fn()
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        for _ in range(20):
            fn()
        t1.record()
        t1.synchronize()
        print("%-28s %.4f ms" % (name, t0.elapsed_time(t1) / 20), flush=True)

    timed("score_list", lambda: T.pair_mlp_score_list(P, Q, W2, b2, w3, b3, *ids))
    for p in (0.0, 0.1):
        timed("train_forward p=%g" % p, lambda: T.pair_mlp_train_forward(P, Q, W2, b2, w3, b3, *ids, p, seed))
        timed("train_backward p=%g" % p, lambda: T.pair_mlp_train_backward(P, Q, W2, b2, w3, b3, *ids, p, seed, dl))
    timed("by_src spmm", lambda: pairs.by_src().spmm(dz1))
    timed("by_dst spmm", lambda: pairs.by_dst().spmm(dz1))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--out", default=None)
    ap.add_argument("--pieces", action="store_true")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("decoder_train_bench needs the MI355X: nothing is measured without it")
    dev = torch.device("cuda:0")
    if a.pieces:
        return pieces(dev)
    doc = {"device": torch.cuda.get_device_name(0), "iters_per_round": a.iters, "rounds": ROUNDS, "dropout": 0.1, "shapes": {}}
    for tag, nd, ns, F in SHAPES:
        graph, hd, hs, dy = problem(nd, ns, F, dev)
        E = graph.edge_pairs().E
        torch.manual_seed(0)
        chain = M.MLPDecoder(F, 0.1).to(dev).train()
        fused = M.MLPDecoder(F, 0.1, fused_training=True).to(dev).train()
        fused.load_state_dict(chain.state_dict())
        hd.requires_grad_(True), hs.requires_grad_(True)

        def step(dec):
            dec.zero_grad(set_to_none=True)
            hd.grad = hs.grad = None
            dec(graph, hd, hs).backward(dy)

        def timed(dec):
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record()
            for _ in range(a.iters):
                step(dec)
            t1.record()
            t1.synchronize()
            return t0.elapsed_time(t1) / a.iters

        def peak(dec):
            step(dec)
            dec.zero_grad(set_to_none=True)
            hd.grad = hs.grad = None
            torch.cuda.synchronize()
            torch.cuda.reset_peak_memory_stats()
            base = torch.cuda.memory_allocated()
            step(dec)
            torch.cuda.synchronize()
            return torch.cuda.max_memory_allocated() - base

        for dec in (chain, fused):  # every shape's first launches, layouts and scratch
            for _ in range(5):
                step(dec)
        torch.cuda.synchronize()
        ms = {"chain": [], "fused": []}
        for _ in range(ROUNDS):
            ms["chain"].append(timed(chain))
            ms["fused"].append(timed(fused))
        spread = max(max(v) - min(v) for v in ms.values())
        gain = min(ms["chain"]) - max(ms["fused"])  # the least the fused path saves over the three rounds
        doc["shapes"][tag] = {
            "n_drug": nd, "n_disease": ns, "embedding": F, "pairs": E,
            "chain_ms": [round(x, 4) for x in ms["chain"]], "fused_ms": [round(x, 4) for x in ms["fused"]],
            "widest_spread_ms": round(spread, 4), "least_gain_ms": round(gain, 4),
            "fused_wins_beyond_spread": bool(gain > spread),
            "peak_bytes_chain": peak(chain),
            "peak_bytes_fused": peak(fused) + int(_lib.lib.dgmi_pair_mlp_train_workspace_bytes(E)),
        }
        print(tag, json.dumps(doc["shapes"][tag]), flush=True)
    text = json.dumps(doc, indent=1)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
