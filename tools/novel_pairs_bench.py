"""Novel-pair ranking: the fused all-pairs decoder top-k against two baselines (one JSON line).

    python tools/novel_pairs_bench.py [--shapes lrssl,config4] [--k 200,1024] [--iters 5] [--check]

Shapes: lrssl (763 x 681, the dataset) and the config-4 node counts (100 000 x 50 000 = 5e9 pairs), known pairs
from ``synth``.  Timed with device events after a warm-up, medians over ``--iters``:
  kernel       ``ops.pair_mlp_topk`` on precomputed P / Q (the HIP kernels, workspace allocation and the count read)
  end_to_end   ``predict.top_novel_pairs`` on a ``Net`` (lrssl: the full model; config 4: ``MLPDecoder.top_pairs`` on
               random width-128 embeddings — the encoder at that size is a training-step benchmark of its own)
  baseline A   chunked torch with the same factorisation: broadcast add, relu, GEMM, relu, dot, ``topk`` per chunk, merge
  baseline B   (lrssl) the reference's flow on our ``Net``: 5 000-pair decoder graphs, a full eval forward per batch,
               sigmoid, host sort (train.py:26-151)
TFLOP/s counts 16 384 FLOP per pair (the two MLP GEMMs) over the kernel time, against the 155 TF f32-MFMA rate.
``--check`` runs the exhaustive fp64 comparison of tests/test_gpu_pairs.py at each chosen shape before timing.
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

PEAK_TF = 155.0
FLOP_PER_PAIR = 16384


def _time(fn, iters, warmup=1):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(iters):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b) / 1e3)
    return statistics.median(ts)


def _baseline_a(P, Q, dec, known_keys, k, rows):
    """Chunked torch, same factorisation: a (rows x n_dis x 128) hidden block per chunk, topk per chunk, merge."""
    W2, b2, w3, b3 = dec.lin2.weight, dec.lin2.bias, dec.lin3.weight.view(-1), dec.lin3.bias
    ns = Q.shape[0]
    vals, keys = [], []
    for a in range(0, P.shape[0], rows):
        b = min(P.shape[0], a + rows)
        h1 = torch.relu(P[a:b, None, :] + Q[None]).view(-1, 128)
        logit = torch.relu(torch.addmm(b2, h1, W2.t())) @ w3 + b3
        key = torch.arange(a * ns, b * ns, device=P.device)
        logit = logit.masked_fill(torch.isin(key, known_keys), float("-inf"))
        t = torch.topk(logit, min(k, logit.numel()))
        vals.append(t.values)
        keys.append(key[t.indices])
    t = torch.topk(torch.cat(vals), k)
    return torch.cat(keys)[t.indices], t.values


def _baseline_b(net, batch, known_np):
    """train.py:26-151 restated on our Net: 5 000-pair decoder graphs, a full eval forward per batch, sigmoid, host sort."""
    from dream_gnn_amd import graph as G

    nd, ns = known_np.shape
    novel = np.argwhere(known_np == 0)
    dev = batch["drug_feat"].device
    scores = []
    with torch.no_grad():
        for a in range(0, len(novel), 5000):
            part = novel[a:a + 5000]
            dec = G.build_dec_graph(torch.from_numpy(part[:, 0]), torch.from_numpy(part[:, 1]), nd, ns, device=dev).int()
            pred, *_ = net(batch["enc_graph"], dec, batch["drug_graph"], batch["drug_sim_feat"], batch["drug_feat"],
                           batch["disease_graph"], batch["disease_sim_feat"], batch["disease_feat"],
                           batch["drug_feature_graph"], batch["disease_feature_graph"])
            scores.append(torch.sigmoid(pred.squeeze(-1)).cpu().numpy())
    s = np.concatenate(scores)
    order = np.argsort(-s, kind="quicksort")
    return novel[order], s[order]


def _shape(name, dev):
    from dream_gnn_amd import model as M
    from dream_gnn_amd import synth

    if name == "lrssl":
        torch.manual_seed(0)
        batch, labels = synth.dataset_shaped_batch([(763, 681, 3051)], device=dev)
        net = M.Net(synth.net_args()).to(dev).eval()
        drug, dis, _ = batch["enc_pairs"]
        pos = labels.cpu() > 0
        known = (drug[pos].to(dev), dis[pos].to(dev))
        with torch.no_grad():
            hd, hs = net.embed(batch["enc_graph"], batch["drug_graph"], batch["drug_sim_feat"], batch["drug_feat"],
                               batch["disease_graph"], batch["disease_sim_feat"], batch["disease_feat"],
                               batch["drug_feature_graph"], batch["disease_feature_graph"])
        return dict(net=net, dec=net.decoder, batch=batch, known=known, hd=hd, hs=hs, nd=763, ns=681)
    if name != "config4":
        raise SystemExit("unknown shape %r (lrssl, config4)" % name)
    nd, ns = 100_000, 50_000
    torch.manual_seed(7)
    dec = M.MLPDecoder(128).to(dev).eval()
    g = torch.Generator(device=dev).manual_seed(8)
    hd, hs = torch.randn(nd, 128, device=dev, generator=g), torch.randn(ns, 128, device=dev, generator=g)
    known = synth.bipartite_edges(nd, ns, 10_000_000, 0, dev)
    return dict(net=None, dec=dec, batch=None, known=known, hd=hd, hs=hs, nd=nd, ns=ns)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="lrssl,config4")
    ap.add_argument("--k", default="200,1024")
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--check", action="store_true", help="exhaustive fp64 comparison at each shape first")
    args = ap.parse_args()

    from dream_gnn_amd import ops, predict

    dev = torch.device("cuda:0")
    ks_list = [int(x) for x in args.k.split(",")]
    rows = []
    for name in args.shapes.split(","):
        s = _shape(name, dev)
        dec, hd, hs, nd, ns = s["dec"], s["hd"], s["hs"], s["nd"], s["ns"]
        with torch.no_grad():
            F = hd.shape[1]
            w1 = dec.lin1.weight
            P, Q = torch.addmm(dec.lin1.bias, hd, w1[:, :F].t()), hs @ w1[:, F:].t()
        kd, ks = s["known"]
        known_keys = torch.sort(kd.long() * ns + ks.long()).values

        def kernel(k):
            return ops.pair_mlp_topk(P, Q, dec.lin2.weight, dec.lin2.bias, dec.lin3.weight, dec.lin3.bias, kd, ks, k)

        if args.check:
            sys.path.insert(0, os.path.join(ROOT, "tests"))
            import test_gpu_pairs as T

            mask = torch.zeros(nd, ns, dtype=torch.bool, device=dev)
            mask[kd.long(), ks.long()] = True
            L, Tl = T._all64(P, Q, dec)
            for k in ks_list:
                T._assert_topk(*kernel(k), L, Tl, mask, k)
                print("check ok: %s k=%d" % (name, k), flush=True)
            del L, Tl, mask
        for k in ks_list:
            kern = _time(lambda: kernel(k), args.iters)
            if s["net"] is not None:
                e2e = _time(lambda: predict.top_novel_pairs(s["net"], s["batch"], s["known"], k=k), args.iters)
            else:
                with torch.no_grad():
                    e2e = _time(lambda: dec.top_pairs(hd, hs, k, (kd, ks)), args.iters)
            chunk = max(1, (1 << 26) // ns)  # ~64 M pairs (a 32 GB fp32 hidden block) per chunk
            with torch.no_grad():
                base_a = _time(lambda: _baseline_a(P, Q, dec, known_keys, k, chunk), 1 if nd > 10_000 else args.iters,
                               warmup=0 if nd > 10_000 else 1)
            row = {"shape": name, "n_drug": nd, "n_dis": ns, "novel_pairs": nd * ns - int(known_keys.numel()), "k": k,
                   "kernel_s": kern, "top_novel_pairs_s": e2e, "baseline_a_s": base_a,
                   "tflops": nd * ns * FLOP_PER_PAIR / kern / 1e12}
            row["fraction_of_155tf"] = row["tflops"] / PEAK_TF
            row["speedup_kernel_vs_a"] = base_a / kern
            if s["net"] is not None:
                known_np = np.zeros((nd, ns), np.int8)
                known_np[kd.long().cpu().numpy(), ks.long().cpu().numpy()] = 1
                base_b = _time(lambda: _baseline_b(s["net"], s["batch"], known_np), 1)
                row["baseline_b_s"] = base_b
                row["speedup_top_novel_pairs_vs_b"] = base_b / e2e
            rows.append(row)
            print(json.dumps(row), flush=True)
        del s, P, Q
        torch.cuda.empty_cache()
    print(json.dumps({"novel_pairs_bench": rows}))


if __name__ == "__main__":
    main()
