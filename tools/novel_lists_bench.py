"""Per-row novel lists: the fused per-row decoder top-k against chunked torch (one JSON line).

    python tools/novel_lists_bench.py [--cases config4,single,lrssl] [--k 50,128] [--iters 5] [--no-baseline]

Cases (known pairs from ``synth``), timed with device events after a warm-up, medians over ``--iters``:
  config4   100 000 drugs x 50 000 diseases (5e9 pairs), per-disease and per-drug lists for each ``--k``:
            kernel      ``ops.pair_mlp_row_topk`` on precomputed P / Q (the HIP kernels, workspace allocation, the flag
                        read)
            baseline A  chunked torch with the same factorisation: broadcast add, relu, GEMM, relu, dot over a block of
                        query rows x every candidate, known pairs masked, ``topk`` per row (per-disease, first k only)
  single    one disease against 100 000 drugs (``rows=[0]`` of the config-4 problem), per-disease lists
  lrssl     763 x 681 (the dataset), every disease, k = 10: ``predict.top_novel_per_disease`` end to end on a ``Net``
            (encoder included) and the kernel alone
TFLOP/s counts 16 384 FLOP per pair (the two MLP GEMMs) over the kernel time, against the 155 TF f32-MFMA rate.
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

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


def _baseline_a(X, C, dec, kq, kc, k, rows):
    """Chunked torch, same factorisation: a (rows x n_cand x 128) hidden block per chunk of query rows, the known pairs
    of the chunk masked, ``topk`` per row."""
    W2, b2, w3, b3 = dec.lin2.weight, dec.lin2.bias, dec.lin3.weight.view(-1), dec.lin3.bias
    nq, nc = X.shape[0], C.shape[0]
    order = torch.argsort(kq)
    kq_s, kc_s = kq[order], kc[order]
    bounds = torch.searchsorted(kq_s, torch.arange(0, nq + rows, rows, device=X.device).clamp(max=nq)).tolist()
    cand = torch.empty(nq, k, dtype=torch.long, device=X.device)
    logit = torch.empty(nq, k, device=X.device)
    for n, a in enumerate(range(0, nq, rows)):
        b = min(nq, a + rows)
        h1 = torch.relu(X[a:b, None, :] + C[None]).view(-1, 128)
        lg = (torch.relu(torch.addmm(b2, h1, W2.t())) @ w3 + b3).view(b - a, nc)
        lo, hi = bounds[n], bounds[n + 1]
        lg[kq_s[lo:hi] - a, kc_s[lo:hi]] = float("-inf")
        t = torch.topk(lg, k, dim=1)
        cand[a:b], logit[a:b] = t.indices, t.values
    return cand, logit


def _config4(dev):
    from dream_gnn_amd import model as M
    from dream_gnn_amd import synth

    nd, ns = 100_000, 50_000
    torch.manual_seed(7)
    dec = M.MLPDecoder(128).to(dev).eval()
    g = torch.Generator(device=dev).manual_seed(8)
    hd, hs = torch.randn(nd, 128, device=dev, generator=g), torch.randn(ns, 128, device=dev, generator=g)
    kd, ks = synth.bipartite_edges(nd, ns, 10_000_000, 0, dev)
    with torch.no_grad():
        w1 = dec.lin1.weight
        P, Q = torch.addmm(dec.lin1.bias, hd, w1[:, :128].t()), hs @ w1[:, 128:].t()
    return dec, P, Q, kd.long(), ks.long()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", default="config4,single,lrssl")
    ap.add_argument("--k", default="50,128")
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--no-baseline", action="store_true", help="skip the chunked-torch baseline (profiling runs)")
    args = ap.parse_args()

    from dream_gnn_amd import ops

    dev = torch.device("cuda:0")
    ks_list = [int(x) for x in args.k.split(",")]
    cases = args.cases.split(",")
    rows = []

    def emit(row):
        rows.append(row)
        print(json.dumps(row), flush=True)

    if "config4" in cases or "single" in cases:
        dec, P, Q, kd, ks = _config4(dev)
        prm = (dec.lin2.weight, dec.lin2.bias, dec.lin3.weight, dec.lin3.bias)
        nd, ns = P.shape[0], Q.shape[0]
        novel = nd * ns - int(kd.numel())
        if "config4" in cases:
            for k in ks_list:
                for by, X, C, kq, kc in (("disease", Q, P, ks, kd), ("drug", P, Q, kd, ks)):
                    with torch.no_grad():
                        kern = _time(lambda: ops.pair_mlp_row_topk(X, C, *prm, kq, kc, k), args.iters)
                    row = {"case": "config4", "by": by, "n_query": X.shape[0], "n_cand": C.shape[0], "novel_pairs": novel,
                           "k": k, "kernel_s": kern, "tflops": nd * ns * FLOP_PER_PAIR / kern / 1e12}
                    row["fraction_of_155tf"] = row["tflops"] / PEAK_TF
                    if by == "disease" and k == ks_list[0] and not args.no_baseline:
                        with torch.no_grad():
                            base_a = _time(lambda: _baseline_a(X, C, dec, kq, kc, k, max(1, (1 << 26) // C.shape[0])), 1,
                                           warmup=0)
                        row["baseline_a_s"] = base_a
                        row["speedup_kernel_vs_a"] = base_a / kern
                    emit(row)
        if "single" in cases:
            k = ks_list[0]
            X = Q[:1].contiguous()
            sel = ks == 0
            kq, kc = ks[sel], kd[sel]
            with torch.no_grad():
                kern = _time(lambda: ops.pair_mlp_row_topk(X, P, *prm, kq, kc, k), max(args.iters, 20))
            emit({"case": "single", "by": "disease", "n_query": 1, "n_cand": nd, "k": k, "kernel_s": kern})
        del dec, P, Q, kd, ks
        torch.cuda.empty_cache()

    if "lrssl" in cases:
        from dream_gnn_amd import model as M
        from dream_gnn_amd import predict, synth

        torch.manual_seed(0)
        batch, labels = synth.dataset_shaped_batch([(763, 681, 3051)], device=dev)
        net = M.Net(synth.net_args()).to(dev).eval()
        drug, dis, _ = batch["enc_pairs"]
        pos = labels.cpu() > 0
        known = (drug[pos].to(dev), dis[pos].to(dev))
        dec = net.decoder
        with torch.no_grad():
            hd, hs = net.embed(batch["enc_graph"], batch["drug_graph"], batch["drug_sim_feat"], batch["drug_feat"],
                               batch["disease_graph"], batch["disease_sim_feat"], batch["disease_feat"],
                               batch["drug_feature_graph"], batch["disease_feature_graph"])
            w1 = dec.lin1.weight
            F = hd.shape[1]
            P, Q = torch.addmm(dec.lin1.bias, hd, w1[:, :F].t()), hs @ w1[:, F:].t()
            prm = (dec.lin2.weight, dec.lin2.bias, dec.lin3.weight, dec.lin3.bias)
            kd, ks = known[0].long(), known[1].long()
            kern = _time(lambda: ops.pair_mlp_row_topk(Q, P, *prm, ks, kd, 10), max(args.iters, 20))
        e2e = _time(lambda: predict.top_novel_per_disease(net, batch, known, k=10), max(args.iters, 20))
        emit({"case": "lrssl", "by": "disease", "n_query": 681, "n_cand": 763, "k": 10, "kernel_s": kern,
              "top_novel_per_disease_s": e2e})
    print(json.dumps({"novel_lists_bench": rows}))


if __name__ == "__main__":
    main()
