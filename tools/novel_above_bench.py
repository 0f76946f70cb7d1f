"""Novel pairs by score and beyond k = 1024: the streaming emit + record sort against the on-chip top-k (one JSON line).

    python tools/novel_above_bench.py [--shapes lrssl,config4] [--iters 3] [--out profiles/novel_above_bench.json]

Shapes: lrssl (763 x 681, the dataset, a full ``Net``) and the config-4 node counts (100 000 x 50 000 = 5e9 pairs, random
width-128 embeddings into ``MLPDecoder``), known pairs from ``synth`` — the set-up of tools/novel_pairs_bench.py.
Timed with device events after a warm-up, medians over ``--iters``.  The yardstick is the on-chip top-k in the same
process: ``topk_op_s`` = ``ops.pair_mlp_topk`` at k = 1024, ``top_pairs_s`` = ``MLPDecoder.top_pairs`` at k = 1024.
  count_s        ``ops.pair_mlp_count_above``: one emit pass with capacity 0 (the emit kernel and the count read)
  above_s        ``ops.pair_mlp_above``: emit pass, count read, record sort (config 4: cuts that let ~1e5 and ~1e6 pairs
                 through, taken from a deep top-k; lrssl: min_score = 0.5)
  sort_s         ``dreamgnn_mi::pair_records_sort`` alone on that many records
  deep_s         ``MLPDecoder.top_pairs_deep`` (config 4: k = 10 000 and 100 000; lrssl: ``predict.top_novel_pairs_deep``
                 at k = 5 000, end to end with the encoder)
Ratios against the yardstick are in the rows (``count_vs_topk_op``, ``deep_vs_top_pairs``); for them the two sides are
timed in turn (a, b, a, b, ...).  Kernel-level times come
from a separate ``rocprofv3 --kernel-trace --stats`` run of this tool (profiles/novel_above_kernel_stats.csv).
"""
from __future__ import annotations

import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import torch  # noqa: E402

from novel_pairs_bench import _shape, _time  # noqa: E402


def _time_alternating(fns, iters):
    """Medians of several functions timed in turn (a, b, a, b, ...), so that drift of the machine hits all alike."""
    import statistics

    for fn in fns:
        fn()
    torch.cuda.synchronize()
    ts = [[] for _ in fns]
    for _ in range(iters):
        for t, fn in zip(ts, fns):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            b.synchronize()
            t.append(a.elapsed_time(b) / 1e3)
    return [statistics.median(t) for t in ts]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="lrssl,config4")
    ap.add_argument("--iters", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "novel_above_bench.json"))
    args = ap.parse_args()

    from dream_gnn_amd import ops, predict

    dev = torch.device("cuda:0")
    rows = []
    for name in args.shapes.split(","):
        s = _shape(name, dev)
        dec, hd, hs, nd, ns = s["dec"], s["hd"], s["hs"], s["nd"], s["ns"]
        kd, ks = s["known"]
        with torch.no_grad():
            P, Q = dec._split_lin1(hd, hs)
            tail = dec._tail()
            base = {"shape": name, "n_drug": nd, "n_dis": ns}
            topk_op = _time(lambda: ops.pair_mlp_topk(P, Q, *tail, kd, ks, 1024), args.iters)
            top_pairs = _time(lambda: dec.top_pairs(hd, hs, 1024, (kd, ks)), args.iters)
            rows.append(dict(base, case="on-chip top-k, k = 1024", topk_op_s=topk_op, top_pairs_s=top_pairs))
            print(json.dumps(rows[-1]), flush=True)

            if name == "config4":
                deep_ks, cut_ranks = (10_000, 100_000), (100_000, 1_000_000)
                ranked = dec.top_pairs_deep(hd, hs, max(cut_ranks), (kd, ks))[2]
                cuts = [float(ranked[r - 1]) for r in cut_ranks]
                del ranked
            else:
                deep_ks, cuts = (5_000,), [predict._cut_logit(0.5, None)]

            for cut in cuts:
                n = ops.pair_mlp_count_above(P, Q, *tail, kd, ks, cut)
                # the emit pass against the yardstick, in turn
                topk_alt, count_s = _time_alternating([lambda: ops.pair_mlp_topk(P, Q, *tail, kd, ks, 1024),
                                                       lambda: ops.pair_mlp_count_above(P, Q, *tail, kd, ks, cut)], args.iters)
                above_s = _time(lambda: ops.pair_mlp_above(P, Q, *tail, kd, ks, cut, 1 << 21), args.iters)
                d, j, l, _ = ops.pair_mlp_above(P, Q, *tail, kd, ks, cut, 1 << 21)
                d, j, l = d.int(), j.int(), l.clone()
                perm = torch.randperm(n, device=dev)
                d, j, l = d[perm].contiguous(), j[perm].contiguous(), l[perm].contiguous()  # (re-sorting sorted input after the warm-up)
                sort_s = _time(lambda: torch.ops.dreamgnn_mi.pair_records_sort(d, j, l, n), args.iters)
                rows.append(dict(base, case="pairs at or above a cut", min_logit=cut, pairs=n, count_s=count_s, above_s=above_s,
                                 sort_s=sort_s, topk_op_in_turn_s=topk_alt, count_vs_topk_op=count_s / topk_alt,
                                 above_vs_topk_op=above_s / topk_alt))
                print(json.dumps(rows[-1]), flush=True)
                del d, j, l, perm

            for k in deep_ks:
                if s["net"] is not None:
                    e2e = _time(lambda: predict.top_novel_pairs(s["net"], s["batch"], s["known"], k=1024), args.iters)
                    deep = _time(lambda: predict.top_novel_pairs_deep(s["net"], s["batch"], s["known"], k=k), args.iters)
                    rows.append(dict(base, case="deep top-k, end to end", k=k, top_novel_pairs_1024_s=e2e, deep_s=deep,
                                     deep_vs_top_novel_pairs=deep / e2e))
                else:
                    top_alt, deep = _time_alternating([lambda: dec.top_pairs(hd, hs, 1024, (kd, ks)),
                                                       lambda: dec.top_pairs_deep(hd, hs, k, (kd, ks))], args.iters)
                    rows.append(dict(base, case="deep top-k", k=k, top_pairs_in_turn_s=top_alt, deep_s=deep,
                                     deep_vs_top_pairs=deep / top_alt))
                print(json.dumps(rows[-1]), flush=True)
        del s, P, Q
        torch.cuda.empty_cache()
    result = json.dumps({"novel_above_bench": rows})
    print(result)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(result + "\n")


if __name__ == "__main__":
    main()
