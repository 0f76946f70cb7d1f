"""Scoring and ranking GIVEN pairs: the list scorer and the count scan against what a user does without them and against
the per-row top-k on the same tables (one JSON line).

    python tools/rank_pairs_bench.py [--shapes lrssl,config4] [--iters 3] [--out profiles/rank_pairs_bench.json]

Shapes (the set-up of tools/novel_pairs_bench.py): lrssl (763 drugs x 681 diseases, a full ``Net``; the list is every
known association, a held-out-sized list) and the config-4 node counts (100 000 drugs x 50 000 diseases, random width-128
embeddings into ``MLPDecoder``, 10 M known pairs; the list is 10 000 random pairs).  Every list is ranked ``by="disease"``:
a pair's drug among all drugs for its disease.  Timed with device events after a warm-up, medians over ``--iters``.
  score_s        ``MLPDecoder.score_pairs``: the lin1 split and the list scorer
  rank_s         ``MLPDecoder.rank_pairs``: the lin1 split, the renumbering to the distinct listed rows, list scorer, bitmap,
                 count scan and the flag read
  rank_op_s      ``ops.pair_mlp_rank_list`` alone on the prepared tables; ``rank_pairs_per_s`` = n_pairs x n_cand / rank_op_s
  row_topk_s     (b) ``ops.pair_mlp_row_topk`` at k = 50 on the same tables (the distinct listed rows as queries, the same
                 known list); ``row_topk_pairs_per_s`` = n_distinct x n_cand / row_topk_s.  The scan does the same MFMA work
                 per pair without the list upkeep: ``rank_vs_row_topk_rate`` >= 1 is the expectation
  torch_s        (a) without the feature: chunks of distinct rows scored in fp32 torch (broadcast add, relu, GEMM, relu, dot),
                 known pairs masked, a comparison count per listed pair
  end_to_end     (lrssl) ``predict.score_pairs`` / ``predict.rank_pairs`` with the encoder
The two ops of the rate comparison are timed in turn (a, b, a, b, ...).
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

from novel_above_bench import _time_alternating  # noqa: E402
from novel_pairs_bench import _shape, _time  # noqa: E402


def _torch_ranks(X, C, tail, pq, pc, kq, kc, rows):
    """(a): ``above`` / ``total`` of the listed pairs in plain fp32 torch, ``rows`` distinct query rows at a time."""
    W2, b2, w3, b3 = tail
    w3 = w3.reshape(-1)
    n_cand = C.shape[0]
    order = torch.argsort(pq)
    pq_s, pc_s = pq[order], pc[order]
    known_keys = torch.sort(kq.long() * n_cand + kc.long()).values
    ids = torch.arange(n_cand, device=X.device)
    above = torch.empty_like(pq)
    total = torch.empty_like(pq)
    for a in range(0, X.shape[0], rows):
        b = min(X.shape[0], a + rows)
        lo, hi = (int(v) for v in torch.searchsorted(pq_s, torch.tensor([a, b], device=X.device)))
        if lo == hi:
            continue
        h1 = torch.relu(X[a:b, None, :] + C[None]).view(-1, 128)
        L = (torch.relu(torch.addmm(b2, h1, W2.t())) @ w3 + b3).view(b - a, n_cand)
        keys = torch.arange(a * n_cand, b * n_cand, device=X.device)
        novel = ~torch.isin(keys, known_keys).view(b - a, n_cand)
        q, c = pq_s[lo:hi] - a, pc_s[lo:hi]
        Lp, t = L[q], L[q, c][:, None]
        valid = novel[q] & (ids[None, :] != c[:, None])
        before = (Lp > t) | ((Lp == t) & (ids[None, :] < c[:, None]))  # (NaN logits are not expected from random tables)
        above[order[lo:hi]] = (valid & before).sum(1)
        total[order[lo:hi]] = valid.sum(1)
    return above, total


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="lrssl,config4")
    ap.add_argument("--iters", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "rank_pairs_bench.json"))
    args = ap.parse_args()

    from dream_gnn_amd import ops, predict
    from dream_gnn_amd.model import _remap_known

    dev = torch.device("cuda:0")
    rows = []
    for name in args.shapes.split(","):
        s = _shape(name, dev)
        dec, hd, hs, nd, ns = s["dec"], s["hd"], s["hs"], s["nd"], s["ns"]
        kd, ks = (t.long() for t in s["known"])
        if name == "lrssl":
            drug, dis = kd.clone(), ks.clone()  # every known association: the size of a held-out list
        else:
            g = torch.Generator(device=dev).manual_seed(9)
            drug = torch.randint(0, nd, (10_000,), device=dev, generator=g)
            dis = torch.randint(0, ns, (10_000,), device=dev, generator=g)
        n_pairs = int(drug.numel())
        with torch.no_grad():
            P, Q = dec._split_lin1(hd, hs)
            tail = dec._tail()
            # the tables MLPDecoder.rank_pairs hands to the op (by="disease")
            distinct = torch.unique(dis)
            pos = torch.full((ns,), -1, dtype=torch.long, device=dev)
            pos[distinct] = torch.arange(distinct.numel(), device=dev)
            X, C, pq, pc = Q.index_select(0, distinct), P, pos[dis], drug
            kq, kc = _remap_known(ks, kd, distinct, ns, nd)
            n_distinct = int(distinct.numel())

            score_s = _time(lambda: dec.score_pairs(hd, hs, drug, dis), args.iters)
            rank_s = _time(lambda: dec.rank_pairs(hd, hs, drug, dis, "disease", (kd, ks)), args.iters)
            rank_op_s, row_topk_s = _time_alternating([lambda: ops.pair_mlp_rank_list(X, C, *tail, pq, pc, kq, kc),
                                                       lambda: ops.pair_mlp_row_topk(X, C, *tail, kq, kc, 50)], args.iters)
            chunk = max(1, (1 << 23) // nd)  # ~8 M pairs (a 4 GB fp32 hidden block) per chunk
            torch_s = _time(lambda: _torch_ranks(X, C, tail, pq, pc, kq, kc, chunk), 1 if nd > 10_000 else args.iters)
            # the two agree (fp32 torch rounds differently: ranks may move where logits are within rounding)
            _, above, total = ops.pair_mlp_rank_list(X, C, *tail, pq, pc, kq, kc)
            t_above, t_total = _torch_ranks(X, C, tail, pq, pc, kq, kc, chunk)
            row = {"shape": name, "by": "disease", "n_query": ns, "n_cand": nd, "n_pairs": n_pairs, "n_distinct_rows": n_distinct,
                   "known_pairs": int(kd.numel()), "score_s": score_s, "score_pairs_per_s": n_pairs / score_s, "rank_s": rank_s,
                   "rank_op_s": rank_op_s, "rank_pairs_per_s": n_pairs * nd / rank_op_s, "row_topk_k50_s": row_topk_s,
                   "row_topk_pairs_per_s": n_distinct * nd / row_topk_s, "torch_s": torch_s, "speedup_rank_vs_torch": torch_s / rank_s,
                   "total_equal_to_torch": bool(torch.equal(total.long(), t_total)),
                   "max_rank_difference_to_torch": int((above.long() - t_above).abs().max())}
            row["rank_vs_row_topk_rate"] = row["rank_pairs_per_s"] / row["row_topk_pairs_per_s"]
            if s["net"] is not None:
                known = (kd, ks)
                row["predict_score_pairs_s"] = _time(lambda: predict.score_pairs(s["net"], s["batch"], drug, dis), args.iters)
                row["predict_rank_pairs_s"] = _time(lambda: predict.rank_pairs(s["net"], s["batch"], drug, dis, known), args.iters)
            rows.append(row)
            print(json.dumps(row), flush=True)
        del s, P, Q, X, C
        torch.cuda.empty_cache()
    result = json.dumps({"rank_pairs_bench": rows})
    print(result)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(result + "\n")


if __name__ == "__main__":
    main()
