"""The workgroup-owned bf16 gather (``spmm_owned_bf16_kernel``, csrc/dgmi_owned.hip) against the bf16 pair of launches, on the eight config-4
products of bench.py — the A/B the built-in rule's bf16 classes are decided by (profiles/owned_bf16/README.md).

    python tools/bf16_owned_ab.py [--reps 20] [--rounds 7] [--variants pair,owned,rule] [--out profiles/owned_bf16/ab.json]
    rocprofv3 --kernel-trace --stats -d DIR -- python tools/bf16_owned_ab.py --variants rule --rounds 1 --reps 5 --out DIR/run.json

The products are those of tools/bf16_gather_bench.py, built by ``bench.build_ops`` (100 000 drugs x 50 000 diseases,
10 M GCMC edges, kNN-64 graphs, F = 128).  Each runs as ``CSRGraph.spmm(X, ss, ds, gather_dtype=torch.bfloat16)`` — the
conversion pass included — under

  pair    ``sliced_owned = 0``: conversion + ``spmm_sliced_bf16_kernel`` + ``reduce_planes_kernel``, what a bf16 caller ran
          before the owned form took bf16 tables: the baseline
  owned   ``sliced_owned = 1``: conversion + ``spmm_owned_bf16_kernel``
  rule    ``sliced_owned = -1``: what the built-in rule selects — what a caller runs

on the same 8-slice layout, in the same process; the variants ALTERNATE inside every round; ms per call by device events,
median and min .. max over the rounds.  ``step``: the eight products one after the other, per variant.  The variants
must agree bit for bit (checked before anything is timed).  Per product the tool names its class as the rule would:
slices, column rounds, row rounds (one workgroup per CU), multiplicities in the ids, bytes of the bf16 table — and
whether the owned median beats the pair's by more than the pair's own min .. max spread (the bar of
profiles/owned_slices/README.md).  A measurement needs the GPU: there is no fallback.
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

LDS_ROW_BYTES = 144 << 10  # kOwnedLdsRowBytes (csrc/dgmi_owned_common.h)


def _ms(fn, reps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / reps


def plan_class(n_dst, n_src, F, n_slices, cus):
    """The class of a plain bf16 product as ``spmm_owned_try`` sees it: ``sliced_lpr`` at 2 bytes per column (widths
    32 / 16 / 8, half the width where a slice exceeds 4 MiB), then ``owned_plan(..., cols_per_lane = 8)``."""
    f8 = -(-F // 8)
    lpr = next((w for w in (32, 16, 8) if f8 / (-(-f8 // w) * w) >= 0.85), 8)
    if lpr >= 32 and n_dst >= 32768 and -(-n_src // n_slices) * min(16 * lpr, 2 * F) > 4 << 20:
        lpr //= 2
    B = -(-n_dst // cus)
    return dict(slices=n_slices, lpr=lpr, col_rounds=-(-F // (8 * lpr)), row_rounds=-(-B // (LDS_ROW_BYTES // (32 * lpr))),
                table_mib=round(n_src * F * 2 / 2 ** 20, 1))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--variants", default="pair,owned,rule", help="comma-separated: pair, owned, rule")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "owned_bf16", "ab.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bf16_owned_ab.py measures on the MI355X: no GPU visible")
    import bench
    from dream_gnn_amd import _lib

    dev = torch.device("cuda:0")
    bf16 = torch.bfloat16
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    products, _, shape = bench.build_ops(torch, 0, 1, dev, "nodes")
    variants = {k: {"pair": 0, "owned": 1, "rule": -1}[k] for k in args.variants.split(",")}

    def run(c, flag):
        _lib.set_tuning("sliced_owned", flag)
        c["G"].spmm(c["X"], c["ss"], c["ds"], out=c["out"], gather_dtype=bf16)

    cases = []
    try:
        for op in products:
            G = op.shard.local
            ds = None if op.ds is None else op.ds.reshape(-1).contiguous()
            c = dict(name=op.name, G=G, X=op.X, ss=op.ss, ds=ds, out=op.y_local)
            assert G.takes_bf16_gather(bench.F), op.name
            got = {}
            for k, flag in variants.items():
                for _ in range(3):  # also warms every shape the timed windows use
                    run(c, flag)
                got[k] = c["out"].clone()
            assert all(torch.equal(y, next(iter(got.values()))) for y in got.values()), "%s: the forms differ" % op.name
            name, layout = G._layout_of(False)
            c["info"] = dict(name=op.name, nnz=op.nnz, n_dst=G.n_dst, n_src=G.n_src, id_mult=G._mult_ids(name, layout) is not None,
                             **plan_class(G.n_dst, G.n_src, bench.F, layout.n_slices, cus))
            cases.append(c)
        torch.cuda.synchronize()
        times = {c["name"]: {k: [] for k in variants} for c in cases}
        step = {k: [] for k in variants}
        for _ in range(args.rounds):
            for c in cases:
                for k, flag in variants.items():
                    times[c["name"]][k].append(_ms(lambda: run(c, flag), args.reps))
            for k, flag in variants.items():
                step[k].append(_ms(lambda: [run(c, flag) for c in cases], max(1, args.reps // 4)))
    finally:
        _lib.set_tuning("sliced_owned", -1)
    stat = lambda v: dict(ms=round(statistics.median(v), 4), min=round(min(v), 4), max=round(max(v), 4))
    rows = []
    for c in cases:
        t = {k: stat(v) for k, v in times[c["name"]].items()}
        row = dict(c["info"], **t)
        if "pair" in t and "owned" in t:
            spread = t["pair"]["max"] - t["pair"]["min"]
            row.update(pair_spread=round(spread, 4), gain_ms=round(t["pair"]["ms"] - t["owned"]["ms"], 4),
                       clears_bar=bool(t["pair"]["ms"] - t["owned"]["ms"] > spread))
        rows.append(row)
    result = dict(tool="bf16_owned_ab", device=torch.cuda.get_device_name(0), cus=cus, shape=list(shape), F=bench.F,
                  reps=args.reps, rounds=args.rounds,
                  baseline="the bf16 pair (sliced_owned = 0) timed in the same process, alternating with the owned form",
                  products=rows, step={k: stat(v) for k, v in step.items()})
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print(json.dumps(result))


if __name__ == "__main__":
    main()
