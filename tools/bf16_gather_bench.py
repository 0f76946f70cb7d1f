"""The bf16 gather of the XCD-local SpMM against the fp32 product, on the eight config-4 products of bench.py.

    python tools/bf16_gather_bench.py [--reps 20] [--rounds 7] [--out profiles/bf16_gather_bench.json]
    rocprofv3 --kernel-trace --stats -d DIR -- python tools/bf16_gather_bench.py --rounds 1 --reps 5 --out DIR/run.json

The products are built by ``bench.build_ops`` itself (same generators and seeds from ``synth``: 100 000 drugs x 50 000
diseases, 10 M GCMC edges, kNN-64 graphs, F = 128).  Per product, ms per call by device events — the variants ALTERNATE
inside every round and the median over the rounds is reported, with the spread (min .. max) beside it:

  fp32        ``CSRGraph.spmm(X, ss, ds, gather_dtype=torch.float32)``: the product as it runs without the feature, in this
              same process (pre-scale pass + fp32 gather + plane reduce)
  bf16        ``CSRGraph.spmm(X, ss, ds, gather_dtype=torch.bfloat16)``: conversion pass + bf16 gather + plane reduce
  gather      the bf16 gather + plane reduce on a table converted beforehand
  convert     ``rows_to_bf16`` alone
  step        the eight products one after the other (each product's ids and table pushed out of the caches by the
              others, as in a training step), fp32 against bf16

and the largest ``|y_bf16 - y_fp32|`` relative to ``max |y_fp32|`` (the rounding of the gathered operand; the
accuracy contract is tests/test_gpu_spmm_bf16.py's).  A measurement needs the GPU: there is no fallback.
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


def _ms(fn, reps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / reps


def _pieces(G, ss, ds):
    """The layout, the scale on the gathered rows, the scale on the output rows and the keywords ``CSRGraph.spmm`` runs
    the plain XCD-local product with (values that are `scale x multiplicity` ride in the id words)."""
    S = G._S
    mult = G._mult_ids("sliced", S.sliced)
    if mult is None:
        return S.sliced, ss, ds, dict(vals=G._vals_for("sliced", S.sliced.eid))
    if mult[0] == "row":
        ds = G._fold(mult[1], ds)
    else:
        ss = G._fold(mult[1], ss)
    return S.sliced, ss, ds, dict(vals=None, indices=mult[2], id_mult=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bf16_gather_bench.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bf16_gather_bench.py measures on the MI355X: no GPU visible")
    import bench
    from dream_gnn_amd import ops

    dev = torch.device("cuda:0")
    bf16, f32 = torch.bfloat16, torch.float32
    products, _, shape = bench.build_ops(torch, 0, 1, dev, "nodes")
    cases = []
    for op in products:
        G = op.shard.local
        ds = None if op.ds is None else op.ds.reshape(-1).contiguous()
        y32 = G.spmm(op.X, op.ss, ds, gather_dtype=f32).clone()
        assert G._S.sliced is not None and G.takes_bf16_gather(bench.F), op.name
        layout, gs, os_, kw = _pieces(G, op.ss, ds)
        xb = ops.rows_to_bf16(op.X, gs)
        y16 = G.spmm(op.X, op.ss, ds, gather_dtype=bf16)
        assert torch.equal(y16, layout.spmm(xb, None, os_, **kw)), op.name
        out = op.y_local
        cases.append(dict(
            name=op.name, nnz=op.nnz, n_dst=G.n_dst, n_src=G.n_src, weighted=op.weighted,
            rel_diff=float((y16 - y32).abs().max() / y32.abs().max()),
            fns=dict(fp32=lambda G=G, op=op, ds=ds, out=out: G.spmm(op.X, op.ss, ds, out=out, gather_dtype=f32),
                     bf16=lambda G=G, op=op, ds=ds, out=out: G.spmm(op.X, op.ss, ds, out=out, gather_dtype=bf16),
                     gather=lambda layout=layout, xb=xb, os_=os_, out=out, kw=kw: layout.spmm(xb, None, os_, out, **kw),
                     convert=lambda op=op, gs=gs: ops.rows_to_bf16(op.X, gs))))
        del y32, y16
    for c in cases:  # warm every shape the timed windows use
        for fn in c["fns"].values():
            for _ in range(3):
                fn()
    torch.cuda.synchronize()
    times = {c["name"]: {k: [] for k in c["fns"]} for c in cases}
    step = {"fp32": [], "bf16": []}
    for _ in range(args.rounds):
        for c in cases:
            for k, fn in c["fns"].items():
                times[c["name"]][k].append(_ms(fn, args.reps))
        for k in step:
            step[k].append(_ms(lambda: [c["fns"][k]() for c in cases], max(1, args.reps // 4)))
    stat = lambda v: dict(ms=round(statistics.median(v), 4), min=round(min(v), 4), max=round(max(v), 4))
    result = dict(tool="bf16_gather_bench", device=torch.cuda.get_device_name(0), shape=list(shape), F=bench.F, reps=args.reps,
                  rounds=args.rounds, baseline="the fp32 product (gather_dtype=float32) timed in the same process",
                  products=[dict({k: v for k, v in c.items() if k != "fns"}, **{k: stat(v) for k, v in times[c["name"]].items()},
                                 speedup=round(statistics.median(times[c["name"]]["fp32"]) / statistics.median(times[c["name"]]["bf16"]), 3))
                            for c in cases],
                  step={k: stat(v) for k, v in step.items()})
    result["step"]["speedup"] = round(result["step"]["fp32"]["ms"] / result["step"]["bf16"]["ms"], 3)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print(json.dumps(result))


if __name__ == "__main__":
    main()
