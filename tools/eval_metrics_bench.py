"""Evaluation metrics on the host against the device, in one process on an MI355X.

    python tools/eval_metrics_bench.py --out DIR/times.json            # the timing run (profiler off)
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR/trace_NAME -- \
        python tools/eval_metrics_bench.py --profile NAME --out DIR/trace_NAME/run.json   # one config, device path only
    python tools/eval_metrics_bench.py --summarise DIR/trace_NAME       # kernel groups, shares, bytes per second

Configs: the lrssl decoder list (467 643 samples, 681 diseases) and a config-4 list (10 M samples, 50 000 diseases), each
overall ("global") and per disease.  Host path = what `harness.evaluate` does after the forward: both tensors copied to
the host, then `harness.auroc_aupr` (per disease: a stable argsort by disease and one call per disease with both
classes).  Device path = `ops.curve_areas(check=False)`, nothing read back, one synchronise at the end of the timed
window.  The two alternate round by round; times are host-clock around work that ends in a synchronise.  The bytes are
those DESIGN 4.14 lists per launch, computed here from the shapes."""
import argparse
import csv
import glob
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

CONFIGS = {
    "lrssl_global": (467_643, 0), "lrssl_disease": (467_643, 681),
    "cfg4_global": (10_000_000, 0), "cfg4_disease": (10_000_000, 50_000),
}
GROUPS = {  # kernel-name fragment -> group
    "curve_keys_kernel": "keys", "sort_hist_kernel": "sort", "sort_bucket_totals_kernel": "sort",
    "sort_bucket_scan_kernel": "sort", "sort_scatter_kernel": "sort", "curve_tile_counts_kernel": "scan",
    "curve_count_carry_kernel": "scan", "curve_tile_terms_kernel": "scan", "curve_close_segments_kernel": "scan",
    "curve_finish_kernel": "finish",
}


def bytes_moved(n, n_segments):
    """Bytes per call of each kernel group: 4-byte fields, digits of up to 9 bits."""
    seg = 4 * n if n_segments else 0
    passes = lambda bits: (bits + 8) // 9
    seg_bits = max(1, int(n_segments).bit_length()) if n_segments else 0  # ids 0 .. S (S = the trash segment)
    per_pass = 4 * n + 12 * n + 12 * n  # histogram reads the key; scatter reads and writes the 12-byte records
    return {"keys": 8 * n + seg + 12 * n, "sort": (passes(32) + (passes(seg_bits) if n_segments else 0)) * per_pass,
            "scan": 2 * (8 * n + seg), "finish": max(n_segments, 1) * (48 + 16 + 16)}


def make(name, dev):
    import torch

    n, S = CONFIGS[name]
    gen = torch.Generator(device=dev).manual_seed(n + S)
    label = (torch.rand(n, device=dev, generator=gen) < 0.1).float()
    score = torch.randn(n, device=dev, generator=gen) + 1.5 * label  # fp32 logits, positives shifted up
    seg = torch.randint(0, S, (n,), device=dev, generator=gen, dtype=torch.int32) if S else None
    return score, label, seg, S


def host_path(score, label, seg, S):
    from dream_gnn_amd import harness

    y, s = label.cpu().numpy(), score.cpu().numpy()  # the copy is part of the path
    if seg is None:
        return [harness.auroc_aupr(y, s)]
    ids = seg.cpu().numpy()
    order = np.argsort(ids, kind="stable")
    cuts = np.searchsorted(ids[order], np.arange(S + 1))
    out = []
    for q in range(S):
        idx = order[cuts[q]:cuts[q + 1]]
        pos = y[idx].sum()
        out.append(harness.auroc_aupr(y[idx], s[idx]) if 0 < pos < idx.size else (np.nan, np.nan))
    return out


def device_path(score, label, seg, S, reps):
    import torch
    from dream_gnn_amd import ops

    for _ in range(reps):
        st = ops.curve_areas(score, label, seg, S, check=False)
    torch.cuda.synchronize()
    return st


def timed(fn):
    t0 = time.perf_counter()
    out = fn()
    return time.perf_counter() - t0, out


def spread(xs):
    xs = sorted(xs)
    return {"median_ms": 1e3 * xs[len(xs) // 2], "min_ms": 1e3 * xs[0], "max_ms": 1e3 * xs[-1], "runs": len(xs)}


def run_timing(args, dev):
    import torch

    result = {"device": torch.cuda.get_device_name(0), "rounds": args.rounds, "reps": args.reps, "configs": {}}
    for name in args.configs:
        score, label, seg, S = make(name, dev)
        n = score.numel()
        device_path(score, label, seg, S, 3)  # warm-up: code objects, allocator blocks
        host_t, dev_t = [], []
        host_rounds = args.rounds if n < 2_000_000 else min(args.rounds, 3)
        for r in range(args.rounds):
            if r < host_rounds:
                t, host = timed(lambda: host_path(score, label, seg, S))
                host_t.append(t)
            t, st = timed(lambda: device_path(score, label, seg, S, args.reps))
            dev_t.append(t / args.reps)
        host = np.asarray(host, dtype=np.float64)
        got = st.area.cpu().numpy()
        both = ~np.isnan(host[:, 0])
        gap = float(np.abs(got[both] - host[both]).max())  # faster and different is not faster
        assert gap <= 4 * n * 2.0 ** -53, (name, gap)
        entry = {"n": n, "n_segments": S, "host": spread(host_t), "device": spread(dev_t), "max_abs_gap": gap,
                 "bytes_per_call": bytes_moved(n, S)}
        entry["host_over_device"] = entry["host"]["median_ms"] / entry["device"]["median_ms"]
        result["configs"][name] = entry
        print(json.dumps({name: entry}), flush=True)
    return result


def run_profile(args, dev):
    name = args.profile
    score, label, seg, S = make(name, dev)
    warm = 3
    device_path(score, label, seg, S, warm)
    t, _ = timed(lambda: device_path(score, label, seg, S, args.reps))
    n = score.numel()
    return {"config": name, "n": n, "n_segments": S, "calls": warm + args.reps, "ms_per_call_under_trace": 1e3 * t / args.reps,
            "bytes_per_call": bytes_moved(n, S)}


def summarise(path):
    run = json.load(open(os.path.join(path, "run.json")))
    files = glob.glob(os.path.join(path, "**", "*kernel_stats.csv"), recursive=True)
    if not files:
        raise SystemExit("no *kernel_stats.csv under " + path)
    ns = {g: 0.0 for g in ("keys", "sort", "scan", "finish", "other")}
    for row in csv.DictReader(open(files[0])):
        group = next((g for frag, g in GROUPS.items() if frag in row["Name"]), "other")
        ns[group] += float(row["TotalDurationNs"])
    ours = sum(v for g, v in ns.items() if g != "other")
    out = {"config": run["config"], "n": run["n"], "n_segments": run["n_segments"], "calls": run["calls"], "groups": {}}
    for g in ("keys", "sort", "scan", "finish"):
        per_call = ns[g] / run["calls"]
        out["groups"][g] = {"us_per_call": per_call / 1e3, "share": ns[g] / ours,
                            "GB_per_s": run["bytes_per_call"][g] / per_call if per_call else None}
    out["kernel_us_per_call"] = ours / run["calls"] / 1e3
    out["other_kernels_us_total"] = ns["other"] / 1e3  # data generation, fills
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", nargs="+", default=list(CONFIGS), choices=list(CONFIGS))
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--profile", choices=list(CONFIGS))
    ap.add_argument("--summarise")
    ap.add_argument("--out")
    args = ap.parse_args()
    if args.summarise:
        result = summarise(args.summarise)
    else:
        import torch

        if not torch.cuda.is_available():
            raise SystemExit("eval_metrics_bench.py measures on an MI355X; there is no GPU here")
        dev = torch.device("cuda:0")
        result = run_profile(args, dev) if args.profile else run_timing(args, dev)
    text = json.dumps(result, indent=1)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        open(args.out, "w").write(text + "\n")


if __name__ == "__main__":
    main()
