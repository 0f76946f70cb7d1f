"""The workgroup-owned LDS form of the XCD-local SpMM (csrc/dgmi_owned.hip) against the sliced pair, each product of
config 4's shapes in a loop of its own: pair and owned alternating (``sliced_owned`` 0 / 1, 30 calls per timing, 5 times),
bit equality, then the sweep gate lag x rows per lane group.  ``python tools/owned_ab.py [OUT.json]``; with ``pmc`` as the
first argument it only runs three calls of each form per product (lags from ``PMC_LAGS``, default -1; workgroups per CU
from ``PMC_WGS``, default 1), for ``rocprofv3 --pmc`` / ``--kernel-trace`` runs of their own (profiles/owned_rows/,
profiles/owned_wgs/, profiles/owned_slices/).  The loops time both owned forms: one 16-wave workgroup per CU and two 12-wave ones."""
import json, os, sys, statistics
import numpy as np, torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from dream_gnn_amd import _lib, ops

dev = torch.device("cuda")
F = 128
rng = np.random.default_rng(0)

def bip(n_dst, n_src, E, n_slices=8):
    dst = torch.from_numpy(rng.integers(0, n_dst, E).astype(np.int32)).to(dev)
    src = torch.from_numpy(rng.integers(0, n_src, E).astype(np.int32)).to(dev)
    sl = ops.SlicedCSR(dst, src, n_dst, n_src, n_slices=n_slices)
    return sl, sl.indices, False

def knn(n, k=64):
    dst = torch.arange(n, dtype=torch.int32, device=dev).repeat_interleave(k)
    src = torch.from_numpy(rng.integers(0, n, n * k).astype(np.int32)).to(dev)
    sl = ops.SlicedCSR(dst, src, n, n)
    mult = torch.from_numpy(rng.integers(0, 2, n * k).astype(np.int32)).to(dev)
    return sl, (sl.indices | (mult[sl.eid.long()] << ops.MULT_SHIFT)).contiguous(), True

products = {"100k_src_to_50k": bip(50_000, 100_000, 10_000_000), "50k_src_to_100k": bip(100_000, 50_000, 10_000_000),
            "knn_100k": knn(100_000), "knn_50k": knn(50_000),
            # the layout dgmi_sliced_layout_slices gives the first product's class (profiles/owned_slices/): last, so that
            # the graphs above stay the ones of the earlier visits
            "100k_src_to_50k_16_slices": bip(50_000, 100_000, 10_000_000, n_slices=16)}

def timed(sl, ids, id_mult, X, ds, out, n=30):
    for _ in range(5):
        sl.spmm(X, None, ds, out, indices=ids, id_mult=id_mult)
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(n):
        sl.spmm(X, None, ds, out, indices=ids, id_mult=id_mult)
    b.record(); torch.cuda.synchronize()
    return a.elapsed_time(b) / n

def knobs(**kw):
    base = dict(sliced_owned=-1, sliced_owned_wgs=0, sliced_owned_rows=0, sliced_owned_lag=-2, sliced_owned_grid=0)
    base.update(kw)
    for k, v in base.items():
        _lib.set_tuning(k, v)

if len(sys.argv) > 1 and sys.argv[1] == "pmc":
    for name, (sl, ids, id_mult) in products.items():
        X = torch.randn(sl.n_src, F, device=dev)
        ds = torch.rand(sl.n_dst, device=dev) + 0.5
        out = torch.empty(sl.n_dst, F, device=dev)
        knobs(sliced_owned=0)
        for _ in range(3):
            sl.spmm(X, None, ds, out, indices=ids, id_mult=id_mult)
        for wgs in [int(x) for x in os.environ.get("PMC_WGS", "1").split(",")]:
            for lag in [int(x) for x in os.environ.get("PMC_LAGS", "-1").split(",")]:
                knobs(sliced_owned=1, sliced_owned_wgs=wgs, sliced_owned_lag=lag)
                for _ in range(3):
                    sl.spmm(X, None, ds, out, indices=ids, id_mult=id_mult)
        torch.cuda.synchronize()
    knobs()
    sys.exit(0)

res = {}
for name, (sl, ids, id_mult) in products.items():
    X = torch.randn(sl.n_src, F, device=dev)
    ds = torch.rand(sl.n_dst, device=dev) + 0.5
    out = torch.empty(sl.n_dst, F, device=dev)
    r = {"pair": [], "owned": [], "owned_wgs2": []}
    knobs(sliced_owned=0); ref = sl.spmm(X, None, ds, indices=ids, id_mult=id_mult).clone()
    knobs(sliced_owned=1, sliced_owned_wgs=1); got = sl.spmm(X, None, ds, indices=ids, id_mult=id_mult).clone()
    knobs(sliced_owned=1, sliced_owned_wgs=2); got2 = sl.spmm(X, None, ds, indices=ids, id_mult=id_mult)
    r["bit_equal"] = bool(torch.equal(ref, got)) and bool(torch.equal(ref, got2))
    for _ in range(5):
        knobs(sliced_owned=0); r["pair"].append(timed(sl, ids, id_mult, X, ds, out))
        knobs(sliced_owned=1, sliced_owned_wgs=1, sliced_owned_lag=-1); r["owned"].append(timed(sl, ids, id_mult, X, ds, out))
        knobs(sliced_owned=1, sliced_owned_wgs=2, sliced_owned_lag=-1); r["owned_wgs2"].append(timed(sl, ids, id_mult, X, ds, out))
    r["sweep"] = {}
    for wgs in (1, 2):
        for lag in (-1, 0, 1):
            for R in (0, 2, 3, 4, 6):
                knobs(sliced_owned=1, sliced_owned_wgs=wgs, sliced_owned_rows=R, sliced_owned_lag=lag)
                r["sweep"]["wgs%d_lag%d_R%d" % (wgs, lag, R)] = round(timed(sl, ids, id_mult, X, ds, out), 4)
    knobs()
    r["pair_median"], r["owned_median"] = statistics.median(r["pair"]), statistics.median(r["owned"])
    r["owned_wgs2_median"] = statistics.median(r["owned_wgs2"])
    res[name] = r
    print(name, json.dumps(r), flush=True)
if len(sys.argv) > 1:
    json.dump(res, open(sys.argv[1], "w"), indent=1)
