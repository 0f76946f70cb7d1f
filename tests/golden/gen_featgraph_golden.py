#!/usr/bin/env python3
"""Generate tests/golden/featgraph_*.npz by running the REFERENCE's ``DrugDataLoader._create_feature_similarity_graph``
in place (build container only).  Arrays only: nothing of the reference's text is stored.

    python tests/golden/gen_featgraph_golden.py        # rewrites the six files, bit-identically

Each file holds ``features`` (N, D) float32, ``k``, ``symm`` (the settings of ``_symm`` that were run) and, per setting
s in {0, 1}, the sparse tensor the reference returned: ``idx_s`` (2, nnz) int64 and ``val_s`` (nnz,) float32, as returned.

  featgraph_n64_k4          64 x  64, k =  4   symm True and False, no zero row
  featgraph_n200_k4        200 x  64, k =  4   symm True
  featgraph_n200_d256_k13  200 x 256, k = 13   symm True
  featgraph_zero_row        64 x  64, k =  4   symm False only, row 17 all zero (data_loader.py:334-335: its norm becomes
                                               1e-10, its similarities are all 0 and its neighbours an arbitrary choice among
                                               ties — unsymmetrised, so that the choice stays inside its own row)
  featgraph_clamp            5 x  64, k =  4   k_actual = N - 1 (data_loader.py:290), both settings
  featgraph_clamp2           3 x  64, k = 20   k_actual = 2, both settings

Features are small integers over 8 (31 levels: the files compress to a byte or less per element, each under 100 KB), drawn
with a seed that is searched — first seed of 0, 1, 2, ... — until, in float64, the k_actual-th and the (k_actual + 1)-th
largest similarity of every non-zero row differ by at least 1e-4: 50 times the 2e-6 of the GPU rule in
tests/test_gpu_knn_exact.py, and two orders above any fp32 error of a similarity, so that every implementation that
orders by cosine similarity picks the same neighbour SETS as the reference's fp32 ``np.dot`` + ``argpartition``.  The gap is
asserted and printed (the smallest one goes into tests/README.md).
"""
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import gen_golden as gg  # noqa: E402  (installs the DGL stand-in, puts the reference on sys.path)

MIN_GAP = 1e-4
# name, N, D, k, settings of _symm, zero rows
CASES = (("n64_k4", 64, 64, 4, (True, False), ()),
         ("n200_k4", 200, 64, 4, (True,), ()),
         ("n200_d256_k13", 200, 256, 13, (True,), ()),
         ("zero_row", 64, 64, 4, (False,), (17,)),
         ("clamp", 5, 64, 4, (True, False), ()),
         ("clamp2", 3, 64, 20, (True, False), ()))


def features_for(seed, N, D, zero):
    rng = np.random.default_rng(seed)
    x = (rng.integers(-15, 16, (N, D)) * 0.125).astype(np.float32)
    # a few heavy columns spread the similarities over a wider range than isotropic rows have
    x[:, :4] *= np.float32(4.0)
    x[list(zero)] = 0
    return x


def kth_gap(x, k, zero):
    """Smallest difference, over the non-zero rows, between the k_actual-th and the (k_actual + 1)-th largest similarity
    (float64).  inf when there is no (k_actual + 1)-th candidate."""
    n = x.shape[0]
    k_actual = min(k, n - 1)
    x64 = x.astype(np.float64)
    norms = np.linalg.norm(x64, axis=1, keepdims=True)
    norms[norms == 0] = 1e-10
    xn = x64 / norms
    s = -np.sort(-(xn @ xn.T), axis=1)
    if k_actual >= n:
        return np.inf
    gap = s[:, k_actual - 1] - s[:, k_actual]
    keep = np.ones(n, dtype=bool)
    keep[list(zero)] = False
    return float(gap[keep].min())


def loader(x, symm):
    ns = types.SimpleNamespace(drug_embed=x, _num_drug=x.shape[0], _symm=symm)
    ns._create_similarity_graph = lambda sim, k: gg.ref_dl.DrugDataLoader._create_similarity_graph(ns, sim, k)
    return ns


def main():
    smallest = np.inf
    for name, N, D, k, symms, zero in CASES:
        seed = 0
        while kth_gap(features_for(seed, N, D, zero), k, zero) < MIN_GAP:
            seed += 1
            assert seed < 100000, "no seed with the gap found"
        x = features_for(seed, N, D, zero)
        gap = kth_gap(x, k, zero)
        assert gap >= MIN_GAP
        smallest = min(smallest, gap)
        arrays = dict(features=x, k=np.int64(k), symm=np.array(symms, dtype=bool))
        for symm in symms:
            g = gg.ref_dl.DrugDataLoader._create_feature_similarity_graph(loader(x, symm), "drug", k)
            assert g.dtype == gg.th.float32 and tuple(g.shape) == (N, N)
            arrays["idx_%d" % int(symm)] = g._indices().numpy().astype(np.int64)
            arrays["val_%d" % int(symm)] = g._values().numpy()
        gg.save("featgraph_" + name, **arrays)
        path = os.path.join(HERE, "featgraph_" + name + ".npz")
        assert os.path.getsize(path) < 100 * 1024
        print("    seed %d, smallest k-th gap %.3e, nnz %s" % (seed, gap, [arrays["val_%d" % int(s)].size for s in symms]))
    print("smallest gap of all fixtures: %.3e" % smallest)


if __name__ == "__main__":
    main()
