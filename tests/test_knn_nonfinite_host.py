"""The non-finite contract of the cosine kNN on the host (no GPU): the reference of test_gpu_knn_nonfinite.py inside its
own zero tolerance, the designs of _knn_nonfinite_cases.py placed where they claim, the builder's finiteness check, and
`graph.feature_similarity_graph` on CPU tensors against the fixtures the reference's own
`_create_feature_similarity_graph` wrote (tests/golden/featgraph_*.npz, tests/golden/gen_featgraph_golden.py)."""
import numpy as np
import pytest
import torch

import _knn_nonfinite_cases as NF

HOST_SHAPES = NF.SMALL_SHAPES + NF.RECT_SHAPES


def _brute(case, k):
    """Lists by `sorted()` on tuple keys over a table the NaN rows were REMOVED from, ids mapped back."""
    fin = [int(i) for i in np.flatnonzero(case.finite)]
    num = case.lat.num[fin].astype(np.int64)
    S = num @ num.T
    out = np.full((case.lat.N, k), -1, dtype=np.int64)
    for a, q in enumerate(fin):
        order = sorted(range(len(fin)), key=lambda b: (-int(S[a, b]), fin[b]))[:k]
        out[q, :len(order)] = [fin[b] for b in order]
    return out


@pytest.mark.parametrize("N,D,k", HOST_SHAPES, ids=str)
def test_expected_lists_equal_brute_force_without_the_nan_rows(N, D, k):
    case = NF.nan_case(N, D)
    want = NF.expected_lists(case, k)
    assert np.array_equal(want, _brute(case, k))
    assert (want[~case.finite] == -1).all() and (want[case.finite] >= 0).all()
    assert case.finite[want[case.finite]].all()          # no NaN row in any list


@pytest.mark.parametrize("few", [NF.FEW_33, NF.FEW_1536], ids=["33", "1536"])
def test_fewer_finite_rows_than_k(few):
    N, D, k, keep = few
    case = NF.few_case(N, D, k, keep)
    assert int(case.finite.sum()) == len(keep) < k and (N, len(keep)) in ((33, 13), (1536, 6))
    want = NF.expected_lists(case, k)
    assert np.array_equal(want, _brute(case, k))
    for q in keep:
        assert sorted(want[q, :len(keep)].tolist()) == sorted(keep) and (want[q, len(keep):] == -1).all()
    if N == 1536:   # the finite rows lie in five different 128-row tiles, one of them the last
        assert len({q // 128 for q in keep}) == 5 and max(keep) // 128 == 11
    # the magnets: row -1 is a copy of the first finite row, row N of the last — similarity exactly 1 to their sources
    before, after = NF.magnets(case)
    assert torch.equal(before[1], case.x[keep[0]]) and torch.equal(after[0], case.x[keep[-1]])
    assert torch.equal(before[0], case.x[keep[1]]) and torch.equal(after[1], case.x[keep[-2]])
    assert bool(torch.isfinite(before).all()) and bool(torch.isfinite(after).all())


@pytest.mark.parametrize("N,D,k", NF.SMALL_SHAPES + NF.RECT_SHAPES + NF.TRI_SHAPES + NF.BIG_SHAPES + [NF.EXACT_ROWS_SHAPE], ids=str)
def test_nan_rows_sit_where_the_design_says(N, D, k):
    case = NF.nan_case(N, D)
    d = case.lat
    p = NF.placement(d)
    t = NF.tile_of(N)
    lo, hi = d.block
    assert all(r < 32 for r in p["front"])                                     # tile 0, always sampled
    assert all(lo <= r < hi for r in p["block"])                               # inside the copies
    assert all(r // t == (N - 1) // t for r in p["last_tile"])                 # the last tile (ragged unless N % t == 0)
    assert set(case.bad) == {r for v in p.values() for r in v}
    if N >= 64:
        assert p["block"][1] + 1 == p["block"][2] and p["block"][1] // t + 1 == p["block"][2] // t   # across a tile boundary
        # a finite query in the middle has NaN candidates in tiles before its own (second direction of the triangular
        # sweep), inside its own diagonal tile, and behind it
        q = p["block"][0] + 1
        assert case.finite[q] and q // t == p["block"][0] // t
        assert min(case.bad) // t < q // t < max(case.bad) // t
    # both forms, and every bit pattern, survive into the tensor
    x = case.x.numpy()
    u = x.view(np.uint32)
    assert set(case.forms.values()) == {"one", "all"}
    seen = set()
    for r in case.bad:
        nan = np.isnan(x[r])
        assert nan.sum() == (1 if case.forms[r] == "one" else D)
        seen |= set(u[r][nan].tolist())
    assert seen <= set(NF.NAN_BITS) and (len(case.bad) < 6 or seen == set(NF.NAN_BITS))
    assert torch.equal(torch.isnan(case.x).any(dim=1), torch.from_numpy(~case.finite))
    # torch's own bf16 conversion keeps all of them NaN; the rounding the screen had did not
    assert bool(torch.isnan(case.x[list(case.bad)].to(torch.bfloat16).float()).any(dim=1).all())


def test_the_old_bf16_rounding_loses_these_nans():
    """Why the payloads are there: `(u + 0x7fff + lsb) >> 16` makes +Inf, -0, +0 and -Inf of four of the six patterns."""
    got = [int(v) for v in NF.old_bf16_bits(np.array(NF.NAN_BITS, dtype=np.uint64))]
    assert got == [0x7FC0, 0x7F80, 0x8000, 0x0000, 0xFF80, 0xFFC0]


@pytest.mark.parametrize("N,D,k", NF.INF_SHAPES[:3], ids=str)
def test_inf_rows_hold_no_nan(N, D, k):
    case = NF.inf_case(N, D)
    x = case.x
    assert not bool(torch.isnan(x).any())
    assert set(case.forms.values()) == {"one", "all", "both"}
    signs = {float(v) for r in case.bad for v in x[r][torch.isinf(x[r])].tolist()}
    assert signs == {float("inf"), float("-inf")}
    # ... but their similarities do: +Inf, -Inf and NaN all occur
    s = x[list(case.bad)].double() @ x.double().t()
    assert bool(torch.isnan(s).any()) and bool((s == float("inf")).any()) and bool((s == float("-inf")).any())


# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bad", [float("nan"), float("inf"), float("-inf")], ids=["nan", "inf", "-inf"])
def test_builder_refuses_non_finite_features(monkeypatch, bad):
    from dream_gnn_amd import graph as G, ops

    counter = NF.Counting(ops._T)
    monkeypatch.setattr(ops, "_T", counter)
    x = torch.randn(40, 16, generator=torch.Generator().manual_seed(1))
    rows = [3, 5, 8, 13, 21, 22, 23, 24, 25, 39]
    for i, r in enumerate(rows):
        x[r, (3 * i) % 16] = bad
    with pytest.raises(ValueError) as e:
        G.feature_similarity_graph(x, 4)
    msg = str(e.value)
    assert "10 of 40" in msg and "3, 5, 8, 13, 21, 22, 23, 24" in msg and "39" not in msg
    with pytest.raises(ValueError):
        G.feature_similarity_graph(x, 4, fused=False)
    assert counter.calls == 0


def test_builder_accepts_a_zero_row():
    from dream_gnn_amd import graph as G

    x = torch.randn(40, 16, generator=torch.Generator().manual_seed(2))
    x[7] = 0
    a = G.feature_similarity_graph(x, 4).coalesce()
    rowsum = torch.zeros(40, dtype=torch.float64).index_add_(0, a.indices()[0], a.values().double())
    assert float((rowsum - 1).abs().max()) <= 1e-6


# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", NF.FEATGRAPH)
def test_feature_graph_equals_the_reference_on_cpu(name):
    from dream_gnn_amd import graph as G

    NF.compare_with_fixture(name, lambda x, k, symm: G.feature_similarity_graph(x, k, symm=symm))
