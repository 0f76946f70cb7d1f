"""The non-finite contract of `dgmi_knn_cosine_topk_f32` (include/dgmi.h) on the GPU, ZERO tolerance: lattice rows of
_knn_cases.py with chosen rows overwritten by NaN (_knn_nonfinite_cases.py: one element or all of them, six bit patterns),
on every path of the search — fp32 kernel + merge, rectangle, triangle, 256 x 256 tiles with two K chunks and with one,
the tile take-over and the exact-rows take-over — plus fewer finite rows than k, rows with +-Inf, the bindings, and
`graph.feature_similarity_graph` against the reference's own output (tests/golden/featgraph_*.npz).

Reference: integer similarity numerators over the FINITE columns only, evaluated on the device in float64 row blocks.
For every finite query, checks (a) of test_gpu_knn_exact.py: the first k_f = min(k, #finite rows) ids valid, finite rows
and distinct, similarities non-increasing and equal to the integer top-k_f, every candidate strictly above the k_f-th value
present; then k - k_f times -1.  A NaN row's list is k times -1.  Ties at the k-th value stay free.

Every table lies inside a buffer of the test's own, `ld = D + 8`, two guard rows before and two after it.  The guard rows
are MAGNETS: copies of finite rows, row -1 a copy of the first finite row (similarity 1 to it, and the lower id).  A kernel
that scores "row -1" — what the rescoring did with its dead slots when a query had fewer than k live entries — puts id -1
ahead of real neighbours and the checks above fail; nothing faults, because the row is this file's memory.  After the call
the whole buffer (guard rows, spare columns, the table), the 4 KiB behind the workspace and 64 elements on either side of
`nbr` still hold what they held.

What this file CANNOT see: a stray read on behalf of a query row that holds a NaN.  NaN times anything is NaN, so whatever
row such a query is scored against, its list comes out as k times -1.  For that case the fix rests on the reading of
`knn_rescore_kernel` (`keep_from` stops at -3, above the -4 of a dead slot: none is ever dereferenced), not on a test.  The
finite queries with fewer than k live entries take the same code and ARE seen by the magnets.

Rows with +-Inf and no NaN are held to address safety only: ids in [0, N) or -1, non-negative ids distinct, sentinels."""
import numpy as np
import pytest
import torch

import _knn_cases as K
import _knn_nonfinite_cases as NF

pytestmark = pytest.mark.gpu

GUARD = 2
NBR_PAD = 64
WS_MARGIN = 4096


class _Owned:
    """The table inside a buffer of the test's own, with magnets around it, and the buffers of one raw call."""

    def __init__(self, dev, case, k):
        N, D = case.x.shape
        self.N, self.D, self.k, self.ld = N, D, k, D + 8
        before, after = NF.magnets(case)
        buf = torch.full((N + 2 * GUARD, self.ld), NF.SENTINEL, dtype=torch.float32)
        buf[:GUARD, :D], buf[GUARD:GUARD + N, :D], buf[GUARD + N:, :D] = before, case.x, after
        self.buf = buf.to(dev)
        self.snap = self.buf.clone()
        self.view = self.buf[GUARD:GUARD + N, :D]
        assert self.view.stride() == (self.ld, 1) and torch.equal(self.view.view(torch.int32).cpu(), case.x.view(torch.int32))

    def run(self):
        from dream_gnn_amd import _lib

        L, N, D, k = _lib.lib, self.N, self.D, self.k
        assert L.dgmi_knn_cosine_supported(N, D, k) == 1
        self.wb = int(L.dgmi_knn_cosine_workspace_bytes(N, D, k))
        assert self.wb == K.workspace_bytes(N, D, k)
        self.ws = torch.full((self.wb + WS_MARGIN,), 0xA5, dtype=torch.uint8, device=self.buf.device)
        self.out = torch.full((N * k + 2 * NBR_PAD,), -7, dtype=torch.int32, device=self.buf.device)
        nbr = self.out[NBR_PAD:NBR_PAD + N * k].view(N, k)
        _lib.check(L.dgmi_knn_cosine_topk_f32(self.view.data_ptr(), self.ld, N, D, k, nbr.data_ptr(), self.ws.data_ptr(), self.wb,
                                              torch.cuda.current_stream().cuda_stream), "dgmi_knn_cosine_topk_f32")
        torch.cuda.synchronize()
        return nbr

    def sentinels_hold(self):
        assert torch.equal(self.buf.view(torch.int32), self.snap.view(torch.int32)), "the table's buffer was written"
        assert bool((self.ws[self.wb:] == 0xA5).all()), "written behind the workspace"
        assert bool((self.out[:NBR_PAD] == -7).all()) and bool((self.out[-NBR_PAD:] == -7).all()), "written beside nbr"

    def flags(self):
        L = K.screen_layout(self.N, self.D, self.k)
        return self.ws[L.flags:L.flags + 4 * self.N].view(torch.int32)

    def tau0_is_a_bound(self, case):
        """(b) of test_gpu_knn_exact.py with NaN rows in the sample: tau0 is a lattice value (or the -2 filler) at or below the
        k-th largest similarity over the FINITE rows — a NaN candidate lifts no threshold; a NaN query's sample is empty."""
        L = K.screen_layout(self.N, self.D, self.k)
        tau = self.ws[L.tau:L.tau + 4 * self.N].view(torch.float32)
        assert bool((tau[list(case.bad)] == -2.0).all())
        num = tau[self.q_finite].double() * case.lat.nz
        assert bool((num == num.round()).all())
        high = num > self.kth
        assert not bool(high.any()), "tau0 above the k-th value over the finite rows for %d queries, first %d: %g > %g" % (
            int(high.sum()), int(self.q_finite[high][0]), float(num[high][0]), float(self.kth[high][0]))


_xi = {}


def _numerators(dev, d):
    if id(d) not in _xi:
        _xi[id(d)] = (d, torch.from_numpy(d.num.astype(np.float64)).to(dev))
    return _xi[id(d)][1]


def _check(dev, case, k, nbr):
    """The contract for NaN rows, every query."""
    d = case.lat
    N = d.N
    fin = torch.from_numpy(case.finite).to(dev)
    n_fin = int(fin.sum())
    kf = min(k, n_fin)
    assert nbr.shape == (N, k) and nbr.dtype == torch.int32
    nb = nbr.long()
    assert bool((nb[~fin] == -1).all()), "a NaN row's list is not k times -1: %s" % nb[~fin][(nb[~fin] != -1).any(1)][:1].tolist()
    assert bool((nb[fin][:, kf:] == -1).all()), "filler other than -1"
    head = nb[:, :kf]
    # ids first: nothing is gathered with an id that was not checked
    hf = head[fin]
    assert int(hf.min()) >= 0 and int(hf.max()) < N, "ids out of range in a finite row's first %d: min %d max %d" % (
        kf, int(hf.min()), int(hf.max()))
    assert bool(fin[hf].all()), "a NaN row is in %d lists" % int((~fin[hf]).any(1).sum())
    srt = hf.sort(dim=1).values
    assert bool((srt[:, 1:] != srt[:, :-1]).all()), "duplicate ids"
    xi = _numerators(dev, d)
    q_all = fin.nonzero().reshape(-1)
    kth_all = torch.empty(q_all.numel(), dtype=torch.float64, device=dev)
    B = max(1, (1 << 26) // N)
    for lo in range(0, q_all.numel(), B):
        q = q_all[lo:lo + B]
        S = xi[q] @ xi.t()                                    # float64, integer-valued, exact
        S[:, ~fin] = -1e6                                     # comparable with nothing
        want = torch.topk(S, kf, dim=1).values
        got = torch.gather(S, 1, head[q])
        bad = (got != want).any(dim=1)
        assert not bool(bad.any()), "similarities differ from the integer top-k over the finite rows in %d lists, first query %d: got %s (ids %s) want %s" % (
            int(bad.sum()), int(q[bad][0]), got[bad][0].tolist(), head[q][bad][0].tolist(), want[bad][0].tolist())
        assert bool((got[:, 1:] <= got[:, :-1]).all())
        kth = want[:, kf - 1:kf]
        assert torch.equal((got > kth).sum(dim=1), (S > kth).sum(dim=1))
        kth_all[lo:lo + B] = kth[:, 0]
        del S
    return q_all, kth_all


def _run_nan(dev, N, D, k, case=None):
    case = NF.nan_case(N, D) if case is None else case
    o = _Owned(dev, case, k)
    nbr = o.run()
    o.sentinels_hold()
    o.q_finite, o.kth = _check(dev, case, k, nbr)
    return case, o, nbr


@pytest.mark.parametrize("N,D,k", NF.SMALL_SHAPES, ids=str)
def test_nan_rows_fp32_kernel_and_merge(dev, N, D, k):
    """Below 1 536 rows: 6 candidate splits at 763 rows, 11 with an empty one at 1 500, one split and k = 16 of 33 rows."""
    assert N < K.SCREEN_MIN_ROWS
    _run_nan(dev, N, D, k)


@pytest.mark.parametrize("N,D,k", NF.RECT_SHAPES + NF.TRI_SHAPES + NF.BIG_SHAPES, ids=str)
def test_nan_rows_screen(dev, N, D, k):
    """The bf16 screen: rectangle (k = 4: 16 slots per lane, one entry after the other; k = 13: 32; k = 40: the batched
    rescoring), the triangular sweep with NaN rows on both sides of the diagonal, 256 x 256 tiles through the LDS-DMA kernel
    with its pool and through the register-staged kernel (one K chunk).  At k <= 8 every finite row of the 300 copies is
    flagged (cap 128), so the tile take-over recomputes 32-query tiles that hold a NaN row next to flagged finite ones."""
    L = K.screen_layout(N, D, k)
    assert L.big == ((N, D, k) in NF.BIG_SHAPES) and L.sym == ((N, D, k) in NF.TRI_SHAPES + NF.BIG_SHAPES)
    case, o, nbr = _run_nan(dev, N, D, k)
    o.tau0_is_a_bound(case)
    flags = o.flags()
    assert bool(((flags == 0) | (flags == 1)).all())
    if not (L.big and D > 64):                                 # (the LDS-DMA kernel marks eight rows at a time when a list is full)
        assert not bool(flags[list(case.bad)].any())           # a NaN query is offered nothing: never flagged
    if k <= 8:
        r = NF.placement(case.lat)["block"][0]
        mates = [q for q in range(r // 32 * 32, r // 32 * 32 + 32) if case.finite[q]]
        assert bool(flags[mates].any()), "no flagged finite row in the 32-query tile of NaN row %d" % r


def test_nan_rows_exact_rows_take_over(dev):
    """k = 64 at 40 997 rows: the rows of the block's first tile find the 300 copies in one region of 256 slots and go
    to `knn_exact_rows_kernel`, which scores EVERY candidate, the NaN rows included, through `wave_topk_insert`."""
    N, D, k = NF.EXACT_ROWS_SHAPE
    case, o, nbr = _run_nan(dev, N, D, k)
    o.tau0_is_a_bound(case)
    flags = o.flags()
    lo, _ = case.lat.block
    first_tile = [q for q in range(lo, (lo // 128 + 1) * 128) if case.finite[q]]
    assert NF.placement(case.lat)["block"][0] // 128 == lo // 128 and bool(flags[first_tile].all())
    assert not bool(flags[list(case.bad)].any())


@pytest.mark.parametrize("few", [NF.FEW_33, NF.FEW_1536], ids=["33", "1536"])
def test_fewer_finite_rows_than_k(dev, few):
    """13 finite rows of 33 at k = 16 (fp32 kernel), 6 of 1 536 at k = 13 (screen: every query's buffer holds fewer than k
    entries, the NaN queries' none).  The finite ids in order, then -1 — with the magnets in front of and behind the table."""
    N, D, k, keep = few
    case = NF.few_case(N, D, k, keep)
    _, o, nbr = _run_nan(dev, N, D, k, case)
    want = torch.from_numpy(NF.expected_lists(case, k))
    got = nbr.long().cpu()
    n = len(keep)
    assert torch.equal(got[:, n:], want[:, n:]) and bool((got[:, n:] == -1).all())
    # in order: where the similarities of a row are all different the ids are those of the host, one for one
    S = K.similarity_numerators(case.lat.num, list(keep))[:, list(keep)]
    for i, q in enumerate(keep):
        if len(set(S[i].tolist())) == n:
            assert got[q].tolist() == want[q].tolist(), q
    if N >= K.SCREEN_MIN_ROWS:
        assert not bool(o.flags().any())


@pytest.mark.parametrize("N,D,k", NF.INF_SHAPES, ids=str)
def test_inf_rows_address_safety(dev, N, D, k):
    """+-Inf elements, no NaN in the table: scores of +Inf, -Inf and NaN.  Address safety only; order unspecified."""
    case = NF.inf_case(N, D)
    o = _Owned(dev, case, k)
    nbr = o.run()
    o.sentinels_hold()
    nb = nbr.long()
    assert int(nb.min()) >= -1 and int(nb.max()) < N
    srt = torch.where(nb >= 0, nb, torch.arange(-k, 0, device=dev)[None, :].expand_as(nb)).sort(dim=1).values
    assert bool((srt[:, 1:] != srt[:, :-1]).all()), "duplicate non-negative ids"


# ---------------------------------------------------------------------------------------------------------------------
def test_ops_binding_gives_the_bits_of_the_raw_call(dev):
    from dream_gnn_amd import ops

    for N, D, k in (NF.SMALL_SHAPES[0], NF.RECT_SHAPES[2]):
        case, o, nbr = _run_nan(dev, N, D, k)
        assert torch.equal(ops.knn_cosine_topk(o.view, k), nbr)
        assert torch.equal(ops.knn_cosine_topk(case.x.to(dev), k), nbr)
        o.sentinels_hold()


@pytest.mark.parametrize("bad", [float("nan"), float("inf")], ids=["nan", "inf"])
def test_builder_refuses_non_finite_features_on_the_device(dev, monkeypatch, bad):
    from dream_gnn_amd import graph as G, ops

    counter = NF.Counting(ops._T)
    monkeypatch.setattr(ops, "_T", counter)
    N, D, k = 2048 + 37, 256, 4
    x = (K.lattice(N, D).x * 4.0).to(dev)
    good = x.clone()
    x[[5, 700, N - 1], [0, 9, D - 1]] = bad
    for fused in (None, True, False):
        with pytest.raises(ValueError, match="3 of %d feature rows" % N):
            G.feature_similarity_graph(x, k, fused=fused)
    assert counter.calls == 0
    a = G.feature_similarity_graph(good, k, fused=True)       # zero rows (ids 9, 10, ...) are accepted
    assert counter.calls == 1 and not bool(good[9].any())
    assert bool(torch.isfinite(a.coalesce().values()).all())


@pytest.mark.parametrize("fused", [None, True], ids=["fused=None", "fused=True"])
@pytest.mark.parametrize("name", NF.FEATGRAPH)
def test_feature_graph_equals_the_reference(dev, monkeypatch, name, fused):
    """`graph.feature_similarity_graph` on the device == the tensor the reference's `_create_feature_similarity_graph`
    returned for the same features: same indices, bit-equal fp32 values.  Every fixture shape fits the kernel, so both
    settings run it (asserted)."""
    from dream_gnn_amd import graph as G, ops

    counter = NF.Counting(ops._T)
    monkeypatch.setattr(ops, "_T", counter)
    seen = []

    def build(x, k, symm):
        n, D = x.shape
        before = counter.calls
        out = G.feature_similarity_graph(x.to(dev), k, symm=symm, fused=fused)
        seen.append((counter.calls - before, ops.knn_cosine_supported(n, D, min(k, n - 1))))
        return out

    NF.compare_with_fixture(name, build)
    assert seen and all(calls == (1 if ok else 0) for calls, ok in seen)
    assert fused is None or all(ok for _, ok in seen)
