"""The row-shard layer (``dream_gnn_amd/shard.py``) inside zero tolerance, without a GPU: the designs of
``_shard_cases.py`` are exact in every summation order and hold what they claim; the cut rule restated as a plain loop
equals ``balanced_row_bounds`` / ``choose_row_bounds``; every rank of every world, built in one process on the
oracle-backed CPU backend, gives its rows of the float64 reference bit for bit (forward, transposed, dropped); and the
exchange — both forms, into a NaN-filled ``out``, through autograd, and the edge partition's all-reduce — does so over
gloo at world 3, 4 and 5, empty ranks included."""
import os
import socket
import sys

import numpy as np
import pytest
import torch

import _cpu_backend
import _shard_cases as SC
import _spmm_cases as C
from test_spmm_cases_host import _orders_agree

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CPU = torch.device("cpu")
NAMES = list(SC.DESIGNS)
F = 8


def _orders_agree_scaled(oracle, rows, cols, n_rows, w, gs, os_, gran, seed):
    """``_orders_agree`` for values ``gran * integer`` (the adjacency): the int64 sum in units of ``gran / 4``, the float64
    reference, the oracle's sequential fp32 / f64 sums and fp32 sums in 20 shuffled edge orders agree bit for bit."""
    X = C.features(int(cols.max()) + 1 if cols.size else 1, F, seed)
    ref = SC.product(rows, cols, n_rows, X, w, gs, None, gran=gran)
    wi = np.rint(w.astype(np.float64) / gran).astype(np.int64) * np.rint(4 * gs.astype(np.float64)[cols]).astype(np.int64)
    assert np.array_equal(wi * (gran / 4), w.astype(np.float64) * gs[cols])
    yi = np.zeros((n_rows, F), np.int64)
    np.add.at(yi, rows, X[cols].astype(np.int64) * wi[:, None])
    assert np.array_equal(ref.astype(np.float64) * (4 / gran), yi.astype(np.float64)) and np.abs(yi).max() > 0
    ip, ix, order = oracle.csr_from_coo(rows, cols, n_rows)
    assert np.array_equal(oracle.spmm_csr(ip, ix, w[order], X, gs, None, acc="f32"), ref)
    assert np.array_equal(oracle.spmm_csr(ip, ix, w[order], X, gs, os_, acc="f32"), SC.product(rows, cols, n_rows, X, w, gs, os_, gran=gran))
    terms = X[cols] * (w * gs[cols])[:, None]
    assert terms.dtype == np.float32
    rng = np.random.default_rng(seed)
    for _ in range(20):
        perm = rng.permutation(rows.size)
        y = np.zeros((n_rows, F), np.float32)
        np.add.at(y, rows[perm], terms[perm])
        assert np.array_equal(y, ref)


@pytest.mark.parametrize("name", NAMES)
def test_every_design_is_exact_forward_and_transposed(oracle, name):
    d = SC.design(name)
    o = SC.operands(d, F)
    if name.startswith("adjacency"):
        _orders_agree_scaled(oracle, d.dst, d.src, d.n_dst, d.vals, o.ss, o.ds, d.gran, 1)
        _orders_agree_scaled(oracle, d.src, d.dst, d.n_src, d.vals, o.ds, o.ss, d.gran, 2)
        return
    for i, (w, ss) in enumerate([(d.vals, o.ss), (None, o.ss), (d.vals, None)]):
        _orders_agree(oracle, d.dst, d.src, d.n_dst, d.n_src, w, ss, o.ds, None, 10 + i)
        # the transposed product: rows = sources, the gather-side scale is dst_scale (granularity 1/4)
        _orders_agree(oracle, d.src, d.dst, d.n_src, d.n_dst, w, None if ss is None else o.ds, o.ss, None, 20 + i)


def test_the_designs_hold_what_they_claim():
    from dream_gnn_amd.shard import balanced_row_bounds, choose_row_bounds

    for name in NAMES:  # a shuffled COO order: `vals[mine]` is a gather, not a prefix
        d = SC.design(name)
        assert d.dst.size < 2 or name == "one_row" or np.any(np.diff(d.dst) < 0), name
    # hub: rectangular, leading / trailing empty rows, duplicate pairs, a heavy row and a heavy column
    d = SC.design("hub")
    deg_in, deg_out = SC.degrees(d)
    assert (d.n_dst, d.n_src) == (41, 23) and deg_in[5] == 400 and deg_in[30] == 7 and deg_in[6:20].max() == 3
    assert not deg_in[:5].any() and not deg_in[20:30].any() and not deg_in[31:].any() and (deg_in[6:20] == 0).sum() == 3
    assert deg_out[SC.HUB_COL] >= 380 and np.unique(d.dst * 100 + d.src).size < d.dst.size
    assert SC.expected_bounds(deg_in, 2) == [0, 6, 41] and SC.expected_bounds(deg_in, 3) == [0, 6, 6, 41]
    assert SC.expected_bounds(deg_in, 8) == [0, 6, 6, 6, 6, 6, 6, 6, 41]
    assert SC.expected_bounds(deg_out, 2) == [0, 3, 23] and SC.expected_bounds(deg_out, 3) == [0, 3, 3, 23]
    for world in (3, 5, 8, 16):  # world 2 cannot hold an empty rank unless the LAST row is the hub: cut 1 is in [1, n - 1]
        for deg in (deg_in, deg_out):
            b = SC.expected_bounds(deg, world)
            rows = np.diff(b)
            nnz = np.array([deg[b[i]:b[i + 1]].sum() for i in range(world)])
            assert (rows == 0).any() and rows[0] > 0, (world, b)              # an empty rank; rank 0 holds the hub
            assert rows[-1] > rows[0] and 0 < nnz[-1] * 4 < nnz[0], (world, b)  # the last rank: most rows, few edges
    # even and its neighbours, by hand.  World 8: blocks of 8 rows x 32 edges = 256.  Two more edges in row 63: the block
    # holds 258 against (1 + 0.01) * 2050 / 8 = 258.8125 — inside (world 4: 514 against 517.625, world 2: 1026 against
    # 1035.25); with half the tolerance 1.005 * 256.25 = 257.53125 — outside.  Twenty-four more: 280 against
    # 1.01 * 2072 / 8 = 261.59; world 4: 536 against 1.01 * 518 = 523.18; world 2: 1048 against 1.01 * 1036 = 1046.36 —
    # outside at every world.  Outside, the nnz cut differs from equal rows (the extra edges sit in the last row).
    for world in (2, 4, 8):
        equal = [i * (64 // world) for i in range(world + 1)]
        for name, inside in (("even", True), ("even_plus2", True), ("even_plus24", False)):
            deg = SC.degrees(SC.design(name))[0]
            assert SC.equal_rows_condition(deg, world) == inside
            got = choose_row_bounds(torch.from_numpy(deg), world).tolist()
            assert (got == equal) == inside and got == SC.expected_choice(deg, world), (name, world, got)
    deg = SC.degrees(SC.design("even_plus2"))[0]
    assert deg[56:].sum() == 258 and deg.sum() == 2050 and 258 <= 1.01 * 2050 / 8 and not 258 <= 1.005 * 2050 / 8
    assert 514 <= 1.01 * 2050 / 4 and 1026 <= 1.01 * 2050 / 2
    assert not SC.equal_rows_condition(deg, 8, tol=0.005)
    assert choose_row_bounds(torch.from_numpy(deg), 8, tol=0.005).tolist() == SC.expected_bounds(deg, 8) != list(range(0, 65, 8))
    deg = SC.degrees(SC.design("even_plus24"))[0]
    assert deg[56:].sum() == 280 and deg[48:].sum() == 536 and deg[32:].sum() == 1048 and deg.sum() == 2072
    assert 280 > 1.01 * 2072 / 8 and 536 > 1.01 * 2072 / 4 and 1048 > 1.01 * 2072 / 2
    d = SC.design("even")
    assert set(SC.degrees(d)[0]) == {32} and set(SC.degrees(d)[1]) == {32}
    # stairs: the running sum hits 210 // 2 = 105 exactly at the end of row 13 / stands one edge short of it there
    hit, short, inside = (SC.degrees(SC.design("stairs_" + k))[0] for k in ("hit", "short", "inside"))
    assert hit.tolist() == list(range(1, 21)) and np.cumsum(hit)[13] == 105 and hit.sum() == 210
    assert np.cumsum(short)[13] == 104 and np.cumsum(short)[14] == 120 and short.sum() == 210
    assert balanced_row_bounds(torch.from_numpy(hit), 2).tolist() == [0, 14, 20]      # right=True would say 15
    assert balanced_row_bounds(torch.from_numpy(short), 2).tolist() == [0, 15, 20]
    sums = set(np.cumsum(inside).tolist())
    assert all(i * 190 // w not in sums for w in (2, 3, 5, 8) for i in range(1, w)) and inside.sum() == 190
    # adjacency: scale[row] * m forward, scale[source] * m as a graph of its own; every entry of M once
    a, at = SC.design("adjacency"), SC.design("adjacency_t")
    _, _, M = SC.MC.adjacency_edges(0)
    rs = M.sum(1)
    assert np.array_equal(a.vals.astype(np.float64) * rs[a.dst], M[a.dst, a.src]) and set(M[a.dst, a.src]) == {1, 2, 3}
    assert np.array_equal(at.vals.astype(np.float64) * rs[at.src], M[at.src, at.dst]) and a.dst.size == (M > 0).sum()
    assert np.all(np.frexp(rs.astype(np.float64))[0] == 0.5) and a.gran == 1 / 128
    assert SC.design("no_edges").dst.size == 0 and SC.design("one_row").n_dst == 1


def test_the_restated_cut_rule_equals_the_library():
    from dream_gnn_amd.shard import balanced_row_bounds, choose_row_bounds

    t = lambda deg: torch.as_tensor(np.asarray(deg, np.int64))
    # the four degenerate cases, by hand: no row -> every cut is its target, 0; no edge -> every target is 0, reached by
    # row 0, cut 1; one row -> it reaches every target, cut 1 = n; a hub in the middle reaches both targets (3 and 6)
    literal = [([], 4, [0, 0, 0, 0, 0]), ([0] * 5, 4, [0, 1, 1, 1, 5]), ([7], 4, [0, 1, 1, 1, 1]), ([0, 0, 9, 0, 0], 3, [0, 3, 3, 5])]
    for deg, parts, want in literal:
        assert SC.expected_bounds(deg, parts) == want
        assert balanced_row_bounds(t(deg), parts).tolist() == want and choose_row_bounds(t(deg), parts).tolist() == want
    cases = [(np.concatenate(SC.degrees(SC.design(n))[:1])) for n in NAMES] + [SC.degrees(SC.design(n))[1] for n in NAMES]
    rng = np.random.default_rng(8)
    for _ in range(200):
        n = int(rng.integers(1, 60))
        deg = rng.integers(0, 6, n) * (rng.random(n) < 0.6)
        for _ in range(int(rng.integers(0, 3))):
            deg[rng.integers(0, n)] = rng.integers(50, 2000)        # hubs
        if rng.random() < 0.3:
            deg[:] = rng.integers(1, 4)                               # uniform: the equal-rows branch where n % parts == 0
        cases.append(deg)
    taken = {True: 0, False: 0}
    for deg in cases:
        for parts in range(1, 18):
            want = SC.expected_bounds(deg, parts)
            assert balanced_row_bounds(t(deg), parts).tolist() == want, (deg, parts)
            assert want[0] == 0 and want[-1] == len(deg) and want == sorted(want) and len(want) == parts + 1
            cond = SC.equal_rows_condition(deg, parts)
            taken[cond] += 1
            got = choose_row_bounds(t(deg), parts).tolist()
            assert got == ([i * (len(deg) // parts) for i in range(parts + 1)] if cond else want), (deg, parts)
    assert taken[True] > 100 and taken[False] > 1000
    assert not SC.equal_rows_condition([1] * 10, 4) and not SC.equal_rows_condition([], 4) and not SC.equal_rows_condition([0] * 8, 4)


@pytest.mark.parametrize("name", NAMES)
def test_every_rank_of_every_world_forward(oracle, name):
    with _cpu_backend.patched():
        for world in SC.WORLDS_HOST:
            SC.check_forward(CPU, SC.design(name), world, F)


@pytest.mark.parametrize("name", NAMES)
def test_every_rank_of_every_world_backward(oracle, name):
    with _cpu_backend.patched():
        for world in SC.WORLDS_HOST:
            SC.check_backward(CPU, SC.design(name), world, F)


@pytest.mark.parametrize("name", NAMES)
def test_every_rank_of_every_world_dropped(oracle, name):
    with _cpu_backend.patched():
        for world in SC.WORLDS_HOST:
            SC.check_dropped(CPU, oracle, SC.design(name), world, F)


def test_shards_without_rows_and_without_edges_occur():
    """What the checks above run through: a rank with no row and a rank with rows but no edge, in ``fwd`` and ``bwd``."""
    d = SC.design("hub")
    deg_in, deg_out = SC.degrees(d)
    for deg in (deg_in, deg_out):
        b = SC.expected_bounds(deg, 5)
        assert any(b[i] == b[i + 1] for i in range(5))
    b = SC.expected_choice(SC.degrees(SC.design("no_edges"))[0], 3)
    assert b == [0, 1, 1, 9]  # rows without edges (ranks 0 and 2) and no rows (rank 1)


# ---------------------------------------------------------------------------------------------
# the exchange over gloo
# ---------------------------------------------------------------------------------------------
def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _worker(rank, world, port, names, q):
    sys.path.insert(0, ROOT)
    sys.path.insert(0, HERE)
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    import torch.distributed as dist

    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        import _cpu_backend as B
        import _shard_cases as S

        res = {}
        with B.patched():
            for name in names:
                res[name] = S.check_gather(torch.device("cpu"), S.design(name), F)
        q.put((rank, res))
    except Exception as exc:  # noqa: BLE001 - reported to the parent instead of a queue timeout
        q.put((rank, {"error": repr(exc)}))
    finally:
        dist.destroy_process_group()


def spawn_and_collect(target, world, args, timeout):
    """One spawn of ``world`` workers; one queue item per worker under a time limit, stragglers killed, exit codes kept."""
    import queue

    import torch.multiprocessing as mp

    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=target, args=(r, world, port) + tuple(args) + (q,)) for r in range(world)]
    for p in procs:
        p.start()
    res = []
    try:
        for _ in procs:
            try:
                res.append(q.get(timeout=timeout))
            except queue.Empty:
                break
        for p in procs:
            p.join(timeout=30 if len(res) == world else 0.1)
    finally:
        for p in procs:
            if p.is_alive():  # a collective that never returns must not outlive the test
                p.kill()
                p.join(timeout=30)
    return sorted(res, key=lambda r: r[0]), [p.exitcode for p in procs]


@pytest.mark.parametrize("world,names", [(3, ("hub",)), (5, ("hub",)), (4, ("even", "even_plus24"))],
                         ids=["world3-hub", "world5-hub", "world4-even"])
def test_the_exchange_over_gloo(oracle, world, names):
    """World 3 and 5 on ``hub``: empty ranks and uneven blocks — the padded all-gather and the direct form with empty
    blocks; world 4 on ``even`` (the unpadded all-gather) and its heavy neighbour (uneven, no empty rank)."""
    from dream_gnn_amd import shard

    for name in names:  # which all-gather each design takes
        b = SC.expected_choice(SC.degrees(SC.design(name))[0], world)
        assert (len(set(np.diff(b))) == 1) == (name == "even")
        assert (0 in np.diff(b)) == (name == "hub")
    assert shard.RowShard.exchange in ("allgather", "direct")
    res, codes = spawn_and_collect(_worker, world, (names,), timeout=120)
    assert [r for r, _ in res] == list(range(world)), (res, codes)
    assert codes == [0] * world, codes
    for rank, out in res:
        assert out == {name: True for name in names}, (rank, out)
