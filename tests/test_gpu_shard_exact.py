"""The row-shard layer (``dream_gnn_amd/shard.py``) on the device at ZERO tolerance: every rank of world 1, 2, 3, 5 and
8 of every design of ``_shard_cases.py`` — built in one process, ``RowShard`` / ``ShardedRelation(rank=r, world=W)`` need
no process group — gives its rows of the float64 reference bit for bit: forward (allocating, and into the middle rows
of a NaN-filled buffer), the ``bwd`` shard of the reversed edges, the dropped views of bench.py's dropout step (forward
and ``spmm_t``), under the planned kernels, the XCD-local kernels (compacted and on the fly) and the workgroup-owned
form; ranks without rows and ranks with rows but no edge included.  One multi-process case runs the exchange itself —
both forms, ``out=`` given and not, autograd — between four ranks that share the GPU over gloo.  The same assertions run
on the host in test_shard_cases_host.py.  Every comparison is ``torch.equal``."""
import os
import sys

import pytest
import torch

import _shard_cases as SC
from test_shard_cases_host import spawn_and_collect

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
pytestmark = pytest.mark.gpu

NAMES = list(SC.DESIGNS)
ROUTES = {"default": (None, True, -1), "sliced-compact": ("sliced", True, -1), "sliced-onthefly": ("sliced", False, -1),
          "sliced-owned": ("sliced", True, 1)}   # ops.FORCE_KERNEL, ops.COMPACT_DROPPED, the sliced_owned knob
WIDTHS = {"default": (4, 128, 6), "sliced-compact": (4, 128, 6), "sliced-onthefly": (4, 128), "sliced-owned": (4, 128)}
CASES = [(route, F) for route in ROUTES for F in WIDTHS[route]]   # F = 6: no multiple of 4 (the dword kernel; never sliced)


@pytest.fixture(autouse=True)
def _knobs_back_to_default():
    from dream_gnn_amd import _lib, ops, shard

    saved = (ops.FORCE_KERNEL, ops.COMPACT_DROPPED, ops.MULT_FORM, shard.RowShard.exchange)
    try:
        yield
    finally:
        ops.FORCE_KERNEL, ops.COMPACT_DROPPED, ops.MULT_FORM, shard.RowShard.exchange = saved
        _lib.set_tuning("sliced_owned", -1)


def _set_route(route):
    from dream_gnn_amd import _lib, ops

    force, compact, owned = ROUTES[route]
    ops.FORCE_KERNEL, ops.COMPACT_DROPPED = force, compact
    _lib.set_tuning("sliced_owned", owned)
    return force, compact


def _route_hook(route, seen):
    """The route was taken: a knob that silently falls back proves nothing."""
    force, compact, _ = ROUTES[route]

    def hook(what, g, F):
        sliced = force == "sliced" and F % 4 == 0
        assert (g._sliced is not None) == sliced, (route, what, F)
        if what == "dropped":
            assert g._keep is not None and (g._sliced_t is not None) == sliced
            assert ("sliced" in g._c and "sliced_t" in g._c) == (sliced and compact) and set(g._c) <= {"sliced", "sliced_t"}
        seen.add((what, sliced, g.n_dst == 0, g.nnz == 0))

    return hook


@pytest.mark.parametrize("route,F", CASES, ids=["%s-F%d" % c for c in CASES])
def test_every_rank_of_every_world_gives_its_rows_of_the_reference(oracle, dev, route, F):
    """``check_forward``, ``check_backward`` and ``check_dropped`` of every design at world 1, 2, 3, 5 and 8."""
    _set_route(route)
    seen = set()
    hook = _route_hook(route, seen)
    for name in NAMES:
        d = SC.design(name)
        for world in SC.WORLDS_GPU:
            SC.check_forward(dev, d, world, F, hook=hook)
            SC.check_backward(dev, d, world, F, hook=hook)
            SC.check_dropped(dev, oracle, d, world, F, hook=hook)
    sliced = ROUTES[route][0] == "sliced" and F % 4 == 0
    # a rank without rows and a rank with rows but no edge went through the route, plain and dropped
    assert {(w, sliced, True, True) for w in ("forward", "dropped")} <= seen
    assert {(w, sliced, False, True) for w in ("forward", "dropped")} <= seen


@pytest.mark.parametrize("name", NAMES)
def test_the_concatenated_ranks_equal_the_unsharded_library(dev, name):
    SC.check_unsharded(dev, SC.design(name), 5, 128)
    SC.check_unsharded(dev, SC.design(name), 8, 6)


MULT_EXPECTED = {("adjacency", "fwd"): {"row"}, ("adjacency", "bwd"): {"col"},
                 ("adjacency_t", "fwd"): {"col"}, ("adjacency_t", "bwd"): {"row"}}


def test_the_multiplicity_form_of_adjacency_shards(dev):
    """``MULT_FORM`` on, the XCD-local route: a row shard of ``D^-1 M`` holds complete rows (values ``scale[row] * m``); a
    row shard of its transpose, and every ``bwd`` shard, sees only part of each column, so ``_mult_form`` may find another
    (scale, multiplicity) split or none — the product (``check_backward``) is exact either way.  What the detection
    returns per design and orientation is pinned here and stated in tests/README.md."""
    from dream_gnn_amd import ops, shard

    ops.FORCE_KERNEL, ops.MULT_FORM = "sliced", True
    seen = {}
    for name in ("adjacency", "adjacency_t"):
        d = SC.design(name)
        dst, src, vals = SC._coo(d, dev)
        for world in SC.WORLDS_GPU:
            SC.check_backward(dev, d, world, 128)
            for r in range(world):
                rel = shard.ShardedRelation(dst, src, d.n_dst, d.n_src, vals=vals, rank=r, world=world)
                for orient, sh in (("fwd", rel.fwd), ("bwd", rel.bwd)):
                    mf = sh.local._mult_form()
                    assert mf is None or (mf[0] in ("row", "col") and int(mf[2].min()) >= 0 and int(mf[2].max()) <= 7)
                    seen.setdefault((name, orient), set()).add(None if mf is None else mf[0])
    assert seen == MULT_EXPECTED, seen
    ops.MULT_FORM = False
    d = SC.design("adjacency")
    dst, src, vals = SC._coo(d, dev)
    rel = shard.ShardedRelation(dst, src, d.n_dst, d.n_src, vals=vals, rank=1, world=3)
    assert rel.fwd.local._mult_form() is None and rel.bwd.local._mult_form() is None
    SC.check_backward(dev, d, 3, 128)


# ---------------------------------------------------------------------------------------------
# the exchange between four ranks that share the GPU (gloo, staged through the host)
# ---------------------------------------------------------------------------------------------
GATHER_WORLD, GATHER_DESIGNS, GATHER_F = 4, ("hub", "even"), 128


def _worker(rank, world, port, q):
    sys.path.insert(0, ROOT)
    sys.path.insert(0, HERE)
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    import torch.distributed as dist

    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        import _shard_cases as S

        out = {}
        S.check_forward(dev, S.design("stairs_hit"), 2, 4)  # ordinary products on a small graph first
        for name in GATHER_DESIGNS:
            out[name] = S.check_gather(dev, S.design(name), GATHER_F, edge_shard=False)  # no device all-reduce on gloo
        torch.cuda.synchronize()
        q.put((rank, out))
    except Exception as exc:  # noqa: BLE001 - reported to the parent instead of a queue timeout
        q.put((rank, {"error": repr(exc)}))
    finally:
        dist.destroy_process_group()


def test_the_exchange_between_four_ranks_on_one_gpu():
    """World 4 on ``hub`` ([0, 6, 6, 6, 41]: two ranks without rows, uneven blocks — the padded all-gather and the direct
    form with empty blocks) and on ``even`` (the unpadded all-gather), F = 128: ``gather_rows`` in both forms, allocating
    and into a NaN-filled ``out``, and ``rel(X, ss, ds)`` with its backward, equal to the references on every rank."""
    import numpy as np

    hub = SC.expected_choice(SC.degrees(SC.design("hub"))[0], GATHER_WORLD)
    assert hub == [0, 6, 6, 6, 41] and SC.expected_choice(SC.degrees(SC.design("even"))[0], GATHER_WORLD) == [0, 16, 32, 48, 64]
    assert len(set(np.diff(hub))) > 1
    res, codes = spawn_and_collect(_worker, GATHER_WORLD, (), timeout=180)
    assert [r for r, _ in res] == list(range(GATHER_WORLD)), (res, codes)
    assert codes == [0] * GATHER_WORLD, codes
    for rank, out in res:
        assert out == {name: True for name in GATHER_DESIGNS}, (rank, out)
