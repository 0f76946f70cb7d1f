"""The owned form WITHOUT a toucher (csrc/dgmi_owned_kernel.h ``DUTY``: sixteen worker waves, the touching of boundaries
and ids a duty of task slots) against the form with one: the same products BIT FOR BIT on the same layout — ``torch.equal``
on the ``int32`` view, NaN payloads and signed zeros included.  A duty only reads, ahead of time, words the workers read
anyway; nothing of a sum may depend on it.

Both forms are forced through ``set_tuning`` (``sliced_owned = 1``; ``sliced_owned_duty`` = 1 / 0) as in
test_gpu_spmm_owned_slices.py, on a graph of 3001 rows over 2500 sources and about 55 000 edges made here: degrees
0 .. 40, multiplicities 1 .. 8, and a run of five rows without edges every 35 rows — so that, whatever the task
geometry, lane groups' runs start and end with empty rows and the hand-over of the gather window starts cold — on layouts
of 8 and of 16 slices.  The settings cross lane-group widths 16 and 32 (two and one column round at F = 128; F = 100
leaves lanes idle), one and two row rounds (``sliced_owned_lds_rows``), grids whose last workgroup is short (7, 19), one
with a workgroup that owns no row (60 workgroups of 51 rows: 59 active), a workgroup with FEWER task slots than a duty
chunk (7 slots, chunks of 8: every duty touches past the phase's last task), one with exactly ``lead`` = 16 slots, duty
chunks of 1, 4 and a whole phase, leads of one chunk (the knob's 0: the built-in; a lead of NO slots is walked on the
host only, test_owned_duty_host.py) and of more than a phase, and one worker wave that takes every task and every duty.
What a bitwise comparison cannot see is whether a duty touches anything at all — a prefetch changes no result: that the
duty kernel runs is the routing test below, and which words a duty reads is the host walk.  Unit values and multiplicities, the plain and the SCALED kernel (scale codes in the id words), ``dst_scale`` and
the epilogue.  One case meets the float64 oracle under the suite's elementwise rule."""
import itertools
from collections import namedtuple

import numpy as np
import pytest
import torch

import _spmm_cases as C
from test_gpu_spmm_owned_scale import _plain, _scaled, _scales
from test_gpu_spmm_owned_slices import KNOBS as _SLICE_KNOBS, _cap, _kernels, _t

pytestmark = pytest.mark.gpu

KNOBS = dict(_SLICE_KNOBS, sliced_owned_scaled=-1, sliced_owned_duty=-1, sliced_owned_duty_chunk=0, sliced_owned_duty_lead=0)
N_DST, N_SRC = 3001, 2500
CHUNK, LEAD = 8, 16  # the chunk and lead of the two settings that say so (the built-in: a duty per phase, a phase ahead)

Graph = namedtuple("Graph", "dst src mult ds")


@pytest.fixture(autouse=True)
def _knobs_back_to_default():
    from dream_gnn_amd import _lib

    try:
        yield
    finally:
        for name, value in KNOBS.items():
            _lib.set_tuning(name, value)


def _set(**knobs):
    from dream_gnn_amd import _lib

    for name, value in dict(KNOBS, **knobs).items():
        _lib.set_tuning(name, value)


def _bits(t):
    return t.contiguous().view(torch.int32)


_made = {}


def graph():
    if "g" not in _made:
        rng = np.random.default_rng(3001)
        deg = rng.integers(0, 41, N_DST)
        deg[(np.arange(N_DST) // 5) % 7 == 0] = 0  # rows 0..4, 35..39, ...: empty, also the first rows of every workgroup of 35 k rows
        deg[-3:] = 0
        dst = np.repeat(np.arange(N_DST), deg)
        src = rng.integers(0, N_SRC, dst.size)
        src[:2] = (0, N_SRC - 1)
        order = rng.permutation(dst.size)
        g = Graph(dst[order].astype(np.int32), src[order].astype(np.int32), rng.integers(1, 9, dst.size).astype(np.int32),
                  rng.uniform(0.5, 1.5, N_DST).astype(np.float32))
        assert 40_000 < dst.size < 300_000
        for a in g:
            a.setflags(write=False)
        _made["g"] = g
    return _made["g"]


def _stage(dev, n_slices):
    from dream_gnn_amd import ops

    if n_slices not in _made:
        g = graph()
        sl = ops.SlicedCSR(_t(g.dst, dev), _t(g.src, dev), N_DST, N_SRC, n_slices=n_slices)
        assert int(sl.range_flag) == 0 and sl.n_slices == n_slices
        ids = (sl.indices | ((_t(g.mult, dev) - 1)[sl.eid.long()] << ops.MULT_SHIFT)).contiguous()
        _made[n_slices] = dict(sl=sl, ids=ids, ds=_t(g.ds, dev))
    return _made[n_slices]


def _tasks(grid, lpr, R, cap=0):
    """Task slots per phase of a full workgroup (owned_plan's arithmetic with a forced R)."""
    B = -(-N_DST // grid)
    fit = (144 << 10) // (16 * lpr)
    fit = min(fit, cap) if cap > 0 else fit
    round_rows = -(-B // -(-B // fit))
    return -(-round_rows // ((64 // lpr) * R))


def settings():
    two = lambda grid: _cap(N_DST, grid, 2)
    out = [
        dict(sliced_lpr=32, sliced_owned_grid=7),                                       # built-in R, a short last workgroup (429 rows: two row rounds)
        dict(sliced_lpr=16, sliced_owned_grid=7),                                       # two column rounds
        dict(sliced_lpr=32, sliced_owned_grid=19, sliced_owned_lds_rows=two(19)),       # two row rounds by the cap
        dict(sliced_lpr=16, sliced_owned_grid=19, sliced_owned_lds_rows=two(19), sliced_owned_rows=3),  # two and two
        dict(sliced_lpr=32, sliced_owned_grid=60, sliced_owned_rows=4, sliced_owned_duty_chunk=CHUNK, sliced_owned_duty_lead=LEAD),  # 7 slots < a chunk; a workgroup without rows
        dict(sliced_lpr=32, sliced_owned_grid=60, sliced_owned_rows=4),                 # the same with the built-in chunk
        dict(sliced_lpr=32, sliced_owned_grid=7, sliced_owned_rows=7, sliced_owned_duty_chunk=CHUNK, sliced_owned_duty_lead=LEAD),  # exactly `lead` = 16 slots
        dict(sliced_lpr=32, sliced_owned_grid=19, sliced_owned_rows=2, sliced_owned_duty_chunk=4, sliced_owned_duty_lead=8),
        dict(sliced_lpr=16, sliced_owned_grid=7, sliced_owned_rows=2, sliced_owned_duty_chunk=1, sliced_owned_duty_lead=0),
        dict(sliced_lpr=32, sliced_owned_grid=19, sliced_owned_rows=1, sliced_owned_duty_chunk=79, sliced_owned_duty_lead=79),  # a phase per duty
        dict(sliced_lpr=32, sliced_owned_grid=7, sliced_owned_rows=5, sliced_owned_duty_lead=500),  # a lead of many phases
        dict(sliced_lpr=32, sliced_owned_grid=3, sliced_owned_workers=1),               # one wave: every task, every duty
        dict(sliced_lpr=16, sliced_owned_grid=19, sliced_owned_workers=16),             # (16 = all of the duty form's, 15 of the toucher form's)
    ]
    return out


def test_settings_are_what_they_claim():
    assert -(-N_DST // 60) == 51 and -(-N_DST // 51) == 59  # 60 workgroups, 59 with rows
    assert N_DST % 429 != 0 and N_DST - 6 * 429 == 427       # grid 7: a short last workgroup
    assert _tasks(60, 32, 4) == 7 < CHUNK
    assert _tasks(7, 32, 7) == LEAD and -(-min(427, 215) // 14) == LEAD  # (the short last workgroup too)
    assert _tasks(19, 32, 1) == 79
    g = graph()
    deg = np.bincount(g.dst, minlength=N_DST)
    assert np.all(deg[:5] == 0) and np.all(deg[-3:] == 0) and deg[5:35].max() > 0
    for B in (429, 158, 51):  # every workgroup's first or last rows meet an empty run somewhere
        assert any(deg[w * B] == 0 for w in range(N_DST // B)) and any(deg[min(N_DST, (w + 1) * B) - 1] == 0 for w in range(-(-N_DST // B)))


def test_duty_form_launches_its_kernel_and_only_where_built(dev):
    """``sliced_owned_duty = 1``: ``spmm_owned_duty_kernel`` at 16- and 32-lane groups, plain and scaled; the toucher form's
    kernel at the widths the duty form is not built for, with 64-bit offsets, under a gate and in the two-workgroup
    form, and for ``sliced_owned_duty`` = 0 and the built-in rule on a product this small."""
    from dream_gnn_amd import ops

    st = _stage(dev, 8)
    sl = st["sl"]
    X = torch.randn(N_SRC, 128, generator=torch.Generator(device="cpu").manual_seed(1)).to(dev)
    table, words = ops.CSRGraph.scale_codes(_t(_scales(N_SRC, "37", 1), dev), sl.indices)
    for lpr in (16, 32):
        _set(sliced_owned=1, sliced_owned_duty=1, sliced_owned_grid=7, sliced_lpr=lpr)
        names = _kernels(lambda: _plain(sl, sl.indices, False, X))
        assert "spmm_owned_duty_kernel" in names and "spmm_owned_kernel" not in names, names
        names = _kernels(lambda: _scaled(sl, words, table, False, X))
        assert "spmm_owned_duty_kernel" in names and "spmm_owned_scaled_kernel" not in names, names
    for knobs in (dict(sliced_lpr=8), dict(sliced_lpr=64), dict(sliced_no_off32=1), dict(sliced_owned_lag=0), dict(sliced_owned_wgs=2),
                  dict(sliced_owned_duty=0), dict(sliced_owned_duty=-1)):
        _set(**dict(dict(sliced_owned=1, sliced_owned_duty=1, sliced_owned_grid=7), **knobs))
        names = _kernels(lambda: _plain(sl, sl.indices, False, X))
        assert "spmm_owned_kernel" in names and "spmm_owned_duty_kernel" not in names, (knobs, names)
    _set(sliced_owned=1, sliced_owned_duty=-1, sliced_owned_grid=7, sliced_lpr=32)
    names = _kernels(lambda: _scaled(sl, words, table, False, X))
    assert "spmm_owned_scaled_kernel" in names and "spmm_owned_duty_kernel" not in names, names


@pytest.mark.parametrize("scaled", [False, True], ids=["plain", "scaled"])
@pytest.mark.parametrize("kind", ["unit", "mult"])
@pytest.mark.parametrize("n_slices", [8, 16])
def test_duty_form_is_bitwise_the_toucher_form(dev, n_slices, kind, scaled):
    from dream_gnn_amd import ops

    st = _stage(dev, n_slices)
    sl, id_mult = st["sl"], kind == "mult"
    ids = st["ids"] if id_mult else sl.indices
    gen = torch.Generator(device="cpu").manual_seed(100 * n_slices + 10 * id_mult + scaled)
    mask = {F: _t(C.out_mask(N_DST, F, 3), dev) for F in (128, 100)}
    X = {F: torch.randn(N_SRC, F, generator=gen).to(dev) for F in (128, 100)}
    if scaled:  # +-0 and a NaN with a payload among the scales: a mangled sign or payload shows
        table, words = ops.CSRGraph.scale_codes(_t(_scales(N_SRC, "nan", 9), dev), ids)
        run = lambda F, ds, m: _scaled(sl, words, table, id_mult, X[F], ds, m)
    else:
        X[128][7, 5], X[128][N_SRC - 1, 127] = float("inf"), -0.0
        run = lambda F, ds, m: _plain(sl, ids, id_mult, X[F], ds, m)
    for i, knobs in enumerate(settings()):
        F = 100 if i % 4 == 1 else 128
        for has_ds, epi in ((False, False), (True, True)) if i % 2 else ((True, False), (False, True)):
            args = (F, st["ds"] if has_ds else None, mask[F] if epi else None)
            _set(sliced_owned=1, sliced_owned_duty=0, **knobs)
            want = run(*args)
            _set(sliced_owned=1, sliced_owned_duty=1, **knobs)
            got = run(*args)
            assert want is not None and got is not None, knobs
            if scaled and not (has_ds or epi):
                assert bool(torch.isnan(want).any())
            rows = (_bits(got) != _bits(want)).any(1).nonzero().flatten().tolist()
            assert not rows, "%d slices %s %s F=%d ds=%s epi=%s: %d rows differ, first %s" % (
                n_slices, kind, knobs, F, has_ds, epi, len(rows), rows[:8])


def test_duty_form_meets_the_float64_oracle(oracle, dev):
    """Multiplicities, a source scale (coded) and ``dst_scale`` through the scaled duty kernel, two row rounds: the suite's
    elementwise rule, ``|y - y64| <= 1e-5 * sum |terms|`` for every element and ``<= 1e-5 * max |y64|``."""
    from dream_gnn_amd import ops

    g, st = graph(), _stage(dev, 8)
    rng = np.random.default_rng(5)
    Xn = rng.standard_normal((N_SRC, 128)).astype(np.float32)
    ss = rng.choice(np.linspace(0.5, 1.5, 300), N_SRC).astype(np.float32)
    table, words = ops.CSRGraph.scale_codes(_t(ss, dev), st["ids"])
    _set(sliced_owned=1, sliced_owned_duty=1, sliced_lpr=32, sliced_owned_grid=7, sliced_owned_lds_rows=_cap(N_DST, 7, 2))
    got = _scaled(st["sl"], words, table, True, _t(Xn, dev), st["ds"])
    assert got is not None
    ip, ix, e0 = oracle.csr_from_coo(g.dst, g.src, N_DST)
    vals = g.mult[e0].astype(np.float32)
    y64 = oracle.spmm_csr(ip, ix, vals, Xn, ss, g.ds, acc="f64")
    yabs = oracle.spmm_csr(ip, ix, vals, Xn, ss, g.ds, acc="abs")
    err = np.abs(got.cpu().numpy().astype(np.float64) - y64)
    assert np.all(err <= 1e-5 * yabs + 1e-30) and err.max() <= 1e-5 * np.abs(y64).max()
