"""Pairs at or above a cut and the deep top-k, host side (no GPU): include/dgmi_above.h declares exactly the new entry
points, the library exports them and the fourth ctypes table matches; argument validation and workspace sizing return
codes before any launch; both torch ops are registered and refuse CPU tensors; ops / MLPDecoder / predict refuse a bad
cut, max_pairs, k and known before touching the device."""
import math
import os
import re

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY_POINTS = ["dgmi_pair_emit_workspace_bytes", "dgmi_pair_mlp_emit_f32", "dgmi_pair_records_sort_f32",
                "dgmi_pair_records_sort_workspace_bytes"]
MAX_RECORDS = 1 << 24


def _text():
    return open(os.path.join(ROOT, "include", "dgmi_above.h")).read()


def _prototypes():
    """name -> parameter list of every DGMI_API prototype of the header"""
    return {m.group(1): m.group(2) for m in re.finditer(r"DGMI_API\s+[\w\s\*]+?\b(dgmi_\w+)\s*\(([^)]*)\)\s*;", _text())}


def test_header_declares_the_above_entry_points():
    assert sorted(_prototypes()) == ENTRY_POINTS
    assert '#include "dgmi.h"' in _text() and "#define DGMI_PAIR_EMIT_MAX_RECORDS (1 << 24)" in _text()


def test_the_other_headers_do_not_declare_them():
    for name in ("dgmi.h", "dgmi_pairs.h", "dgmi_rank.h"):
        text = open(os.path.join(ROOT, "include", name)).read()
        assert not any(e in text for e in ENTRY_POINTS), name


def test_library_exports_the_above_entry_points():
    from dream_gnn_amd import _lib

    assert sorted(_lib.ABOVE_SIGNATURES) == ENTRY_POINTS
    for other in (_lib.SIGNATURES, _lib.PAIR_SIGNATURES, _lib.RANK_SIGNATURES):
        assert not set(_lib.ABOVE_SIGNATURES) & set(other)
    assert _lib.PAIR_EMIT_MAX_RECORDS == MAX_RECORDS
    protos = _prototypes()
    ctype_of = {"int64_t": "c_long", "int32_t": "c_int", "float": "c_float", "size_t": "c_ulong", "dgmi_stream_t": "c_void_p"}
    for name, (res, args) in _lib.ABOVE_SIGNATURES.items():
        fn = getattr(_lib.lib, name)
        assert fn.restype is res and list(fn.argtypes) == args, name
        params = [p.strip() for p in protos[name].split(",")]
        assert len(params) == len(args), name  # one argument per parameter of the prototype ...
        for p, a in zip(params, args):         # ... of the matching kind
            if "*" in p:
                assert a.__name__ == "c_void_p", (name, p)
            else:
                assert a.__name__ == ctype_of[p.split()[0]], (name, p)


def _emit(L, **kw):
    a = dict(P=16, ldp=128, n_drug=100, Q=16, ldq=128, n_dis=50, h1=128, h2=64, W2=16, b2=16, w3=16, b3=16, kd=None,
             ks=None, n_known=0, cut=0.0, cap=10, od=16, os=16, ol=16, oc=16, oi=16, ws=16, wsb=1 << 40, stream=None)
    a.update(kw)
    return L.dgmi_pair_mlp_emit_f32(a["P"], a["ldp"], a["n_drug"], a["Q"], a["ldq"], a["n_dis"], a["h1"], a["h2"], a["W2"],
                                    a["b2"], a["w3"], a["b3"], a["kd"], a["ks"], a["n_known"], a["cut"], a["cap"], a["od"],
                                    a["os"], a["ol"], a["oc"], a["oi"], a["ws"], a["wsb"], a["stream"])


def test_emit_argument_validation_returns_codes_without_a_gpu():
    from dream_gnn_amd import _lib

    L = _lib.lib
    assert _emit(L, cap=-1) == -1 and _emit(L, cap=MAX_RECORDS + 1) == -1        # capacity outside 0..2**24
    assert _emit(L, h1=256) == -1 and _emit(L, h2=32) == -1                      # only the reference's widths
    assert _emit(L, ldp=127) == -1 and _emit(L, ldq=64) == -1 and _emit(L, ldp=130) == -1 and _emit(L, ldq=134) == -1
    assert _emit(L, P=None) == -1 and _emit(L, Q=None) == -1 and _emit(L, b3=None) == -1 and _emit(L, W2=None) == -1
    assert _emit(L, b2=None) == -1 and _emit(L, w3=None) == -1
    assert _emit(L, od=None) == -1 and _emit(L, os=None) == -1 and _emit(L, ol=None) == -1  # records, capacity > 0
    assert _emit(L, oc=None) == -1 and _emit(L, oi=None) == -1
    assert _emit(L, cap=0, oc=None) == -1 and _emit(L, cap=0, oi=None) == -1     # the count is always written
    assert _emit(L, n_known=5) == -1 and _emit(L, n_known=5, kd=16) == -1        # known ids missing
    assert _emit(L, P=20) == -1 and _emit(L, Q=24) == -1 and _emit(L, W2=8) == -1  # not 16-B aligned
    assert _emit(L, n_drug=2 ** 31) == -1 and _emit(L, n_dis=2 ** 31) == -1      # ids beyond int32
    assert _emit(L, n_drug=-1) == -1 and _emit(L, n_dis=-1) == -1 and _emit(L, n_known=-1) == -1
    assert _emit(L, ws=None) == -3 and _emit(L, wsb=64) == -3                    # workspace missing / short
    # capacity 0 permits null record pointers: the call gets past the argument checks to the workspace check
    assert _emit(L, cap=0, od=None, os=None, ol=None, wsb=64) == -3
    assert _emit(L, cap=MAX_RECORDS, wsb=64) == -3 and _emit(L, cut=float("nan"), wsb=64) == -3
    # (the empty problem stores a count of 0 on the device: tests/test_gpu_above.py)


def _sort(L, **kw):
    a = dict(d=16, s=16, l=16, n=100, ws=16, wsb=1 << 40, stream=None)
    a.update(kw)
    return L.dgmi_pair_records_sort_f32(a["d"], a["s"], a["l"], a["n"], a["ws"], a["wsb"], a["stream"])


def test_sort_argument_validation_returns_codes_without_a_gpu():
    from dream_gnn_amd import _lib

    L = _lib.lib
    assert _sort(L, n=0) == 0 and _sort(L, n=0, d=None, s=None, l=None, ws=None) == 0   # nothing to do
    assert _sort(L, n=-1) == -1 and _sort(L, n=MAX_RECORDS + 1) == -1
    assert _sort(L, d=None) == -1 and _sort(L, s=None) == -1 and _sort(L, l=None) == -1
    assert _sort(L, ws=None) == -3 and _sort(L, wsb=64) == -3
    assert _sort(L, n=MAX_RECORDS, wsb=MAX_RECORDS * 4) == -3


def test_workspace_sizing_is_host_arithmetic():
    from dream_gnn_amd import _lib

    W = _lib.lib.dgmi_pair_emit_workspace_bytes
    assert W(0, 50) == 0 and W(10, 0) == 0 and W(-1, 10) == 0 and W(2 ** 31, 10) == 0 and W(10, 2 ** 31) == 0
    assert W(100_000, 50_000) >= 100_000 * ((50_000 + 31) // 32) * 4  # the known-pair bitmap: a word per drug per 32 diseases
    assert W(100_000, 50_000) < _lib.lib.dgmi_pair_topk_workspace_bytes(100_000, 50_000, 1)  # and no lists
    sizes = [W(n, 681) for n in (1, 2, 63, 64, 65, 763, 100_000)]
    assert sizes == sorted(sizes) and sizes[0] > 0
    S = _lib.lib.dgmi_pair_records_sort_workspace_bytes
    assert S(0) == 0 and S(-1) == 0 and S(MAX_RECORDS + 1) == 0
    sizes = [S(n) for n in (1, 100, 8192, 8193, 1 << 20, MAX_RECORDS)]
    assert sizes == sorted(sizes) and sizes[0] > 0
    assert S(1 << 20) >= 7 * 4 * (1 << 20)  # the key array and two three-field record buffers


def _cpu_args():
    return (torch.zeros(2, 128), torch.zeros(2, 128), torch.zeros(64, 128), torch.zeros(64), torch.zeros(64), torch.zeros(1),
            None, None)


def test_torch_ops_are_registered_and_have_no_cpu_kernel():
    from dream_gnn_amd import _lib  # noqa: F401

    emit = torch.ops.dreamgnn_mi.pair_mlp_emit.default._schema
    assert [a.name for a in emit.arguments] == ["P", "Q", "W2", "b2", "w3", "b3", "known_drug", "known_dis", "min_logit",
                                                "out_drug", "out_dis", "out_logit"]
    assert [r.name for r in emit.returns] == ["count", "info"]
    assert [a.name for a in emit.arguments if a.alias_info is not None and a.alias_info.is_write] == ["out_drug", "out_dis",
                                                                                                     "out_logit"]
    sort = torch.ops.dreamgnn_mi.pair_records_sort.default._schema
    assert [a.name for a in sort.arguments] == ["drug", "dis", "logit", "n"] and len(sort.returns) == 0
    ids, logit = torch.zeros(4, dtype=torch.int32), torch.zeros(4)
    with pytest.raises(NotImplementedError):
        torch.ops.dreamgnn_mi.pair_mlp_emit(*_cpu_args(), 0.0, ids, ids.clone(), logit)
    with pytest.raises(NotImplementedError):
        torch.ops.dreamgnn_mi.pair_records_sort(ids, ids.clone(), logit, 4)


def test_ops_refuse_cpu_tensors_and_bad_max_pairs():
    from dream_gnn_amd import ops

    assert ops.PAIR_EMIT_MAX_RECORDS == MAX_RECORDS
    assert issubclass(ops.TooManyPairs, RuntimeError)
    e = ops.TooManyPairs(28_800, 1000)
    assert e.count == 28_800 and e.max_pairs == 1000 and "28800" in str(e) and "1000" in str(e)
    for bad in (0, -1, MAX_RECORDS + 1):
        with pytest.raises(ValueError, match="max_pairs"):
            ops.pair_mlp_above(*_cpu_args(), 0.0, bad)
    with pytest.raises(RuntimeError, match="MI355X only"):
        ops.pair_mlp_above(*_cpu_args(), 0.0, 10)
    with pytest.raises(RuntimeError, match="MI355X only"):
        ops.pair_mlp_count_above(*_cpu_args(), 0.0)


def test_decoder_checks_k_and_max_pairs_first():
    from dream_gnn_amd import model as M

    dec = M.MLPDecoder(4)
    hd, hs = torch.zeros(7, 4), torch.zeros(5, 4)
    for k in (0, -3, (1 << 20) + 1):
        with pytest.raises(ValueError, match="k must be"):
            dec.top_pairs_deep(hd, hs, k)
    for bad in (0, MAX_RECORDS + 1):
        with pytest.raises(ValueError, match="max_pairs"):
            dec.pairs_above(hd, hs, 0.0, max_pairs=bad)
    assert M.MLPDecoder.DEEP_MAX_K == 1 << 20


class _NoDeviceNet(torch.nn.Module):
    """Fails the test if a function gets as far as encoding."""

    def embed(self, *a, **k):
        raise AssertionError("the model was touched before the arguments were validated")


def test_predict_functions_validate_before_the_device():
    import dream_gnn_amd
    from dream_gnn_amd import predict

    for name in ("novel_pairs_above", "count_novel_pairs_above", "top_novel_pairs_deep"):
        assert getattr(dream_gnn_amd, name) is getattr(predict, name) and name in dream_gnn_amd.__all__
    assert predict.DEEP_MAX_K == 1 << 20 and predict.MAX_PAIRS == MAX_RECORDS and predict.MAX_K == 1024
    batch = {"drug_feat": torch.zeros(7, 4), "disease_feat": torch.zeros(5, 4)}
    net = _NoDeviceNet()
    for fn in (predict.novel_pairs_above, predict.count_novel_pairs_above):
        with pytest.raises(ValueError, match="exactly one"):
            fn(net, batch, None)
        with pytest.raises(ValueError, match="exactly one"):
            fn(net, batch, None, min_score=0.5, min_logit=0.0)
        for p in (0.0, 1.0, -0.1, 1.5, float("nan")):
            with pytest.raises(ValueError, match=r"\(0, 1\)"):
                fn(net, batch, None, min_score=p)
        with pytest.raises(ValueError, match="shape"):
            fn(net, batch, np.zeros((5, 7)), min_logit=0.0)
        with pytest.raises(ValueError, match="length"):
            fn(net, batch, ([0, 1], [2]), min_score=0.5)
    for bad in (0, -1, MAX_RECORDS + 1):
        with pytest.raises(ValueError, match="max_pairs"):
            predict.novel_pairs_above(net, batch, None, min_logit=0.0, max_pairs=bad)
    for k in (0, -1, (1 << 20) + 1):
        with pytest.raises(ValueError, match="k must be"):
            predict.top_novel_pairs_deep(net, batch, None, k)
    with pytest.raises(ValueError, match="shape"):
        predict.top_novel_pairs_deep(net, batch, np.zeros((5, 7)), 2000)
    with pytest.raises(ValueError, match="length"):
        predict.top_novel_pairs_deep(net, batch, ([0, 1], [2]), 2000)
    assert net.training  # untouched


def test_min_score_becomes_one_fp32_logit():
    from dream_gnn_amd import predict

    assert predict._cut_logit(0.5, None) == 0.0
    for p in (0.9, 0.1, 0.999999, 1e-30):
        want = np.float32(math.log(p / (1.0 - p)))
        got = predict._cut_logit(p, None)
        assert np.float32(got) == want and got == float(want)
    assert predict._cut_logit(None, 1.25) == 1.25 and predict._cut_logit(None, 0.1) == float(np.float32(0.1))
    assert math.isnan(predict._cut_logit(None, float("nan"))) and predict._cut_logit(None, float("-inf")) == float("-inf")
