"""Scoring and ranking GIVEN pairs, host side (no GPU): include/dgmi_given.h declares exactly the new entry points, the
library exports them and the sixth ctypes table matches; argument validation and workspace sizing return codes before
any launch; the torch ops are registered; ops / MLPDecoder / predict refuse bad id lists and a bad `by` before touching
the device."""
import os
import re

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY_POINTS = ["dgmi_pair_mlp_rank_list_f32", "dgmi_pair_mlp_score_list_f32", "dgmi_pair_rank_workspace_bytes"]


def _text():
    return open(os.path.join(ROOT, "include", "dgmi_given.h")).read()


def _declared():
    return sorted(set(re.findall(r"DGMI_API\s+[\w\s\*]+?\b(dgmi_\w+)\s*\(", _text())))


def test_header_declares_the_given_entry_points():
    assert _declared() == ENTRY_POINTS
    assert '#include "dgmi.h"' in _text()


def test_library_exports_the_given_entry_points():
    from dream_gnn_amd import _lib

    assert sorted(_lib.GIVEN_SIGNATURES) == _declared()
    for other in (_lib.SIGNATURES, _lib.PAIR_SIGNATURES, _lib.RANK_SIGNATURES, _lib.ABOVE_SIGNATURES, _lib.BF16_SIGNATURES):
        assert not set(_lib.GIVEN_SIGNATURES) & set(other)
    for name, (res, args) in _lib.GIVEN_SIGNATURES.items():
        fn = getattr(_lib.lib, name)
        assert fn.restype is res and list(fn.argtypes) == args, name
    for name in ENTRY_POINTS:  # one argument per parameter of the prototype
        proto = re.search(name + r"\s*\(([^)]*)\)", _text()).group(1)
        assert len(proto.split(",")) == len(_lib.GIVEN_SIGNATURES[name][1]), name


_BASE = dict(X=16, ldx=128, n_query=100, C=16, ldc=128, n_cand=50, h1=128, h2=64, W2=16, b2=16, w3=16, b3=16, pq=16, pc=16,
             n_pairs=40, kq=None, kc=None, n_known=0, ol=16, oa=16, ot=16, oi=16, ws=16, wsb=1 << 40, stream=None)


def _score(L, **kw):
    a = dict(_BASE)
    a.update(kw)
    return L.dgmi_pair_mlp_score_list_f32(a["X"], a["ldx"], a["n_query"], a["C"], a["ldc"], a["n_cand"], a["h1"], a["h2"], a["W2"],
                                          a["b2"], a["w3"], a["b3"], a["pq"], a["pc"], a["n_pairs"], a["ol"], a["oi"], a["stream"])


def _rank(L, **kw):
    a = dict(_BASE)
    a.update(kw)
    return L.dgmi_pair_mlp_rank_list_f32(a["X"], a["ldx"], a["n_query"], a["C"], a["ldc"], a["n_cand"], a["h1"], a["h2"], a["W2"],
                                         a["b2"], a["w3"], a["b3"], a["pq"], a["pc"], a["n_pairs"], a["kq"], a["kc"], a["n_known"],
                                         a["ol"], a["oa"], a["ot"], a["oi"], a["ws"], a["wsb"], a["stream"])


@pytest.mark.parametrize("call", [_score, _rank])
def test_argument_validation_returns_codes_without_a_gpu(call):
    from dream_gnn_amd import _lib

    L = _lib.lib
    assert call(L, n_pairs=0) == 0 and call(L, n_pairs=0, X=None, C=None, pq=None, ol=None) == 0  # empty list: nothing written
    assert call(L, h1=256) == -1 and call(L, h2=32) == -1                       # only the reference's widths
    assert call(L, ldx=127) == -1 and call(L, ldc=64) == -1 and call(L, ldx=130) == -1 and call(L, ldc=132 + 2) == -1
    assert call(L, X=None) == -1 and call(L, C=None) == -1 and call(L, b3=None) == -1 and call(L, W2=None) == -1
    assert call(L, b2=None) == -1 and call(L, w3=None) == -1
    assert call(L, pq=None) == -1 and call(L, pc=None) == -1 and call(L, ol=None) == -1 and call(L, oi=None) == -1
    assert call(L, X=20) == -1 and call(L, C=24) == -1 and call(L, W2=8) == -1   # not 16-B aligned
    assert call(L, n_query=2 ** 31) == -1 and call(L, n_cand=2 ** 31) == -1 and call(L, n_pairs=2 ** 31) == -1
    assert call(L, n_query=-1) == -1 and call(L, n_cand=-1) == -1 and call(L, n_pairs=-1) == -1


def test_rank_list_validation_of_known_ids_outputs_and_workspace():
    from dream_gnn_amd import _lib

    L = _lib.lib
    assert _rank(L, oa=None) == -1 and _rank(L, ot=None) == -1
    assert _rank(L, n_known=5) == -1 and _rank(L, n_known=5, kq=16) == -1 and _rank(L, n_known=5, kc=16) == -1
    assert _rank(L, n_known=-1) == -1
    assert _rank(L, ws=None) == -3 and _rank(L, wsb=64) == -3                   # workspace missing / short
    need = L.dgmi_pair_rank_workspace_bytes(100, 50, 40)
    assert _rank(L, wsb=need - 1) == -3
    assert _rank(L, n_pairs=0, ws=None, wsb=0) == 0                             # an empty list needs none


def test_workspace_sizing_is_host_arithmetic():
    from dream_gnn_amd import _lib

    W = _lib.lib.dgmi_pair_rank_workspace_bytes
    assert W(0, 50, 10) == 0 and W(10, 0, 10) == 0 and W(10, 10, 0) == 0
    assert W(-1, 10, 10) == 0 and W(10, -1, 10) == 0 and W(10, 10, -1) == 0
    assert W(2 ** 31, 10, 10) == 0 and W(10, 2 ** 31, 10) == 0 and W(10, 10, 2 ** 31) == 0
    # the known-pair bitmap: one word per candidate per 32 queries (rounded up to 256 bytes), whatever the list length
    bitmap = 100_000 * ((50_000 + 31) // 32) * 4
    assert W(50_000, 100_000, 10_000) == (bitmap + 255) // 256 * 256 == W(50_000, 100_000, 1)
    assert 0 < W(1, 1, 1) <= 256
    sizes = [W(n, 100_000, 100) for n in (1, 32, 33, 1000, 50_000)]
    assert sizes == sorted(sizes) and sizes[0] == sizes[1] < sizes[2]
    # what MLPDecoder.rank_pairs saves by passing only the distinct listed rows: 313 instead of 50 000
    assert W(313, 100_000, 10_000) * 100 < W(50_000, 100_000, 10_000)


def test_torch_ops_are_registered():
    from dream_gnn_amd import _lib  # noqa: F401

    ns = torch.ops.dreamgnn_mi
    assert hasattr(ns, "pair_mlp_score_list") and hasattr(ns, "pair_mlp_rank_list")
    schema = ns.pair_mlp_score_list.default._schema
    assert [a.name for a in schema.arguments] == ["X", "C", "W2", "b2", "w3", "b3", "pair_query", "pair_cand"]
    assert [r.name for r in schema.returns] == ["logit", "info"]
    schema = ns.pair_mlp_rank_list.default._schema
    assert [a.name for a in schema.arguments] == ["X", "C", "W2", "b2", "w3", "b3", "pair_query", "pair_cand", "known_query",
                                                  "known_cand"]
    assert [r.name for r in schema.returns] == ["logit", "above", "total", "info"]
    z = (torch.zeros(2, 128), torch.zeros(2, 128), torch.zeros(64, 128), torch.zeros(64), torch.zeros(64), torch.zeros(1),
         torch.zeros(1, dtype=torch.int64), torch.zeros(1, dtype=torch.int64))
    with pytest.raises(NotImplementedError):  # no CPU kernel
        ns.pair_mlp_score_list(*z)
    with pytest.raises(NotImplementedError):
        ns.pair_mlp_rank_list(*z, None, None)


def test_ops_refuse_bad_lists_and_cpu_tensors():
    from dream_gnn_amd import ops

    dec = (torch.zeros(2, 128), torch.zeros(2, 128), torch.zeros(64, 128), torch.zeros(64), torch.zeros(64), torch.zeros(1))
    ids = torch.zeros(3, dtype=torch.int64)
    for fn in (ops.pair_mlp_score_list, ops.pair_mlp_rank_list):
        with pytest.raises(ValueError, match="length"):
            fn(*dec, ids, ids[:2])
        with pytest.raises(ValueError, match="int32 / int64"):
            fn(*dec, ids.float(), ids)
        with pytest.raises(ValueError, match="int32 / int64"):
            fn(*dec, ids, ids.bool())
        with pytest.raises(ValueError, match="1-D"):
            fn(*dec, ids.view(1, 3), ids.view(1, 3))
        with pytest.raises(RuntimeError, match="MI355X only"):
            fn(*dec, ids, ids)


def test_decoder_checks_ids_and_by_first():
    from dream_gnn_amd import model as M

    dec = M.MLPDecoder(4)
    hd, hs = torch.zeros(7, 4), torch.zeros(5, 4)
    for fn in (dec.score_pairs, dec.rank_pairs):
        with pytest.raises(ValueError, match="length"):
            fn(hd, hs, [0, 1], [2])
        with pytest.raises(ValueError, match="integer"):
            fn(hd, hs, [0.5, 1.0], [2, 3])
        with pytest.raises(ValueError, match="integer"):
            fn(hd, hs, torch.tensor([True, False]), [2, 3])
        with pytest.raises(ValueError, match="1-D"):
            fn(hd, hs, [[0, 1]], [[2, 3]])
    with pytest.raises(ValueError, match="by"):
        dec.rank_pairs(hd, hs, [0], [1], by="pair")
    d, s = M.pair_ids(np.array([2, 0], dtype=np.int32), [1, 4])
    assert d.dtype == s.dtype == torch.int64 and d.tolist() == [2, 0] and s.tolist() == [1, 4]
    d, s = M.pair_ids([], [])
    assert d.numel() == s.numel() == 0 and d.dtype == torch.int64


class _NoDeviceNet(torch.nn.Module):
    """Fails the test if the functions get as far as encoding."""

    def embed(self, *a, **k):
        raise AssertionError("score_pairs / rank_pairs touched the model before validating their arguments")


def test_predict_functions_validate_before_the_device():
    import dream_gnn_amd
    from dream_gnn_amd import predict

    for name in ("score_pairs", "rank_pairs", "PairRanks"):
        assert getattr(dream_gnn_amd, name) is getattr(predict, name) and name in dream_gnn_amd.__all__
    batch = {"drug_feat": torch.zeros(7, 4), "disease_feat": torch.zeros(5, 4)}
    net = _NoDeviceNet()
    with pytest.raises(ValueError, match="length"):
        predict.score_pairs(net, batch, [0, 1], [2])
    with pytest.raises(ValueError, match="integer"):
        predict.score_pairs(net, batch, [0.0, 1.0], [2, 3])
    with pytest.raises(ValueError, match="length"):
        predict.rank_pairs(net, batch, [0, 1], [2], None)
    with pytest.raises(ValueError, match="integer"):
        predict.rank_pairs(net, batch, [0, 1], torch.tensor([True, False]), None)
    with pytest.raises(ValueError, match="by"):
        predict.rank_pairs(net, batch, [0, 1], [2, 3], None, by="row")
    with pytest.raises(ValueError, match="shape"):
        predict.rank_pairs(net, batch, [0, 1], [2, 3], np.zeros((5, 7)))
    with pytest.raises(ValueError, match="length"):
        predict.rank_pairs(net, batch, [0, 1], [2, 3], ([0, 1], [2]))
    assert net.training  # untouched
