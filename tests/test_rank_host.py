"""Per-row decoder top-k, host side (no GPU): include/dgmi_rank.h declares exactly the new entry points, the library
exports them and the third ctypes table matches; argument validation and workspace sizing return codes before any
launch; the torch op is registered; ops / MLPDecoder / predict refuse bad k, rows and known before touching the device;
NovelLists.to_frame has its columns."""
import os
import re

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY_POINTS = ["dgmi_pair_mlp_row_topk_f32", "dgmi_row_topk_workspace_bytes"]


def _text():
    return open(os.path.join(ROOT, "include", "dgmi_rank.h")).read()


def _declared():
    return sorted(set(re.findall(r"DGMI_API\s+[\w\s\*]+?\b(dgmi_\w+)\s*\(", _text())))


def test_header_declares_the_row_entry_points():
    assert _declared() == ENTRY_POINTS
    assert '#include "dgmi.h"' in _text() and "#define DGMI_ROW_TOPK_MAX_K 128" in _text()


def test_library_exports_the_row_entry_points():
    from dream_gnn_amd import _lib

    assert sorted(_lib.RANK_SIGNATURES) == _declared()
    assert not set(_lib.RANK_SIGNATURES) & set(_lib.SIGNATURES)
    assert not set(_lib.RANK_SIGNATURES) & set(_lib.PAIR_SIGNATURES)
    assert _lib.ROW_TOPK_MAX_K == 128
    for name, (res, args) in _lib.RANK_SIGNATURES.items():
        fn = getattr(_lib.lib, name)
        assert fn.restype is res and list(fn.argtypes) == args, name
    for name in ENTRY_POINTS:  # one argument per parameter of the prototype
        proto = re.search(name + r"\s*\(([^)]*)\)", _text()).group(1)
        assert len(proto.split(",")) == len(_lib.RANK_SIGNATURES[name][1]), name


def _call(L, **kw):
    a = dict(X=16, ldx=128, n_query=100, C=16, ldc=128, n_cand=50, h1=128, h2=64, W2=16, b2=16, w3=16, b3=16,
             kq=None, kc=None, n_known=0, k=10, oc=16, ol=16, on=16, oi=16, ws=16, wsb=1 << 40, stream=None)
    a.update(kw)
    return L.dgmi_pair_mlp_row_topk_f32(a["X"], a["ldx"], a["n_query"], a["C"], a["ldc"], a["n_cand"], a["h1"], a["h2"],
                                        a["W2"], a["b2"], a["w3"], a["b3"], a["kq"], a["kc"], a["n_known"], a["k"], a["oc"],
                                        a["ol"], a["on"], a["oi"], a["ws"], a["wsb"], a["stream"])


def test_argument_validation_returns_codes_without_a_gpu():
    from dream_gnn_amd import _lib

    L = _lib.lib
    assert _call(L, n_query=0) == 0 and _call(L, n_query=0, X=None, C=None) == 0  # empty problem: nothing written
    assert _call(L, k=0) == -1 and _call(L, k=129) == -1                          # k outside 1..128
    assert _call(L, h1=256) == -1 and _call(L, h2=32) == -1                       # only the reference's widths
    assert _call(L, ldx=127) == -1 and _call(L, ldc=64) == -1 and _call(L, ldx=130) == -1 and _call(L, ldc=132 + 2) == -1
    assert _call(L, X=None) == -1 and _call(L, C=None) == -1 and _call(L, b3=None) == -1 and _call(L, W2=None) == -1
    assert _call(L, oc=None) == -1 and _call(L, ol=None) == -1 and _call(L, on=None) == -1 and _call(L, oi=None) == -1
    assert _call(L, n_known=5) == -1 and _call(L, n_known=5, kq=16) == -1           # known ids missing
    assert _call(L, X=20) == -1 and _call(L, C=24) == -1 and _call(L, W2=8) == -1   # not 16-B aligned
    assert _call(L, n_query=2 ** 31) == -1 and _call(L, n_cand=2 ** 31) == -1      # ids beyond int32
    assert _call(L, n_query=-1) == -1 and _call(L, n_cand=-1) == -1 and _call(L, n_known=-1) == -1
    assert _call(L, ws=None) == -3 and _call(L, wsb=64) == -3                     # workspace missing / short


def test_workspace_sizing_is_host_arithmetic():
    from dream_gnn_amd import _lib

    W = _lib.lib.dgmi_row_topk_workspace_bytes
    assert W(0, 50, 10) == 0 and W(10, 0, 10) == 0 and W(10, 10, 0) == 0 and W(10, 10, 129) == 0
    assert W(-1, 10, 10) == 0 and W(2 ** 31, 10, 10) == 0 and W(10, 2 ** 31, 10) == 0
    small = W(681, 763, 10)
    assert 0 < small < W(50_000, 100_000, 50)
    # monotone in n_query and in k
    sizes = [W(n, 100_000, 50) for n in (1, 31, 32, 33, 1000, 50_000, 100_000)]
    assert sizes == sorted(sizes)
    sizes = [W(50_000, 100_000, k) for k in (1, 10, 50, 64, 100, 128)]
    assert sizes == sorted(sizes) and sizes[0] < sizes[-1]
    big = W(50_000, 100_000, 50)
    assert big >= 100_000 * ((50_000 + 31) // 32) * 4  # the known-pair bitmap: one word per candidate per 32 queries


def test_torch_op_is_registered():
    from dream_gnn_amd import _lib  # noqa: F401

    assert hasattr(torch.ops.dreamgnn_mi, "pair_mlp_row_topk")
    schema = torch.ops.dreamgnn_mi.pair_mlp_row_topk.default._schema
    assert [a.name for a in schema.arguments] == ["X", "C", "W2", "b2", "w3", "b3", "known_query", "known_cand", "k"]
    assert [r.name for r in schema.returns] == ["cand", "logit", "count", "info"]
    with pytest.raises(NotImplementedError):  # no CPU kernel
        torch.ops.dreamgnn_mi.pair_mlp_row_topk(torch.zeros(2, 128), torch.zeros(2, 128), torch.zeros(64, 128),
                                                torch.zeros(64), torch.zeros(64), torch.zeros(1), None, None, 1)


def test_ops_refuse_cpu_tensors_and_bad_k():
    from dream_gnn_amd import ops

    assert ops.ROW_TOPK_MAX_K == 128
    args = (torch.zeros(2, 128), torch.zeros(2, 128), torch.zeros(64, 128), torch.zeros(64), torch.zeros(64), torch.zeros(1),
            None, None)
    with pytest.raises(ValueError, match="128"):
        ops.pair_mlp_row_topk(*args, 129)
    with pytest.raises(ValueError, match="128"):
        ops.pair_mlp_row_topk(*args, 0)
    with pytest.raises(RuntimeError, match="MI355X only"):
        ops.pair_mlp_row_topk(*args, 5)


def test_decoder_checks_k_by_and_rows_first():
    from dream_gnn_amd import model as M

    dec = M.MLPDecoder(4)
    hd, hs = torch.zeros(7, 4), torch.zeros(5, 4)
    with pytest.raises(ValueError, match="128"):
        dec.top_pairs_per_row(hd, hs, 129)
    with pytest.raises(ValueError, match="by"):
        dec.top_pairs_per_row(hd, hs, 5, by="pair")
    with pytest.raises(ValueError, match="duplicate"):
        dec.top_pairs_per_row(hd, hs, 5, rows=[1, 1])
    with pytest.raises(ValueError, match="outside"):
        dec.top_pairs_per_row(hd, hs, 5, by="disease", rows=[5])
    with pytest.raises(ValueError, match="outside"):
        dec.top_pairs_per_row(hd, hs, 5, by="drug", rows=[-1])
    assert M.query_rows(None, 3) is None and M.query_rows(np.array([2, 0]), 3).tolist() == [2, 0]
    with pytest.raises(ValueError, match="1-D"):
        M.query_rows([[0, 1]], 3)
    with pytest.raises(ValueError, match="1-D"):
        M.query_rows([0.5], 3)


class _NoDeviceNet(torch.nn.Module):
    """Fails the test if the per-row functions get as far as encoding."""

    def embed(self, *a, **k):
        raise AssertionError("top_novel_per_disease / top_novel_per_drug touched the model before validating its arguments")


def test_per_row_functions_validate_before_the_device():
    from dream_gnn_amd import predict, top_novel_per_disease, top_novel_per_drug

    assert top_novel_per_disease is predict.top_novel_per_disease and top_novel_per_drug is predict.top_novel_per_drug
    assert predict.ROW_MAX_K == 128
    batch = {"drug_feat": torch.zeros(7, 4), "disease_feat": torch.zeros(5, 4)}
    net = _NoDeviceNet()
    for fn, rows_kw, n in ((top_novel_per_disease, "diseases", 5), (top_novel_per_drug, "drugs", 7)):
        with pytest.raises(ValueError, match="128"):
            fn(net, batch, np.zeros((7, 5)), k=129)
        with pytest.raises(ValueError, match="128"):
            fn(net, batch, None, k=0)
        with pytest.raises(ValueError, match="shape"):
            fn(net, batch, np.zeros((5, 7)), k=10)
        with pytest.raises(ValueError, match="length"):
            fn(net, batch, ([0, 1], [2]), k=10)
        with pytest.raises(ValueError, match="duplicate"):
            fn(net, batch, None, k=10, **{rows_kw: [0, 2, 0]})
        with pytest.raises(ValueError, match="outside"):
            fn(net, batch, None, k=10, **{rows_kw: [0, n]})
    assert net.training  # untouched


def test_novel_lists_frame_has_its_columns():
    from dream_gnn_amd.predict import NovelLists

    logit = torch.tensor([[3.0, 1.0, float("nan")], [-2.0, float("nan"), float("nan")]])
    drug = torch.tensor([[4, 0, -1], [2, -1, -1]])
    dis = torch.tensor([[1, 1, -1], [3, -1, -1]])
    out = NovelLists("disease", torch.tensor([1, 3]), drug, dis, logit, torch.sigmoid(logit), torch.tensor([2, 1]))
    df = out.to_frame()
    assert list(df.columns) == ["query_id", "rank", "drug_id", "disease_id", "score"] and len(out) == 2
    assert df["query_id"].tolist() == [1, 1, 3] and df["rank"].tolist() == [1, 2, 1]
    assert df["drug_id"].tolist() == [4, 0, 2] and df["disease_id"].tolist() == [1, 1, 3]
    assert np.allclose(df["score"], torch.sigmoid(torch.tensor([3.0, 1.0, -2.0])).numpy())
    df = out.to_frame(drug_names=["a", "b", "c", "d", "e"])
    assert list(df.columns)[-1] == "drug_name" and df["drug_name"].tolist() == ["e", "a", "c"]
