"""All-pairs decoder top-k, host side (no GPU): include/dgmi_pairs.h declares exactly the new entry points, the
library exports them and the ctypes table matches; argument validation and workspace sizing return codes before any
launch; the torch op is registered; top_novel_pairs refuses bad k / known before touching the device."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY_POINTS = ["dgmi_pair_mlp_topk_f32", "dgmi_pair_topk_workspace_bytes"]


def _declared():
    text = open(os.path.join(ROOT, "include", "dgmi_pairs.h")).read()
    return sorted(set(re.findall(r"DGMI_API\s+[\w\s\*]+?\b(dgmi_\w+)\s*\(", text)))


def test_header_declares_the_pair_entry_points():
    assert _declared() == ENTRY_POINTS
    text = open(os.path.join(ROOT, "include", "dgmi_pairs.h")).read()
    assert '#include "dgmi.h"' in text and "#define DGMI_PAIR_TOPK_MAX_K 1024" in text


def test_library_exports_the_pair_entry_points():
    from dream_gnn_amd import _lib

    assert sorted(_lib.PAIR_SIGNATURES) == _declared()
    assert not set(_lib.PAIR_SIGNATURES) & set(_lib.SIGNATURES)
    for name, (res, args) in _lib.PAIR_SIGNATURES.items():
        fn = getattr(_lib.lib, name)
        assert fn.restype is res and list(fn.argtypes) == args, name
    # one argument per parameter of the prototype
    text = open(os.path.join(ROOT, "include", "dgmi_pairs.h")).read()
    for name in ENTRY_POINTS:
        proto = re.search(name + r"\s*\(([^)]*)\)", text).group(1)
        assert len(proto.split(",")) == len(_lib.PAIR_SIGNATURES[name][1]), name


def _call(L, **kw):
    a = dict(P=16, ldp=128, n_drug=100, Q=16, ldq=128, n_dis=50, h1=128, h2=64, W2=16, b2=16, w3=16, b3=16,
             kd=None, ks=None, n_known=0, k=10, od=16, os_=16, ol=16, oi=16, ws=16, wsb=1 << 40, stream=None)
    a.update(kw)
    return L.dgmi_pair_mlp_topk_f32(a["P"], a["ldp"], a["n_drug"], a["Q"], a["ldq"], a["n_dis"], a["h1"], a["h2"], a["W2"],
                                    a["b2"], a["w3"], a["b3"], a["kd"], a["ks"], a["n_known"], a["k"], a["od"], a["os_"],
                                    a["ol"], a["oi"], a["ws"], a["wsb"], a["stream"])


def test_argument_validation_returns_codes_without_a_gpu():
    from dream_gnn_amd import _lib

    L = _lib.lib
    assert _call(L, n_drug=0) == 0 and _call(L, n_dis=0, P=None, Q=None) == 0  # empty problem
    assert _call(L, k=0) == -1 and _call(L, k=1025) == -1                     # k outside 1..1024
    assert _call(L, h1=256) == -1 and _call(L, h2=32) == -1                   # only the reference's widths
    assert _call(L, ldp=127) == -1 and _call(L, ldq=64) == -1 and _call(L, ldp=130) == -1  # ld < 128, not a multiple of 4
    assert _call(L, P=None) == -1 and _call(L, b3=None) == -1 and _call(L, oi=None) == -1  # null pointers
    assert _call(L, n_known=5) == -1                                          # known ids missing
    assert _call(L, P=20) == -1                                               # P not 16-B aligned
    assert _call(L, n_drug=2 ** 31) == -1 and _call(L, n_dis=2 ** 31) == -1  # ids beyond int32
    assert _call(L, n_drug=-1) == -1 and _call(L, n_known=-1) == -1
    assert _call(L, ws=None) == -3 and _call(L, wsb=64) == -3                 # workspace missing / short


def test_workspace_sizing_is_host_arithmetic():
    from dream_gnn_amd import _lib

    W = _lib.lib.dgmi_pair_topk_workspace_bytes
    assert W(0, 50, 10) == 0 and W(10, 0, 10) == 0 and W(10, 10, 0) == 0 and W(10, 10, 1025) == 0
    small, big = W(763, 681, 200), W(100_000, 50_000, 200)
    assert 0 < small < big
    assert big >= 100_000 * ((50_000 + 31) // 32) * 4  # the known-pair bitmap
    assert W(100_000, 50_000, 1024) > big              # per-workgroup lists grow with k
    assert big < 100_000 * ((50_000 + 31) // 32) * 4 + (64 << 20)


def test_torch_op_is_registered():
    from dream_gnn_amd import _lib  # noqa: F401

    assert hasattr(torch.ops.dreamgnn_mi, "pair_mlp_topk")
    schema = torch.ops.dreamgnn_mi.pair_mlp_topk.default._schema
    assert [a.name for a in schema.arguments] == ["P", "Q", "W2", "b2", "w3", "b3", "known_drug", "known_dis", "k"]
    assert len(schema.returns) == 4
    with pytest.raises(NotImplementedError):  # no CPU kernel
        torch.ops.dreamgnn_mi.pair_mlp_topk(torch.zeros(2, 128), torch.zeros(2, 128), torch.zeros(64, 128), torch.zeros(64),
                                            torch.zeros(64), torch.zeros(1), None, None, 1)


def test_ops_refuse_cpu_tensors_and_bad_k():
    from dream_gnn_amd import ops

    args = (torch.zeros(2, 128), torch.zeros(2, 128), torch.zeros(64, 128), torch.zeros(64), torch.zeros(64), torch.zeros(1),
            None, None)
    with pytest.raises(ValueError, match="1024"):
        ops.pair_mlp_topk(*args, 1025)
    with pytest.raises(RuntimeError, match="MI355X only"):
        ops.pair_mlp_topk(*args, 5)


class _NoDeviceNet(torch.nn.Module):
    """Fails the test if top_novel_pairs gets as far as encoding."""

    def embed(self, *a, **k):
        raise AssertionError("top_novel_pairs touched the model before validating its arguments")


def test_top_novel_pairs_validates_before_the_device():
    from dream_gnn_amd import predict, top_novel_pairs

    assert top_novel_pairs is predict.top_novel_pairs and predict.MAX_K == 1024
    batch = {"drug_feat": torch.zeros(7, 4), "disease_feat": torch.zeros(5, 4)}
    net = _NoDeviceNet()
    with pytest.raises(ValueError, match="1024"):
        top_novel_pairs(net, batch, np.zeros((7, 5)), k=1025)
    with pytest.raises(ValueError, match="1024"):
        top_novel_pairs(net, batch, None, k=0)
    with pytest.raises(ValueError, match="shape"):
        top_novel_pairs(net, batch, np.zeros((5, 7)), k=10)
    with pytest.raises(ValueError, match="shape"):
        top_novel_pairs(net, batch, torch.zeros(7, 6), k=10)
    with pytest.raises(ValueError, match="length"):
        top_novel_pairs(net, batch, ([0, 1], [2]), k=10)


def test_novel_pairs_frame_has_the_reference_columns():
    from dream_gnn_amd.predict import NovelPairs

    logit = torch.tensor([3.0, 1.0, -2.0])
    out = NovelPairs(torch.tensor([4, 0, 2]), torch.tensor([1, 3, 3]), logit, torch.sigmoid(logit))
    df = out.to_frame()
    assert list(df.columns) == ["drug_id", "disease_id", "score"] and len(out) == 3
    assert df["drug_id"].tolist() == [4, 0, 2] and np.allclose(df["score"], torch.sigmoid(logit).numpy())
    df = out.to_frame(drug_names=["a", "b", "c", "d", "e"])
    assert df["drug_name"].tolist() == ["e", "a", "c"]

