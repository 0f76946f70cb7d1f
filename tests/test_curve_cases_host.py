"""Curve areas, host side (no GPU): the integer reference of _curve_cases.py equals harness.auroc_aupr, sklearn's curves
and the golden metrics; the designs contain what they claim; include/dgmi_curve.h declares exactly the new entry points,
the ctypes table matches, and argument validation and workspace sizing return their codes before any launch."""
import math
import os
import re

import numpy as np
import pytest
import torch

import _curve_cases as C

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY_POINTS = ["dgmi_curve_areas_f32", "dgmi_curve_areas_workspace_bytes"]
HOST_SIZES = [n for n in C.SIZES if n >= 2]


def _both_classes(label):
    return 0 < np.count_nonzero(label) < label.size


# ---------------------------------------------------------------------------------------------
# the reference against the host curve code
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", HOST_SIZES)
@pytest.mark.parametrize("design", C.DESIGNS, ids=lambda d: d.__name__)
def test_reference_equals_the_host_curves(design, n):
    from dream_gnn_amd import harness
    from sklearn import metrics

    if not C.applies(design, n):
        return
    score, label = design(n)
    if not _both_classes(label):  # the host curve code divides by zero there; the definition says NaN
        ref = C.reference(score, label)
        assert math.isnan(ref.auroc[0]) and math.isnan(ref.aupr[0]) == (np.count_nonzero(label) == 0)
        return
    ref = C.reference(score, label)
    # the host codes compare values, for which -0 == +0 as for the key; they take differences (inf - inf) or refuse
    # infinities, so those become huge numbers: the order is what counts.  The designs hold no NaN.
    finite = np.clip(score.astype(np.float64), -1e300, 1e300)
    auroc, aupr = harness.auroc_aupr(label, finite)
    assert abs(ref.auroc[0] - auroc) <= C.bound(n) and abs(ref.aupr[0] - aupr) <= C.bound(n)
    fpr, tpr, _ = metrics.roc_curve(label, finite)
    precision, recall, _ = metrics.precision_recall_curve(label, finite)
    assert abs(ref.auroc[0] - metrics.auc(fpr, tpr)) <= C.bound(n)
    assert abs(ref.aupr[0] - metrics.auc(recall, precision)) <= C.bound(n)


def test_reference_equals_the_golden_metrics():
    z = np.load(os.path.join(ROOT, "tests", "golden", "metrics.npz"))
    for i in range(3):
        ref = C.reference(z["score%d" % i], z["true%d" % i])
        assert abs(ref.auroc[0] - z["auroc"][i]) <= 1e-12 and abs(ref.aupr[0] - z["aupr"][i]) <= 1e-12


@pytest.mark.parametrize("n", HOST_SIZES)
def test_exact_cases(n):
    score, label = C.all_tied(n)
    ref = C.reference(score, label)
    assert ref.auroc[0] == 0.5 and ref.count[0, 4] == 1
    ref = C.reference(*C.separated(n))
    assert ref.auroc[0] == 1.0 and ref.aupr[0] == 1.0
    assert C.reference(*C.reversed_(n)).auroc[0] == 0.0


def test_reference_counts_thresholds_flags_and_segments():
    score = np.array([2.0, -0.0, 0.0, np.nan, -1.0, 0.0], np.float32)
    label = np.array([1, 0, 1, 1, 0, 0.5], np.float32)
    ref = C.reference(score, label)
    # groups, descending: {2}, {-0, 0, 0}, {-1}, {NaN}; a label of 0.5 counts as positive
    assert ref.count[0].tolist() == [4, 2, 3, 1, 4, 1 * (2 * 1 + 2) + 1 * (2 * 3 + 0)] and ref.info == 0b011
    assert C.reference(score, label, threshold=math.inf).count[0, 2:4].tolist() == [0, 0]
    assert C.reference(score, label, threshold=-math.inf).count[0, 2:4].tolist() == [3, 2]  # the NaN never qualifies
    assert C.reference(score, label, threshold=math.nan).count[0, 2:4].tolist() == [0, 0]
    seg = np.array([1, 1, 5, -1, 3, 1], np.int32)
    ref = C.reference(score, label, seg, 4)
    assert ref.info == 0b111 and ref.count[:, :2].tolist() == [[0, 0], [2, 1], [0, 0], [0, 1]]
    assert np.isnan(ref.auroc[[0, 2, 3]]).all() and np.isnan(ref.aupr[[0, 2, 3]]).all() and ref.auroc[1] == 0.75


# ---------------------------------------------------------------------------------------------
# the designs contain what they claim
# ---------------------------------------------------------------------------------------------
def test_designs_contain_what_they_claim():
    for n in (8193, 24593):
        assert C.group_lengths(C.distinct(n)[0]).max() == 1
        assert C.group_lengths(C.all_tied(n)[0]).tolist() == [n]
        score, label = C.separated(n)
        assert score[label == 1].min() > score[label == 0].max() and C.group_lengths(score).max() == 1
        assert [C.group_lengths(C.few_levels(k)(n)[0]).size for k in (2, 7)] == [2, 7]
        ends = np.cumsum(C.group_lengths(C.ties_across_every_64(n)[0]))
        assert not np.any(ends[:-1] % 64 == 0) and np.all(np.diff(np.r_[0, ends])[1:-1] == 64)
        for design in (C.only_positives, C.only_negatives):
            assert np.unique(design(n)[1]).size == 1
    lengths = C.group_lengths(C.tie_across_sort_tile(24593)[0])
    big = int(np.argmax(lengths))
    assert lengths[big] == 8197 and int(lengths[:big].sum()) == 8190 and (np.delete(lengths, big) == 1).all()
    assert 8190 < C.SORT_TILE < 8190 + 8197
    score = C.signed_zeros(8193)[0]
    assert np.signbit(score[score == 0]).any() and not np.signbit(score[score == 0]).all()
    assert C.group_lengths(score).size == 3  # -0 and +0 are one group
    assert np.isinf(C.infinities(8193)[0]).any() and set(np.sign(C.infinities(8193)[0][np.isinf(C.infinities(8193)[0])])) == {-1.0, 1.0}
    d = C.denormals(8193)[0]
    assert np.all(np.abs(d) < np.finfo(np.float32).tiny) and C.group_lengths(d).size == 11


def test_segment_designs_contain_what_they_claim():
    n = 24593
    seg, S, sizes = C.boundary_segments(n)
    assert np.array_equal(np.bincount(seg, minlength=S), sizes) and sizes.sum() == n
    assert sizes[0] == sizes[3] == sizes[-1] == 0 and (sizes == 1).sum() >= 6
    ends = set(np.cumsum(sizes).tolist())
    assert {63, 64, 65, 8191, 8192, 8193, 16383, 16384, 16385} <= ends
    starts = np.cumsum(sizes) - sizes
    assert np.any((sizes > 0) & (starts // 2048 + 3 <= (starts + sizes - 1) // 2048))  # one segment over >= 3 scan tiles
    seg, S, sizes = C.boundary_segments(100003)
    assert sizes.max() > 3 * C.SORT_TILE
    seg, S, sizes = C.single_sample_segments(65)
    assert S == 65 and sorted(seg.tolist()) == list(range(65))
    seg, S, sizes = C.out_of_range_segments(8193)
    assert ((seg < 0) | (seg >= S)).sum() == len(range(0, 8193, 7)) and {-1, S, 2 ** 31 - 1} <= set(seg.tolist())
    label = C.one_class_segment(np.zeros(8193, np.float32), seg, 5)
    assert label[seg == 5].all() and not label[seg != 5].any()


# ---------------------------------------------------------------------------------------------
# the C entry points without a GPU
# ---------------------------------------------------------------------------------------------
def _text():
    return open(os.path.join(ROOT, "include", "dgmi_curve.h")).read()


def test_header_declares_the_curve_entry_points_and_the_table_matches():
    from dream_gnn_amd import _lib

    declared = sorted(set(re.findall(r"DGMI_API\s+[\w\s\*]+?\b(dgmi_\w+)\s*\(", _text())))
    assert declared == ENTRY_POINTS == sorted(_lib.CURVE_SIGNATURES)
    assert '#include "dgmi.h"' in _text()
    for other in (_lib.SIGNATURES, _lib.PAIR_SIGNATURES, _lib.RANK_SIGNATURES, _lib.ABOVE_SIGNATURES, _lib.BF16_SIGNATURES,
                  _lib.GIVEN_SIGNATURES, _lib.LAYOUT_SIGNATURES):
        assert not set(_lib.CURVE_SIGNATURES) & set(other)
    for name, (res, args) in _lib.CURVE_SIGNATURES.items():
        fn = getattr(_lib.lib, name)
        assert fn.restype is res and list(fn.argtypes) == args, name
        proto = re.search(name + r"\s*\(([^)]*)\)", _text()).group(1)
        assert len(proto.split(",")) == len(args), name
    assert int(re.search(r"#define DGMI_CURVE_MAX_SEGMENTS \(1 << (\d+)\)", _text()).group(1)) == 24 and _lib.CURVE_MAX_SEGMENTS == 1 << 24
    header = open(os.path.join(ROOT, "include", "dgmi.h")).read()  # dgmi.h and its version stay as they are
    assert "dgmi_curve" not in header and _lib.lib.dgmi_abi_version() == _lib.ABI_VERSION


_BASE = dict(score=16, label=16, segment=None, n=1000, n_segments=0, threshold=0.0, count=16, area=16, info=16, ws=16,
             wsb=1 << 40, stream=None)


def _areas(L, **kw):
    a = dict(_BASE)
    a.update(kw)
    return L.dgmi_curve_areas_f32(a["score"], a["label"], a["segment"], a["n"], a["n_segments"], a["threshold"], a["count"],
                                  a["area"], a["info"], a["ws"], a["wsb"], a["stream"])


def test_argument_validation_returns_codes_without_a_gpu():
    from dream_gnn_amd import _lib

    L = _lib.lib
    for name in ("score", "label", "count", "area", "info"):
        assert _areas(L, **{name: None}) == -1, name
    assert _areas(L, n=-1) == -1 and _areas(L, n=2 ** 31) == -1 and _areas(L, n=2 ** 40) == -1
    assert _areas(L, n_segments=-1) == -1 and _areas(L, n_segments=2 ** 24 + 1, segment=16) == -1
    assert _areas(L, n_segments=5) == -1                                      # segments without ids
    assert _areas(L, ws=None) == -3 and _areas(L, wsb=64) == -3                # workspace missing / short
    for n, S in ((1000, 0), (1000, 5), (8193, 2 ** 24)):
        need = L.dgmi_curve_areas_workspace_bytes(n, S)
        assert need > 0 and _areas(L, n=n, n_segments=S, segment=16 if S else None, wsb=need - 1) == -3


def test_workspace_sizing_is_host_arithmetic():
    from dream_gnn_amd import _lib

    W = _lib.lib.dgmi_curve_areas_workspace_bytes
    assert W(-1, 0) == 0 and W(2 ** 31, 0) == 0 and W(10, -1) == 0 and W(10, 2 ** 24 + 1) == 0 and W(0, 0) == 0 and W(0, 7) == 0
    assert W(2 ** 31 - 1, 2 ** 24) > 0
    sizes = [W(n, 0) for n in (1, 2048, 2049, 100003, 10_000_000)]
    assert sizes == sorted(sizes) and len(set(sizes)) == 5
    assert W(100003, 0) == W(100003, 681)  # the segment stage sorts in the key stage's buffers
    # two padded record sets and the sort's two: twelve int32 arrays, and little else
    assert 48 * 10_000_000 <= W(10_000_000, 0) <= 50 * 10_000_000


def test_torch_op_is_registered_and_the_wrappers_validate_first():
    from dream_gnn_amd import harness, ops

    schema = torch.ops.dreamgnn_mi.curve_areas.default._schema
    assert [a.name for a in schema.arguments] == ["score", "label", "segment", "n_segments", "threshold"]
    assert [r.name for r in schema.returns] == ["count", "area", "info"]
    score, label = torch.zeros(4), torch.zeros(4)
    with pytest.raises(NotImplementedError):  # no CPU kernel
        torch.ops.dreamgnn_mi.curve_areas(score, label, None, 0, 0.0)
    with pytest.raises(RuntimeError, match="MI355X only"):
        ops.curve_areas(score, label)
    with pytest.raises(RuntimeError, match="MI355X only"):
        harness.auroc_aupr_device(label, score)
    with pytest.raises(ValueError, match="by must be"):
        harness.evaluate_device(None, {}, label, by="pair")
