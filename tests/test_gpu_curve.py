"""ops.curve_areas on the MI355X against the integer reference of _curve_cases.py: zero tolerance on every count, on U2
and on auroc (one correctly rounded division of integers), aupr within 4 n 2**-53; bit-equal under reruns, permutations
and the one-segment form; segments equal to themselves alone; flags, thresholds, operand forms, the golden metrics, the
harness evaluation and one graph capture."""
import math
import os

import numpy as np
import pytest
import torch

import _curve_cases as C

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _run(dev, score, label, segment=None, n_segments=0, threshold=0.0, check=False):
    from dream_gnn_amd import ops

    t = lambda a: None if a is None else torch.as_tensor(np.ascontiguousarray(a)).to(dev)
    return ops.curve_areas(t(score), t(label), t(segment), n_segments, threshold, check=check)


def _bits(stats):
    return stats.count.cpu().numpy(), stats.area.cpu().numpy().view(np.int64), int(stats.info[0])


def _assert_matches(stats, ref, n, what):
    """Zero tolerance on the integers, on info and on auroc; aupr within the bound; NaN exactly where defined."""
    count, area = stats.count.cpu().numpy(), stats.area.cpu().numpy()
    assert stats.count.dtype == torch.int64 and stats.area.dtype == torch.float64 and stats.info.dtype == torch.int32
    assert np.array_equal(count, ref.count), (what, count[:4], ref.count[:4])
    assert int(stats.info[0]) == ref.info, what
    P, N, U2 = (ref.count[:, c] for c in (0, 1, 5))
    with np.errstate(all="ignore"):  # the same expression on the host
        auroc = np.where(P * N == 0, np.nan, U2.astype(np.float64) / (2 * P * N).astype(np.float64))
    assert np.array_equal(area[:, 0], auroc, equal_nan=True), what
    assert np.array_equal(np.isnan(area[:, 0]), P * N == 0) and np.array_equal(np.isnan(area[:, 1]), P == 0), what
    ok = P > 0
    err = np.abs(area[ok, 1] - ref.aupr[ok])
    assert err.size == 0 or err.max() <= C.bound(n), (what, err.max(), C.bound(n))
    for name, col in (("P", 0), ("N", 1), ("tp", 2), ("fp", 3), ("groups", 4), ("u2", 5)):
        assert torch.equal(getattr(stats, name), stats.count[:, col])
    assert torch.equal(stats.auroc, stats.area[:, 0]) and torch.equal(stats.aupr, stats.area[:, 1])


# ---------------------------------------------------------------------------------------------
# every design at every size
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", C.SIZES)
def test_designs_match_the_reference(dev, n):
    for design in C.DESIGNS:
        if not C.applies(design, n):
            continue
        score, label = design(n)
        _assert_matches(_run(dev, score, label), C.reference(score, label), n, "%s n=%d" % (design.__name__, n))


@pytest.mark.parametrize("n", [2, 65, 8193, 24593])
def test_exact_cases(dev, n):
    st = _run(dev, *C.all_tied(n))
    assert float(st.auroc[0]) == 0.5 and int(st.groups[0]) == 1
    st = _run(dev, *C.separated(n))
    assert float(st.auroc[0]) == 1.0 and abs(float(st.aupr[0]) - 1.0) <= C.bound(n)
    assert float(_run(dev, *C.reversed_(n)).auroc[0]) == 0.0


@pytest.mark.parametrize("n", [65, 8193, 100003])
def test_bit_equal_across_runs_permutations_and_the_one_segment_form(dev, n):
    rng = np.random.default_rng(n)
    for design in (C.distinct, C.few_levels(7), C.ties_across_every_64, C.infinities):
        score, label = design(n)
        first = _bits(_run(dev, score, label))
        again = _bits(_run(dev, score, label))
        perm = rng.permutation(n)
        moved = _bits(_run(dev, score[perm], label[perm]))
        one = _bits(_run(dev, score, label, np.zeros(n, np.int32), 1))
        for other in (again, moved, one):
            assert np.array_equal(first[0], other[0]) and np.array_equal(first[1], other[1]) and first[2] == other[2]
    seg, S, _ = C.random_segments(n)
    score, label = C.few_levels(7)(n)
    perm = rng.permutation(n)
    a, b = _bits(_run(dev, score, label, seg, S)), _bits(_run(dev, score[perm], label[perm], seg[perm], S))
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])


# ---------------------------------------------------------------------------------------------
# segments
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", C.SEGMENT_SIZES)
@pytest.mark.parametrize("design", C.SEGMENT_DESIGNS, ids=lambda d: d.__name__)
def test_segments_match_the_reference_and_themselves_alone(dev, design, n):
    if not C.segment_applies(design, n):
        return
    seg, S, sizes = design(n)
    for scores in (C.few_levels(7), C.distinct, C.ties_across_every_64):
        score, label = scores(n)
        if S > 5 and sizes[5] > 0:
            label = C.one_class_segment(label, seg, 5)  # a segment with one class only
        ref = C.reference(score, label, seg, S, 0.5)
        st = _run(dev, score, label, seg, S, 0.5)
        _assert_matches(st, ref, n, "%s/%s n=%d" % (design.__name__, scores.__name__, n))
        if S > 5 and sizes[5] > 0:
            assert int(st.N[5]) == 0 and math.isnan(float(st.auroc[5])) and not math.isnan(float(st.aupr[5]))
    # each of a few segments evaluated alone: the same integers, aupr within the bound
    count, area = st.count.cpu().numpy(), st.area.cpu().numpy()
    filled = np.flatnonzero(sizes)
    for s in filled[np.unique(np.linspace(0, filled.size - 1, 6).astype(int))] if filled.size else []:
        mine = seg == s
        alone = _run(dev, score[mine], label[mine], None, 0, 0.5)
        assert np.array_equal(alone.count.cpu().numpy()[0], count[s]), (s, n)
        one = alone.area.cpu().numpy()[0]
        assert np.array_equal(one[:1], area[s, :1], equal_nan=True)
        assert (math.isnan(one[1]) and math.isnan(area[s, 1])) or abs(one[1] - area[s, 1]) <= C.bound(int(mine.sum()))
    assert np.array_equal(count[sizes == 0], np.zeros((int((sizes == 0).sum()), 6), np.int64))
    assert np.isnan(area[sizes == 0]).all()


def test_macro_accuracy_and_f1_on_the_device(dev):
    n = 8193
    seg, S, _ = C.random_segments(n)
    score, label = C.few_levels(7)(n)
    st = _run(dev, score, label, seg, S, 0.5)
    ref = C.reference(score, label, seg, S, 0.5)
    P, N, tp, fp = (ref.count[:, c].astype(np.float64) for c in range(4))
    assert np.allclose(st.accuracy().cpu().numpy(), (tp + N - fp) / (P + N), rtol=0, atol=1e-15)
    assert np.allclose(st.f1().cpu().numpy(), 2 * tp / (2 * tp + fp + (P - tp)), rtol=0, atol=1e-15)
    auroc, aupr = st.macro()
    assert auroc.is_cuda and abs(float(auroc) - np.nanmean(ref.auroc)) <= 1e-14 and abs(float(aupr) - np.nanmean(ref.aupr)) <= 1e-14
    score, label = C.distinct(n)
    whole = _run(dev, score, label)
    pred = score >= 0
    assert abs(float(whole.accuracy()[0]) - np.mean(pred == (label == 1))) <= 1e-15


# ---------------------------------------------------------------------------------------------
# flags
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [65, 8193])
def test_flags(dev, n):
    score, label = C.few_levels(7)(n)
    seg, S, _ = C.random_segments(n)
    clean = _run(dev, score, label, seg, S, check=True)
    assert int(clean.info[0]) == 0

    nan_score = score.copy()
    nan_score[[3, n - 2]] = np.nan
    assert C.group_lengths(np.delete(score, [3, n - 2])).size == C.group_lengths(score).size
    st = _run(dev, nan_score, label)
    ref = C.reference(nan_score, label)
    _assert_matches(st, ref, n, "NaN scores")
    assert int(st.info[0]) == 1 and int(st.groups[0]) == C.group_lengths(score).size + 1  # the NaNs form one more group, the last one ...
    moved = nan_score.copy()
    moved[[3, n - 2]] = -np.inf                              # ... so they count exactly like a score below all others
    assert np.array_equal(st.count.cpu().numpy()[0, [0, 1, 4, 5]], C.reference(moved, label).count[0, [0, 1, 4, 5]])
    with pytest.raises(RuntimeError, match="NaN"):
        _run(dev, nan_score, label, check=True)

    half = label.copy()
    half[5] = 0.5
    st = _run(dev, score, half)
    _assert_matches(st, C.reference(score, half), n, "label 0.5")
    assert int(st.info[0]) == 2
    with pytest.raises(RuntimeError, match="neither 0 nor 1"):
        _run(dev, score, half, check=True)

    bad, S, sizes = C.out_of_range_segments(n)
    st = _run(dev, score, label, bad, S)
    _assert_matches(st, C.reference(score, label, bad, S), n, "segment ids out of range")
    assert int(st.info[0]) == 4 and int((st.P + st.N).sum()) == int(sizes.sum()) < n
    with pytest.raises(RuntimeError, match="out of range"):
        _run(dev, score, label, bad, S, check=True)
    st = _run(dev, nan_score, half, bad, S)
    assert int(st.info[0]) == 7


# ---------------------------------------------------------------------------------------------
# thresholds
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [64, 8193])
def test_thresholds(dev, n):
    seg, S, _ = C.random_segments(n)
    for design in (C.few_levels(7), C.signed_zeros, C.infinities, C.denormals, C.distinct):
        score, label = design(n)
        for theta in (0.0, float(score[n // 3]), math.inf, -math.inf):
            what = "%s theta=%r" % (design.__name__, theta)
            _assert_matches(_run(dev, score, label, threshold=theta), C.reference(score, label, threshold=theta), n, what)
            _assert_matches(_run(dev, score, label, seg, S, theta), C.reference(score, label, seg, S, theta), n, what)
    st = _run(dev, score, label, threshold=math.nan)
    assert int(st.tp[0]) == 0 and int(st.fp[0]) == 0
    st = _run(dev, score, label, threshold=-math.inf)
    assert int(st.tp[0]) == int(st.P[0]) and int(st.fp[0]) == int(st.N[0])


# ---------------------------------------------------------------------------------------------
# operand forms
# ---------------------------------------------------------------------------------------------
def test_operand_forms(dev):
    from dream_gnn_amd import harness, ops

    n = 8193
    score, label = C.few_levels(7)(n)
    seg, S, _ = C.random_segments(n)
    want = _bits(_run(dev, score, label, seg, S))
    ts, tl, tg = torch.from_numpy(score).to(dev), torch.from_numpy(label).to(dev), torch.from_numpy(seg).to(dev)

    def same(stats):
        got = _bits(stats)
        return np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]) and got[2] == want[2]

    wide = torch.zeros(n, 3, device=dev)
    wide[:, 1] = ts
    strided_l = torch.zeros(2 * n, device=dev)
    strided_l[::2] = tl
    strided_g = torch.full((n, 2), -7, dtype=torch.int32, device=dev)
    strided_g[:, 0] = tg
    keep = (wide.clone(), strided_l.clone(), strided_g.clone())
    assert same(ops.curve_areas(wide[:, 1], strided_l[::2], strided_g[:, 0], S, check=False))
    assert torch.equal(wide, keep[0]) and torch.equal(strided_l, keep[1]) and torch.equal(strided_g, keep[2])  # unmodified
    assert same(ops.curve_areas(ts.view(-1, 1), tl.view(-1, 1), tg.view(-1, 1), S, check=False))  # the (E, 1) logits of the decoder
    assert same(ops.curve_areas(ts, tl.bool(), tg.long(), S))
    assert same(ops.curve_areas(ts, tl.long(), tg, S))
    assert same(ops.curve_areas(ts, tl.to(torch.int8), tg, S))
    assert same(harness.auroc_aupr_device(tl, ts, tg, S))
    assert torch.equal(ts, torch.from_numpy(score).to(dev)) and torch.equal(tl, torch.from_numpy(label).to(dev))
    assert torch.equal(tg, torch.from_numpy(seg).to(dev))
    with pytest.raises(RuntimeError, match="float32"):
        ops.curve_areas(ts.double(), tl)
    with pytest.raises(RuntimeError, match="entries"):
        ops.curve_areas(ts, tl[:-1])
    with pytest.raises(ValueError, match="go together"):
        ops.curve_areas(ts, tl, tg)
    empty = ops.curve_areas(ts[:0], tl[:0], tg[:0], 3)
    assert empty.count.tolist() == [[0] * 6] * 3 and torch.isnan(empty.area).all() and int(empty.info[0]) == 0
    empty = ops.curve_areas(ts[:0], tl[:0])
    assert empty.count.tolist() == [[0] * 6] and torch.isnan(empty.area).all()


# ---------------------------------------------------------------------------------------------
# the reference's numbers
# ---------------------------------------------------------------------------------------------
def test_golden_metrics_on_the_device(dev):
    z = np.load(os.path.join(ROOT, "tests", "golden", "metrics.npz"))
    for i in range(3):
        st = _run(dev, z["score%d" % i], z["true%d" % i], check=True)
        assert abs(float(st.auroc[0]) - z["auroc"][i]) <= 1e-12 and abs(float(st.aupr[0]) - z["aupr"][i]) <= 1e-12


def test_evaluate_device_equals_the_host_evaluation(dev):
    from dream_gnn_amd import harness as H, model as M, synth

    torch.manual_seed(3)
    batch, labels = synth.dataset_shaped_batch([(160, 120, 600)], emb=768, k=4, seed=0, device=dev)
    net = M.Net(synth.net_args(n_drug=batch["n_drug"], n_dis=batch["n_dis"])).to(dev)
    n = labels.numel()
    auroc, aupr = H.evaluate(net, batch, labels)
    st = H.evaluate_device(net, batch, labels, check=True)
    assert abs(float(st.auroc[0]) - auroc) <= C.bound(n) and abs(float(st.aupr[0]) - aupr) <= C.bound(n)
    assert int(st.P[0]) == int(labels.sum()) and int(st.P[0] + st.N[0]) == n

    with torch.no_grad():
        net.eval()
        pred, *_ = net(batch["enc_graph"], batch["dec_graph"], batch["drug_graph"], batch["drug_sim_feat"], batch["drug_feat"],
                       batch["disease_graph"], batch["disease_sim_feat"], batch["disease_feat"],
                       batch.get("drug_feature_graph"), batch.get("disease_feature_graph"))
    score, y = pred.view(-1).cpu().numpy(), labels.cpu().numpy()
    drug, dis, _ = batch["enc_pairs"]
    for by, ids, count in (("disease", dis.numpy(), batch["n_dis"]), ("drug", drug.numpy(), batch["n_drug"])):
        st = H.evaluate_device(net, batch, labels, by=by)
        assert st.auroc.shape == (count,)
        got_auroc, got_aupr = st.auroc.cpu().numpy(), st.aupr.cpu().numpy()
        for q in range(count):  # the host loop over diseases / drugs
            mine = ids == q
            if 0 < y[mine].sum() < mine.sum():
                a, p = H.auroc_aupr(y[mine], score[mine])
                assert abs(got_auroc[q] - a) <= C.bound(n) and abs(got_aupr[q] - p) <= C.bound(n), (by, q)
            else:
                assert math.isnan(got_auroc[q])
        _assert_matches(st, C.reference(score, y, ids, count), n, "by=" + by)


def test_one_capture_replays_on_new_scores(dev):
    """ops.curve_areas(check=False) recorded as a single straight-line stream after a warm-up call, replayed after the
    scores were overwritten in place: the bits of the eager result."""
    from dream_gnn_amd import ops

    n = 24593
    seg, S, _ = C.random_segments(n)
    old, label = C.few_levels(7)(n)
    new, _ = C.distinct(n)
    score = torch.from_numpy(old).to(dev)
    tl, tg = torch.from_numpy(label).to(dev), torch.from_numpy(seg).to(dev)
    ops.curve_areas(score, tl, tg, S, check=False)  # warm-up: code objects and kernel attributes exist before the recording
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        captured = ops.curve_areas(score, tl, tg, S, check=False)
    score.copy_(torch.from_numpy(new).to(dev))
    graph.replay()
    torch.cuda.synchronize()
    eager = ops.curve_areas(score, tl, tg, S, check=False)
    a, b = _bits(captured), _bits(eager)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and a[2] == b[2]
    _assert_matches(captured, C.reference(new, label, seg, S), n, "replayed")
