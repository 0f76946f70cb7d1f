"""The references of ``_edge_cases.py`` inside their own zero tolerance, and its designs doing what they claim under the
geometry restated from ``dgmi_edge.hip`` / ``dgmi_select.hip`` (no GPU): every kernel form, every loop-trip count, the
tail statement, a cap crossing per kernel, every column-sum trip / tail split, the window clamps of the selection."""
import numpy as np
import torch

import _edge_cases as EC


# ---------------------------------------------------------------------------------------------
# forms and strides
# ---------------------------------------------------------------------------------------------
def test_every_width_and_variant_takes_the_kernel_it_is_listed_under():
    for widths, form in ((EC.POW2_WIDTHS, "pow2"), (EC.VEC4_WIDTHS, "vec4"), (EC.DWORD_WIDTHS, "dword")):
        for Fa, Fb in widths:
            v = EC.concat_variants(Fa, Fb)
            for name, (lda, ldb, ldo, oa, ob, oo) in v.items():
                got = EC.concat_form(Fa, Fb, lda, ldb, ldo, 4 * oa, 4 * ob, 4 * oo)
                assert got == (form if name in ("plain", "strided") else "dword"), (Fa, Fb, name)
            assert (len(v) == 8) == (form != "dword")
    # by hand: 128 + 128 is one edge per wave, 512 + 512 one per block, 344 + 344 has 172 float4 (no divisor of 256)
    assert EC.concat_form(128, 128, 128, 128, 256) == "pow2" and EC.concat_form(344, 344, 344, 344, 688) == "vec4"
    assert EC.concat_form(128, 64, 128, 64, 192) == "vec4" and EC.concat_form(12, 12, 12, 12, 24) == "vec4"
    assert EC.concat_form(128, 128, 128, 128, 256, po=4) == "dword" and EC.concat_form(5, 7, 5, 7, 12) == "dword"
    for F in EC.ADD_WIDTHS:
        for name, (lda, ldb, ldo, oa, ob, oo) in EC.add_variants(F).items():
            vec = 4 if F % 4 == 0 and name in ("plain", "strided") else 1
            assert EC.add_form(F, lda, ldb, ldo, 4 * oa, 4 * ob, 4 * oo) == (vec, False), (F, name)
            assert EC.add_form(F, lda, ldb, ldo, 4 * oa, 4 * ob, 4 * oo, 0) == (vec, True)
            assert EC.add_form(F, lda, ldb, ldo, 4 * oa, 4 * ob, 4 * oo, 4) == (1, True)  # a bias 4 bytes off: dword
    forms = {EC.add_form(F, F, F, F, pbias=b) for F in EC.ADD_WIDTHS for b in (None, 0, 4)}
    assert forms == {(4, False), (4, True), (1, False), (1, True)}
    assert EC.scale_form(128, 128, 136) == 4 and EC.scale_form(128, 133, 128) == 1 and EC.scale_form(7, 7, 7) == 1
    assert EC.scale_form(128, 128, 128, po=4) == 1


def test_grid_for_and_stride_geometry_by_hand():
    assert [EC.grid_for(n) for n in (0, 1, 256, 257, 8192 * 256, 8192 * 256 + 1, 10 ** 9)] == [1, 1, 1, 2, 8192, 8192, 8192]
    g = EC.stride_geometry(8192 * 256 + 5)
    assert (g.grid, g.trips_min, g.trips_max, g.capped) == (8192, 1, 2, True)
    g = EC.stride_geometry(8192 * 256)
    assert (g.trips_min, g.trips_max, g.capped) == (1, 1, False)
    g = EC.stride_geometry(4096 * 256 + 77, EC.EPILOGUE_CAP)
    assert (g.grid, g.trips_max, g.capped) == (4096, 2, True)
    assert not EC.stride_geometry(4096 * 256 - 1, EC.EPILOGUE_CAP).capped


def _pow2_brute(E, Fa, Fb):
    """The kernel's loop, slot by slot: (trips, tail, edges written)."""
    W4 = (Fa + Fb) // 4
    epb = 256 // W4
    blocks = -(-E * W4 // 256)
    stride = EC.grid_for(blocks * 256 // 2) * epb
    trips, tail, written = [], [], []
    for e0 in range(stride):
        e, t = e0, 0
        while e + stride < E:
            written += [e, e + stride]
            e += 2 * stride
            t += 1
        trips.append(t)
        tail.append(e < E)
        if e < E:
            written.append(e)
    return stride, np.array(trips), np.array(tail), sorted(written)


def test_pow2_geometry_equals_the_loop_and_the_edge_counts_realise_every_claim():
    for Fa, Fb in EC.POW2_WIDTHS:
        epb = 256 // ((Fa + Fb) // 4)
        seen = set()
        for E in EC.pow2_edge_counts(Fa, Fb):
            g = EC.pow2_geometry(E, Fa, Fb)
            stride, trips, tail, written = _pow2_brute(E, Fa, Fb)
            assert g.stride == stride and np.array_equal(g.trips, trips) and np.array_equal(g.tail, tail)
            assert written == list(range(E))  # every edge exactly once
            assert g.strides <= 2             # below the cap the grid is half the blocks
            if E == 1:
                seen.add("one")
            if not g.trips.any():
                seen.add("tail only")         # at most one stride: no slot loops
            if E < g.stride:
                seen.add("below one stride")
            if E == g.stride:
                seen.add("one stride")
            if E == 2 * g.stride:
                seen.add("two strides")
                assert g.trips.min() == 1 and not g.tail.any()
            if E == 2 * g.stride - 1:
                seen.add("two strides - 1")
                assert g.trips.sum() == g.stride - 1 and g.tail.sum() == 1
            if g.trips.any() and g.tail.any():
                seen.add("loop and tail in one launch")
            if E == 2 * epb + 1:
                assert g.stride == 2 * epb and g.trips.sum() == 1 and g.tail.sum() == 2 * epb - 1  # "two strides + 1"
        want = {"one", "tail only", "one stride", "two strides", "loop and tail in one launch"}
        assert want <= seen, (Fa, Fb, want - seen)
        assert epb == 1 or {"two strides - 1", "below one stride"} <= seen  # 512 + 512: one edge is one stride
        # the cap crossing: three strides (an odd number), every slot loops once, three slots also take the tail
        E = EC.cap_edge_count("pow2", Fa, Fb)
        g = EC.pow2_geometry(E, Fa, Fb)
        assert g.grid == EC.GRID_CAP and g.strides == 3 and g.trips.min() == g.trips.max() == 1 and g.tail.sum() == 3
        assert E * (Fa + Fb) * 4 < 70e6
        assert EC.pow2_geometry(E - 4, Fa, Fb).strides == 2  # one block pair fewer and the cap is not reached
    assert EC.pow2_geometry(EC.cap_edge_count("pow2", 128, 128), 128, 128).stride == 32_768


def test_grid_stride_edge_counts_reach_one_trip_a_block_edge_inside_an_edge_and_the_cap():
    cases = [("vec4", Fa, Fb) for Fa, Fb in EC.VEC4_WIDTHS] + [("dword", Fa, Fb) for Fa, Fb in EC.DWORD_WIDTHS]
    cases += [("pow2", Fa, Fb) for Fa, Fb in EC.POW2_WIDTHS]  # the variants that fall to the dword kernel
    for form, Fa, Fb in cases:
        W = (Fa + Fb) if form == "dword" else (Fa + Fb) // 4
        counts = EC.stride_edge_counts(W)
        units = [E * W for E in counts]
        assert counts[0] == 1 and (min(units) < 256 or W >= 256) and max(units) > 512
        assert any(u % 256 for u in units if u > 256) or W % 256 == 0  # a ragged last block
        if form != "pow2":
            g = EC.stride_geometry(EC.concat_units(form, EC.cap_edge_count(form, Fa, Fb), Fa, Fb))
            assert g.capped and (g.trips_min, g.trips_max) == (1, 2)
            assert not EC.stride_geometry(EC.concat_units(form, EC.cap_edge_count(form, Fa, Fb) - 4, Fa, Fb)).capped or W > 1024
    for F in EC.ADD_WIDTHS:
        for W in {F, F // 4 if F % 4 == 0 else F}:
            g = EC.stride_geometry(EC.cap_edge_count("dword", F, 0) * W if W == F else (EC.GRID_CAP * 256 // W + 4) * W)
            assert g.capped and g.trips_max == 2


def test_indices_name_both_ends_skip_one_node_and_repeat():
    for E in (1, 2, 64, 257, 5000):
        src, dst = EC.edge_pairs(E, EC.N_A, EC.N_B)
        assert src[0] == 0 and dst[0] == EC.N_B - 1 and src.min() >= 0 and src.max() < EC.N_A and dst.max() < EC.N_B
        if E > 1:
            assert src[-1] == EC.N_A - 1 and dst[-1] == 0
        if E >= 64:
            for ids, n in ((src, EC.N_A), (dst, EC.N_B)):
                assert EC.unnamed_node(n) not in ids
                runs = np.flatnonzero(np.diff(ids) != 0)
                assert np.diff(np.concatenate([[-1], runs, [E - 1]])).max() >= 6  # a run of equal ids
                if E >= 5000:
                    assert set(ids.tolist()) == set(range(n)) - {EC.unnamed_node(n)}


# ---------------------------------------------------------------------------------------------
# references against a second evaluation
# ---------------------------------------------------------------------------------------------
def test_concat_reference_is_fancy_indexing_and_the_tables_hold_every_special():
    for Fa, Fb in ((8, 24), (5, 7), (0, 12), (1, 0)):
        lda, ldb = Fa + 8, Fb + 8
        A, B = EC.bit_table(EC.N_A, Fa, lda, 1), EC.bit_table(EC.N_B, Fb, ldb, 2)
        src, dst = EC.edge_pairs(300, EC.N_A, EC.N_B)
        want = EC.concat_reference(src, dst, A, Fa, B, Fb)
        assert np.array_equal(want, np.concatenate([A[:, :Fa][src], B[:, :Fb][dst]], axis=1))
        assert EC.SENT_BITS not in want and EC.SPARE_BITS not in want
        if Fa + Fb >= 12:
            assert set(EC.SPECIAL_BITS) <= set(want.reshape(-1).tolist())
        assert np.all(A[:, Fa:] == EC.SPARE_BITS) and np.isnan(A[:, Fa:].view(np.float32)).all()


def test_add_reference_is_numpy_fp32_and_torch_relu_on_ordinary_and_special_values():
    for F in (12, 7):
        for special in (False, True):
            if special:
                A, B, src, dst = EC.special_tables(F, F + 8, F)
            else:
                A, B = EC.int_table(EC.N_A, F, F + 8, 1), EC.int_table(EC.N_B, F, F, 2)
                src, dst = EC.edge_pairs(500, EC.N_A, EC.N_B)
            bias = EC.int_table(1, F, F, 3)[0]
            for b in (None, bias):
                with np.errstate(invalid="ignore"):
                    x32 = A[src, :F] + B[dst, :F]
                    if b is not None:
                        x32 = x32 + b
                assert x32.dtype == np.float32
                assert EC.same_values(EC.add_reference(src, dst, A, B, b, F, 0), x32)
                assert EC.same_values(EC.add_reference(src, dst, A, B, b, F, 1), torch.relu(torch.from_numpy(x32)).numpy())
            if special:
                got = EC.add_reference(src, dst, A, B, None, F, 1)[:49, 0].reshape(7, 7)
                nan, inf = np.nan, np.inf  # rows / columns: NaN, +inf, -inf, -0, +0, 3, -3
                assert np.isnan(got[0]).all() and np.isnan(got[:, 0]).all()       # NaN + anything stays NaN through relu
                assert np.isnan(got[1, 2]) and np.isnan(got[2, 1])                # inf - inf
                assert got[1, 1] == inf and got[1, 5] == inf and got[2, 2] == 0 and got[2, 5] == 0  # -inf becomes 0
                assert got[5, 6] == 0 and got[5, 5] == 6 and got[6, 6] == 0 and got[3, 3] == 0
                raw = EC.add_reference(src, dst, A, B, None, F, 0)[:49, 0].reshape(7, 7)
                assert np.signbit(raw[3, 3]) and not np.signbit(raw[3, 4]) and raw[2, 2] == -inf
    assert not EC.same_values(np.array([np.nan, 1.0]), np.array([0.0, 1.0])) and EC.same_values(np.array([-0.0]), np.array([0.0]))


def test_epilogue_reference_against_an_integer_evaluation_and_every_kind_meets_every_gradient():
    n = 4096 * 256 + 77
    dY, Y, mask = EC.epilogue_operands(n)
    assert set(np.unique(dY[np.isfinite(dY)]).tolist()) == set(range(-8, 0)) | set(range(1, 9))
    kinds = np.arange(n) % 5
    for k in range(5):
        assert len(set(dY[(kinds == k) & np.isfinite(dY)].tolist())) == 16
        for lo in (40, 45, 50):  # +inf, -inf, NaN each against every Y kind
            assert k in kinds[lo:lo + 5]
    assert np.signbit(Y[3]) and Y[3] == 0 and not np.signbit(Y[2]) and np.isnan(Y[4])
    fin = np.isfinite(dY)
    d = dY[fin].astype(np.int64)
    pos = (Y[fin] > 0)
    for act in (0, 1, 2):
        for m in ((None, mask) if act != 2 else (None,)):
            want = EC.epilogue_reference(dY, Y, m, act)
            if act == 2:
                quarter = np.where(pos, d * 8, 0)           # in units of 0.25
            else:
                quarter = d * np.where(pos | (act == 0), 4, 1)
                if m is not None:
                    quarter = quarter * (m[fin].astype(np.int64) * 2)
            assert np.array_equal(want[fin], (quarter / 4).astype(np.float32)), (act, m is None)
    w = EC.epilogue_reference(dY, Y, mask, 1)
    assert np.isnan(w[50:55]).all() and np.isnan(w[[40, 43, 46, 49]]).all()  # NaN gradient; inf * (mask 0)
    w2 = EC.epilogue_reference(dY, Y, None, 2)
    assert w2[40] == np.inf and np.all(w2[41:45] == 0) and w2[50] != w2[50] and np.all(w2[51:55] == 0)  # Y > 0 at i % 5 == 0 only
    # where > and >= differ: Y == +0 and -0 under act 1 take the slope, under act 2 give 0
    assert w[2] == dY[2] * 0.25 * 2 and w2[2] == 0 and w2[3] == 0 and EC.epilogue_reference(dY, Y, None, 1)[3] == dY[3] * 0.25


def test_colsum_rank_add_and_scale_references_are_float64_products_and_np_add_at():
    for n in EC.COLSUM_N:
        for W, B in ((65, 3), (1, 64), (344, 1)):
            A, coef = EC.colsum_operands(n, W, B, W + 4, n + 3)
            want = EC.colsum_reference(A, coef, n, W)
            assert want.shape == (B, W)
            assert np.array_equal(want, (coef[:, :n].astype(np.float64) @ A[:n, :W].astype(np.float64)).astype(np.float32))
            acc = np.zeros((B, W))
            for b in range(B if n <= 261 else 1):
                np.add.at(acc[b], np.tile(np.arange(W), n), (coef[b, :n, None].astype(np.float64) * A[:n, :W]).reshape(-1))
                assert np.array_equal(want[b], acc[b].astype(np.float32))
            if n:
                assert np.all(A[max(0, n - 16):n, :W] != 0) and np.all(coef[:, max(0, n - 16):n] != 0)
            else:
                assert not want.any()
            G, cf, gs = EC.rank_add_operands(n, W, B, W + 4, n + 3, W + 8)
            want = EC.rank_add_reference(G, cf, gs, n, W)
            f64 = G[:n, :W].astype(np.float64) + cf[:, :n].astype(np.float64).T @ gs[:, :W].astype(np.float64)
            assert np.array_equal(want, f64.astype(np.float32))
    X, scale = EC.scale_operands(300, 12, 20)
    assert set(scale.tolist()) == set(EC.SCALE_VALUES.tolist())
    assert np.array_equal(EC.scale_reference(X, scale, 300, 12), X[:, :12] * scale[:, None])


def test_colsum_row_counts_reach_every_trip_and_tail_split():
    assert EC.colsum_geometry(0) == [(0, 0)] * 16
    assert EC.colsum_geometry(127) == [(1, 0)] * 15 + [(0, 7)]
    assert EC.colsum_geometry(128) == [(1, 0)] * 16
    assert EC.colsum_geometry(129) == [(1, 1)] + [(1, 0)] * 15
    assert EC.colsum_geometry(17) == [(0, 2)] + [(0, 1)] * 15
    assert EC.colsum_geometry(15)[-1] == (0, 0) and EC.colsum_geometry(1)[0] == (0, 1)
    seen = {g for n in EC.COLSUM_N for g in EC.colsum_geometry(n)}
    assert {t for _, t in seen} == set(range(8)) and {t for t, _ in seen} == {0, 1, 2, 5, 6}
    assert (2, 0) in seen and (2, 1) in seen and (1, 7) in seen and (5, 7) in seen and (6, 0) in seen
    for n in EC.COLSUM_N:  # brute force: rows of wave w are w, w + 16, ...
        for w, (trips, tail) in enumerate(EC.colsum_geometry(n)):
            u, t = w, 0
            while u + 7 * 16 < n:
                u, t = u + 128, t + 1
            assert (t, len(range(u, n, 16))) == (trips, tail)


# ---------------------------------------------------------------------------------------------
# multiplicity
# ---------------------------------------------------------------------------------------------
def test_multiplicity_design_claims_and_expectation_equals_the_fp32_detection():
    cases = EC.multiplicity_cases()
    assert {len(cases["good-%dmod4" % r]) % 4 for r in (1, 2, 3)} == {1, 2, 3}
    good = EC.multiplicity_rows()
    names = [r.name for r in good]
    for L in EC.MULT_LENGTHS:
        for pos in {p % L for p in EC.MULT_POSITIONS if -L <= p < L}:
            r = good[names.index("min@%d/%d" % (pos, L))]
            assert r.vals.size == L and int(np.argmin(r.vals)) == pos and (r.vals == r.vals.min()).sum() == 1
            assert r.mult[pos] == 0 and (L == 1 or r.mult.max() == 7) and r.scale == r.vals.min()
    assert {"min@63/64", "min@64/65", "min@64/129", "min@128/129", "min@199/200", "min@0/1"} <= set(names)
    for c in range(1, 8):
        r = good[names.index("c=%d" % c)]
        assert r.vals.size > 64 and r.vals.min() == c * r.scale and r.mult.min() == c - 1 and r.mult.max() == 7
    assert EC.multiplicity_expectation([8, 8, 8], 0.5)[0] == 4.0  # "c = 8" with a form is an all-equal row: c = 1 takes it
    assert EC.multiplicity_expectation([1, 9], 1.0) == (0.0, None) and EC.multiplicity_expectation([2, 18], 1.0) == (0.0, None)
    assert EC.multiplicity_expectation([6, 8], 1.0)[0] == 2.0 and list(EC.multiplicity_expectation([6, 8], 1.0)[1]) == [2, 3]
    r = good[names.index("all-8s")]
    assert r.vals.size == 130 and r.scale == 8 * 2.0 ** -7 and not r.mult.any()
    assert names.count("empty") == 2
    for name, rows in cases.items():
        want = EC.multiplicity_case(rows)
        assert want.indptr[-1] == want.vals.size == want.mult.size
        assert want.fail == (1 if name.startswith("fail") or name == "breakers" else 0)
        for i, r in enumerate(rows):
            scale, mult, failed = EC.kernel_multiplicity_fp32(r.vals)
            b, e = want.indptr[i], want.indptr[i + 1]
            assert scale == want.row_scale[i], (name, r.name)
            assert failed == (r.mult is None and r.vals.size > 0), (name, r.name)
            assert np.array_equal(want.mult[b:e], np.zeros(e - b, np.int32) if mult is None else mult)
    for r in EC.breaker_rows():  # without its one element the row has a form; the element sits where the name says
        pos = int(r.name.split("@")[1].split("/")[0])
        rest = np.delete(r.vals, pos)
        assert not EC.kernel_multiplicity_fp32(rest)[2] and EC.kernel_multiplicity_fp32(r.vals)[2]
        assert r.vals[pos] > rest.min() and r.vals[pos] < 1.01 * rest.min()
    assert {int(r.name.split("@")[1].split("/")[0]) for r in EC.breaker_rows()} >= {0, 63, 64, 128, 199}
    for kind in EC.FAIL_KINDS:
        assert EC.kernel_multiplicity_fp32(EC.failing_row(kind).vals)[2], kind
    # a minimum over the first 64 values only: unnoticed on power-of-two scales (the c-loop recovers s exactly), one ulp
    # off on the rowsum rows
    for r in good:
        if r.vals.size:
            a, b = EC.kernel_multiplicity_fp32(r.vals), EC.kernel_multiplicity_fp32(r.vals, min_over=64)
            assert a[0] == b[0] and np.array_equal(a[1], b[1])
    for r in EC.rowsum_rows():
        a, b = EC.kernel_multiplicity_fp32(r.vals), EC.kernel_multiplicity_fp32(r.vals, min_over=64)
        assert a[0] == r.scale == r.vals[64] and np.array_equal(a[1], r.mult) and not a[2]
        assert not b[2] and b[0] != a[0] and abs(float(b[0]) - float(a[0])) < 2e-7 * float(a[0])


def test_reference_adjacency_rows_pass_64_values_and_have_the_exact_form():
    indptr, vals, m = EC.reference_adjacency()
    assert np.diff(indptr).min() > 64 and set(m.tolist()) == {1, 2}
    for i in range(indptr.size - 1):
        v, mi = vals[indptr[i]:indptr[i + 1]], m[indptr[i]:indptr[i + 1]]
        assert mi.min() == 1
        scale, mult, failed = EC.kernel_multiplicity_fp32(v)
        assert not failed and scale == v.min() and np.array_equal(mult, mi - 1)
        assert abs(float(v.astype(np.float64).sum()) - 1.0) < 1e-5  # D^-1 (...): rows sum to 1


# ---------------------------------------------------------------------------------------------
# selection
# ---------------------------------------------------------------------------------------------
def test_restated_hash_and_lexsort_description_equal_the_oracle(oracle):
    lists = [(E, k) for E in EC.SMALL_WINDOW_E for k in EC.small_window_keeps(E)] + list(EC.LAST_BIN_CASES)
    lists += [(65_537, 65_536), (65_535, 1), (1000, 0), (1000, 1000)]
    for E, keep in lists:
        for seed in EC.SELECT_SEEDS + (EC.LAST_BIN_SEED,):
            assert np.array_equal(oracle._edge_hash(seed, E).astype(np.uint32), EC.edge_hash(seed, np.arange(E, dtype=np.uint32)))
            for off in (0, 17):
                assert np.array_equal(EC.select_description(E, keep, seed, off), oracle.random_subset_select(E, keep, seed, off))
            m = EC.select_mask(E, keep, seed)
            assert m.sum() == keep and np.array_equal(m, oracle.random_subset_mask(E, keep, seed))
            assert np.array_equal(m, oracle.keep_mask(EC.select_description(E, keep, seed), E))
    for i in range(8):
        E, keep, seed, off = (EC.BATCH[k][i] for k in ("E", "keep", "seed", "off"))
        assert np.array_equal(EC.select_description(E, keep, seed, off), oracle.random_subset_select(E, keep, seed, off))


def test_hash_is_a_bijection_of_the_edge_id():
    for seed in EC.SELECT_SEEDS:
        assert np.unique(EC.edge_hash(seed, np.arange(1 << 17, dtype=np.uint32))).size == 1 << 17


def test_selection_lists_sit_on_both_sides_of_the_window_threshold_and_reach_every_clamp():
    assert EC.WINDOW_MIN_E == 65_536
    assert [EC.select_path(E, E // 2) for E in EC.EDGE_E] == ["block", "window", "window"]
    assert EC.select_path(65_537, 0) == "none" and EC.select_path(65_537, 65_537) == "block"
    hit = miss = 0
    for E in EC.EDGE_E[1:]:
        for keep in EC.edge_keeps(E):
            for seed in EC.SELECT_SEEDS:
                w = EC.select_window(E, keep, seed)
                assert w.outcome == "window" and 1 <= w.n_coll <= 16     # the default window holds the key
                assert w.lo_clamped == (keep <= 2) and w.hi_clamped == (keep >= E - 2)
                n = EC.select_window(E, keep, seed, narrow=True)
                hit, miss = hit + (n.outcome == "window"), miss + (n.outcome == "miss")
    assert miss >= 10 and hit >= 1  # the narrow window misses for most lists and holds the key for some
    paths = [EC.select_path(E, k) for E, k in zip(EC.BATCH["E"], EC.BATCH["keep"])]
    assert paths == ["window", "block", "none", "block", "block", "block", "window", "block"]
    # select_window_min = 2: short lists take the window passes with the window over the whole hash space
    both = 0
    for E in EC.SMALL_WINDOW_E:
        for keep in EC.small_window_keeps(E):
            assert EC.select_path(E, keep, 2) == "window"
            for seed in EC.SELECT_SEEDS:
                w = EC.select_window(E, keep, seed)
                assert w.outcome == "window"
                if E <= 64:
                    assert w.lo == 0 and w.lo_clamped and w.hi_clamped and w.binw > 2 ** 20
                both += w.lo_clamped and w.hi_clamped
    assert both >= 15
    assert EC.select_path(2, 1, 2) == "window" and EC.select_path(2, 2, 2) == "block"
    for E, keep in EC.LAST_BIN_CASES:
        w = EC.select_window(E, keep, EC.LAST_BIN_SEED)
        assert w.outcome == "window" and w.bin == 4095 and w.bin_hi_clamped and w.lo == 0 and w.binw == 2 ** 20 + 1
