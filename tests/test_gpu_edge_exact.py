"""The per-edge, epilogue and selection kernels through the C ABI with buffers the test owns — ZERO tolerance: the three
gather-concat kernels and four gather-add forms, the epilogue's backward, the complement form's column sums and their
gradient, the row pre-scale, the multiplicity detection (``csrc/dgmi_edge.hip``) and the subset selection
(``csrc/dgmi_select.hip``), on the designed inputs of ``_edge_cases.py``.

Every call makes three assertions: every output element equals the reference (copies as int32 bit patterns; computed
values exactly, zeros by value and NaN by position); what the call must not write is still the sentinel the buffer was
filled with (the spare columns of a strided output, 64 elements before and after every array); the inputs are unchanged,
guards included.  The torch wrappers are held to the raw calls once per group."""
import ctypes

import numpy as np
import pytest
import torch

import _edge_cases as EC

pytestmark = pytest.mark.gpu

GUARD = 64
BAND = 4096
BAND_BYTE = 0xA5
SENT_I = -0x2A2A2A2B
F_BITS = int(np.array([EC.SENT_F], np.float32).view(np.int32)[0])


@pytest.fixture(scope="module", autouse=True)
def _selection_knobs_back():
    from dream_gnn_amd import _lib

    yield
    _lib.set_tuning("select_window_min", 0)
    _lib.set_tuning("select_narrow_window", 0)


class Arr:
    """A device array of 4-byte elements inside an allocation filled with a sentinel: 64 guard elements on both sides,
    the array ``off`` elements off a 16-byte boundary."""

    def __init__(self, dev, a, fill, off=0):
        a = np.ascontiguousarray(a)
        assert a.dtype.itemsize == 4
        self.shape, self.lo, self.n = a.shape, GUARD + off, a.size
        self.host = np.full(self.lo + self.n + GUARD, fill, np.int32)
        self.host[self.lo:self.lo + self.n] = a.reshape(-1).view(np.int32)
        self.t = torch.from_numpy(self.host.copy()).to(dev)
        assert self.t.data_ptr() % 16 == 0
        self.ptr = self.t.data_ptr() + 4 * self.lo
        assert self.ptr % 16 == 4 * (off % 4)

    def read(self):
        return self.t.cpu().numpy()

    def unchanged(self):
        return np.array_equal(self.read(), self.host)

    def _expected(self, want):
        full = self.host.copy()
        full[self.lo:self.lo + self.n] = np.ascontiguousarray(want).reshape(-1).view(np.int32)
        return full

    def holds_bits(self, want):
        """The whole allocation: ``want`` (spare columns still the sentinel) inside untouched guards, bit for bit."""
        return np.array_equal(self.read(), self._expected(want))

    def holds_values(self, want):
        return EC.same_values(self.read().view(np.float32), self._expected(want).view(np.float32))

    def inner(self, dtype=np.float32):
        return self.read()[self.lo:self.lo + self.n].view(dtype).reshape(self.shape)


def _padded(want, ld, fill):
    """``want`` (rows, W) as int32 bits inside a (rows, ld) array whose spare columns hold the sentinel."""
    full = np.full((want.shape[0], ld), fill, np.int32)
    full[:, :want.shape[1]] = np.ascontiguousarray(want).view(np.int32)
    return full


class _Raw:
    def __init__(self, dev):
        from dream_gnn_amd import _lib, ops

        self.dev, self.L, self.stream, self.T = dev, _lib.lib, ops._stream(dev), _lib.torch_ops

    def done(self, status, inputs):
        torch.cuda.synchronize()
        assert status == 0, status
        for a in inputs:
            assert a.unchanged(), "an input was written"

    def ids(self, a):
        return Arr(self.dev, a, SENT_I)

    def t(self, a):
        return torch.from_numpy(np.ascontiguousarray(a)).to(self.dev)

    # -- gather-concat ------------------------------------------------------------------------
    def concat(self, src, dst, Fa, Fb, variant, want_form):
        lda, ldb, ldo, oa, ob, oo = variant
        E, W = src.size, Fa + Fb
        A, B = EC.bit_table(EC.N_A, Fa, lda, 1), EC.bit_table(EC.N_B, Fb, ldb, 2)
        s, d = self.ids(src), self.ids(dst)
        a, b = Arr(self.dev, A, EC.SPARE_BITS, oa), Arr(self.dev, B, EC.SPARE_BITS, ob)
        out = Arr(self.dev, np.full((E, ldo), EC.SENT_BITS, np.uint32), EC.SENT_BITS, oo)
        assert EC.concat_form(Fa, Fb, lda, ldb, ldo, a.ptr % 16, b.ptr % 16, out.ptr % 16) == want_form
        st = self.L.dgmi_gather_concat_f32(s.ptr, d.ptr, E, a.ptr, lda, Fa, b.ptr, ldb, Fb, out.ptr, ldo, self.stream)
        self.done(st, (s, d, a, b))
        want = EC.concat_reference(src, dst, A, Fa, B, Fb)
        assert out.holds_bits(_padded(want, ldo, EC.SENT_BITS)), (E, Fa, Fb, variant)
        return want, A, B

    # -- gather-add ---------------------------------------------------------------------------
    def add(self, src, dst, A, B, bias, bias_off, F, variant, act, want_vec):
        lda, ldb, ldo, oa, ob, oo = variant
        E = src.size
        s, d = self.ids(src), self.ids(dst)
        a, b = Arr(self.dev, A, EC.SPARE_BITS, oa), Arr(self.dev, B, EC.SPARE_BITS, ob)
        bi = None if bias is None else Arr(self.dev, bias, EC.SPARE_BITS, bias_off)
        out = Arr(self.dev, np.full((E, ldo), EC.SENT_F, np.float32), F_BITS, oo)
        form = EC.add_form(F, lda, ldb, ldo, a.ptr % 16, b.ptr % 16, out.ptr % 16, None if bi is None else bi.ptr % 16)
        assert form == (want_vec, bias is not None), (form, want_vec)
        st = self.L.dgmi_gather_add_f32(s.ptr, d.ptr, E, a.ptr, lda, b.ptr, ldb, None if bi is None else bi.ptr, F, out.ptr, ldo,
                                        act, self.stream)
        self.done(st, (s, d, a, b) + (() if bi is None else (bi,)))
        want = EC.add_reference(src, dst, A, B, bias, F, act)
        assert out.holds_values(_padded(want, ldo, F_BITS)), (E, F, variant, bias is not None, bias_off, act)
        return want


@pytest.fixture(scope="module")
def raw(dev):
    return _Raw(dev)


_CONCAT = [("pow2", a, b) for a, b in EC.POW2_WIDTHS] + [("vec4", a, b) for a, b in EC.VEC4_WIDTHS] \
    + [("dword", a, b) for a, b in EC.DWORD_WIDTHS]


# ---------------------------------------------------------------------------------------------
# (a) gather-concat and gather-add: widths, strides, misalignment, edge counts
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form,Fa,Fb", _CONCAT, ids=["%s-%d+%d" % c for c in _CONCAT])
def test_gather_concat_every_width_variant_and_edge_count(raw, form, Fa, Fb):
    """A plain call at every designed edge count of its kernel; 8 spare columns everywhere (NaN in the tables' spare
    columns) at the same counts; one leading dimension = 1 (mod 4) or one base 4 bytes off falls to the dword kernel with
    the same result."""
    W = (Fa + Fb) if form == "dword" else (Fa + Fb) // 4
    counts = EC.pow2_edge_counts(Fa, Fb) if form == "pow2" else EC.stride_edge_counts(W)
    variants = EC.concat_variants(Fa, Fb)
    for E in counts:
        src, dst = EC.edge_pairs(E, EC.N_A, EC.N_B)
        for name in ("plain", "strided"):
            raw.concat(src, dst, Fa, Fb, variants[name], form)
    for name, v in variants.items():
        if name in ("plain", "strided"):
            continue
        for E in (1, counts[-1]) + tuple(EC.stride_edge_counts(Fa + Fb)[2:4]):
            src, dst = EC.edge_pairs(E, EC.N_A, EC.N_B)
            raw.concat(src, dst, Fa, Fb, v, "dword")
    if Fa and Fb:  # the wrapper once per width: contiguous tables, the same bits
        src, dst = EC.edge_pairs(counts[-1], EC.N_A, EC.N_B)
        want, A, B = raw.concat(src, dst, Fa, Fb, variants["plain"], form)
        got = raw.T.gather_concat_raw(raw.t(src), raw.t(dst), raw.t(A.view(np.float32)), raw.t(B.view(np.float32)))
        assert np.array_equal(got.cpu().numpy().view(np.uint32), want)


@pytest.mark.parametrize("form,Fa,Fb", [("pow2", 128, 128), ("vec4", 344, 344), ("dword", 5, 7)])
def test_gather_concat_past_the_grid_cap(raw, form, Fa, Fb):
    """Just past 8192 blocks: the power-of-two kernel spans three strides (every slot loops once, three also take the
    tail; 67 MB), the other two start their second grid-stride trip (34 MB, 8 MB)."""
    E = EC.cap_edge_count(form, Fa, Fb)
    if form == "pow2":
        assert EC.pow2_geometry(E, Fa, Fb).strides == 3
    else:
        assert EC.stride_geometry(EC.concat_units(form, E, Fa, Fb)).capped
    src, dst = EC.edge_pairs(E, EC.N_A, EC.N_B)
    raw.concat(src, dst, Fa, Fb, EC.concat_variants(Fa, Fb)["plain"], form)


def _bias(F, kind):
    return (None, 0) if kind == "none" else (EC.int_table(1, F, F, 3)[0], 1 if kind == "off" else 0)


@pytest.mark.parametrize("F", EC.ADD_WIDTHS)
def test_gather_add_every_form_bias_and_activation(raw, F):
    """F x {plain, 8 spare columns} x bias {none, aligned, 4 bytes off} x act {0, 1} at every designed edge count; the
    variants that must fall to the dword form at two counts; `gather_add_raw` once."""
    variants = EC.add_variants(F)
    vec = 4 if F % 4 == 0 else 1
    counts = sorted(set(EC.stride_edge_counts(F // vec) + EC.stride_edge_counts(F)))
    for name, v in variants.items():
        A, B = EC.int_table(EC.N_A, F, v[0], 1), EC.int_table(EC.N_B, F, v[1], 2)
        plain = name in ("plain", "strided")
        for E in (counts if plain else (1, counts[-1])):
            src, dst = EC.edge_pairs(E, EC.N_A, EC.N_B)
            for kind in EC.BIAS_KINDS if plain else ("none", "aligned"):
                bias, boff = _bias(F, kind)
                for act in (0, 1):
                    want = raw.add(src, dst, A, B, bias, boff, F, v, act, vec if plain and kind != "off" else 1)
        if name == "plain":
            got = raw.T.gather_add_raw(raw.t(src), raw.t(dst), raw.t(A), raw.t(B), raw.t(bias), 1)
            assert EC.same_values(got.cpu().numpy(), want)


@pytest.mark.parametrize("F,vec", [(128, 4), (7, 1)])
def test_gather_add_past_the_grid_cap(raw, F, vec):
    E = EC.GRID_CAP * 256 // (F // vec) + 4
    assert EC.stride_geometry(E * (F // vec)).capped
    src, dst = EC.edge_pairs(E, EC.N_A, EC.N_B)
    A, B = EC.int_table(EC.N_A, F, F, 1), EC.int_table(EC.N_B, F, F, 2)
    raw.add(src, dst, A, B, _bias(F, "aligned")[0], 0, F, EC.add_variants(F)["plain"], 1, vec)


# ---------------------------------------------------------------------------------------------
# (b) gather-add on special values: torch.relu semantics
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("F", [128, 12, 7, 1])
def test_gather_add_relu_keeps_nan_and_infinities_like_torch(raw, F):
    """NaN, +inf, -inf, -0, +0, 3 and -3 in every column of seven rows of both tables, all 49 pairs: under act = 1 a NaN
    sum (NaN + x, inf - inf) stays NaN, -inf becomes 0, +inf stays — `torch.relu`, which the decoder's unfused path and
    the reference apply; every form (16-byte and dword, bias none / aligned / 4 bytes off)."""
    vec = 4 if F % 4 == 0 else 1
    for name in ("plain", "strided"):
        v = EC.add_variants(F)[name]
        A, B, src, dst = EC.special_tables(F, v[0], v[1])
        for kind in EC.BIAS_KINDS:
            bias, boff = _bias(F, kind)
            for act in (0, 1):
                want = raw.add(src, dst, A, B, bias, boff, F, v, act, vec if kind != "off" else 1)
                assert np.isnan(want[:7]).all() and np.isnan(want[9, 0]) and want[8, 0] == np.inf  # NaN + x, inf - inf, inf + inf
    A, B, src, dst = EC.special_tables(F, F, F)
    got = raw.T.gather_add_raw(raw.t(src), raw.t(dst), raw.t(A), raw.t(B), None, 1)
    assert EC.same_values(got.cpu().numpy(), EC.add_reference(src, dst, A, B, None, F, 1))
    x = raw.t(A)[raw.t(src).long(), :F] + raw.t(B)[raw.t(dst).long(), :F]
    assert EC.same_values(got.cpu().numpy(), torch.relu(x).cpu().numpy())


# ---------------------------------------------------------------------------------------------
# (c) epilogue backward
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", EC.EPILOGUE_N)
def test_epilogue_backward_on_every_sign_of_y(raw, n):
    """act 0 / 1 / 2, mask or none; Y positive, negative, +0, -0, NaN against every non-zero gradient and +-inf / NaN
    gradients, held to the formula of `dgmi.h`; n on both sides of a block and of the 4096-block grid."""
    dY, Y, mask = EC.epilogue_operands(n)
    for act in (0, 1, 2):
        for m in ((None, mask) if act != 2 else (None,)):
            d, y = Arr(raw.dev, dY, F_BITS), Arr(raw.dev, Y, F_BITS)
            mk = None if m is None else Arr(raw.dev, m, F_BITS)
            out = Arr(raw.dev, np.full(n, EC.SENT_F, np.float32), F_BITS)
            st = raw.L.dgmi_epilogue_backward_f32(d.ptr, y.ptr, None if mk is None else mk.ptr, n, act, EC.SLOPE, EC.MASK_SCALE,
                                                  out.ptr, raw.stream)
            raw.done(st, (d, y) + (() if mk is None else (mk,)))
            want = EC.epilogue_reference(dY, Y, m, act)
            assert out.holds_values(want), (n, act, m is not None)
            if n == 257:
                got = raw.T.epilogue_backward(raw.t(dY), raw.t(Y), None if m is None else raw.t(m), act, EC.SLOPE, EC.MASK_SCALE)
                assert EC.same_values(got.cpu().numpy(), want)


# ---------------------------------------------------------------------------------------------
# (d) column sums and their gradient
# ---------------------------------------------------------------------------------------------
def _colsum(raw, n, W, B, lda, ldc, ldo):
    A, coef = EC.colsum_operands(n, W, B, lda, ldc)
    want = _padded(EC.colsum_reference(A, coef, n, W), ldo, F_BITS)
    outs = []
    for _ in range(2):
        a, c = Arr(raw.dev, A, EC.SPARE_BITS), Arr(raw.dev, coef, EC.SPARE_BITS)
        out = Arr(raw.dev, np.full((B, ldo), EC.SENT_F, np.float32), F_BITS)
        st = raw.L.dgmi_weighted_colsum_f32(a.ptr if n else None, lda, c.ptr, ldc, n, W, B, out.ptr, ldo, raw.stream)
        raw.done(st, (a, c))
        assert out.holds_values(want), (n, W, B, lda)
        outs.append(out.read())
    assert np.array_equal(outs[0], outs[1])  # a second run is bit-identical
    if n == 0:
        assert not out.inner()[:, :W].any()


@pytest.mark.parametrize("n", EC.COLSUM_N)
def test_weighted_colsum_at_every_trip_and_tail_split(raw, n):
    """n on both sides of every 16- and 128-row changeover, W on both sides of a 64-column block, 1 / 3 / 64 blocks,
    leading dimensions larger than needed; n = 0 writes zeros with A = NULL; twice, bit-identical."""
    for W in EC.COLSUM_W:
        for B in EC.COLSUM_B:
            _colsum(raw, n, W, B, W + 3, n + 5, W + 7)
            if B == 3:
                _colsum(raw, n, W, B, W, n, W)


def _rank_add(raw, n, W, B, ldg, ldc, lds):
    G, coef, gs = EC.rank_add_operands(n, W, B, ldg, ldc, lds)
    want = G.copy()  # the spare columns stay as they are
    want[:, :W] = EC.rank_add_reference(G, coef, gs, n, W)
    outs = []
    for _ in range(2):
        g, c, s = Arr(raw.dev, G, F_BITS), Arr(raw.dev, coef, EC.SPARE_BITS), Arr(raw.dev, gs, EC.SPARE_BITS)
        st = raw.L.dgmi_rank_add_f32(g.ptr, ldg, c.ptr, ldc, s.ptr, lds, n, W, B, raw.stream)
        raw.done(st, (c, s))
        assert g.holds_values(want), (n, W, B)
        outs.append(g.read())
    assert np.array_equal(outs[0], outs[1])


@pytest.mark.parametrize("n", EC.COLSUM_N)
def test_rank_add_with_strided_operands(raw, n):
    """The spare columns of G (NaN) are neither read into a sum nor written."""
    for W in EC.COLSUM_W:
        for B in EC.COLSUM_B:
            _rank_add(raw, n, W, B, W + 3, n + 5, W + 7)
    _rank_add(raw, n, 65, 3, 65, n, 65)


def test_rank_add_past_its_grid_cap(raw):
    n, W = 3049, 344
    assert EC.stride_geometry(n * W, EC.EPILOGUE_CAP).capped
    _rank_add(raw, n, W, 3, W, n, W)


@pytest.mark.parametrize("i0", [1, 2])
def test_colsum_rows_layout_in_one_buffer(raw, i0):
    """The layout of `colsum_rows_`: every R-th row of `feat_ext` from row i0 on (lda = R W), the sums written to the B
    rows behind the n R rows of the SAME buffer; the gradient back onto those rows; both wrappers equal the raw calls."""
    n, R, W, B = 261, 3, 65, 3
    coef = EC.colsum_operands(n, W, B, W, n)[1]
    feat = EC.int_table(n * R, W, W, 29)  # rows u R + i0 are the summed ones
    ext = np.concatenate([feat, np.full((B, W), EC.SENT_F, np.float32)])
    want = ext.copy()
    want[n * R:] = (coef.astype(np.float64) @ feat[i0::R].astype(np.float64)).astype(np.float32)
    f, c = Arr(raw.dev, ext, F_BITS), Arr(raw.dev, coef, EC.SPARE_BITS)
    st = raw.L.dgmi_weighted_colsum_f32(f.ptr + 4 * i0 * W, R * W, c.ptr, n, n, W, B, f.ptr + 4 * n * R * W, W, raw.stream)
    raw.done(st, (c,))
    assert f.holds_values(want)
    t = raw.t(ext)
    raw.T.colsum_rows_(t, raw.t(coef), n, R, i0)
    assert np.array_equal(t.cpu().numpy(), want)
    gs = EC.int_table(B, W, W, 23)
    gwant = feat.copy()
    gwant[i0::R] = EC.rank_add_reference(feat[i0::R], coef, gs, n, W)
    g, s = Arr(raw.dev, feat, F_BITS), Arr(raw.dev, gs, EC.SPARE_BITS)
    st = raw.L.dgmi_rank_add_f32(g.ptr + 4 * i0 * W, R * W, c.ptr, n, s.ptr, W, n, W, B, raw.stream)
    raw.done(st, (c, s))
    assert g.holds_values(gwant)
    t = raw.t(feat)
    raw.T.colsum_rows_backward_(t, raw.t(coef), raw.t(gs), n, R, i0)
    assert np.array_equal(t.cpu().numpy(), gwant)


# ---------------------------------------------------------------------------------------------
# (e) row pre-scale
# ---------------------------------------------------------------------------------------------
_SCALE = [(300, 128, 128, 128, 0, 0, 4), (300, 128, 136, 140, 0, 0, 4), (300, 128, 133, 128, 0, 0, 1), (300, 128, 128, 129, 0, 0, 1),
          (300, 128, 128, 128, 1, 0, 1), (300, 128, 128, 128, 0, 1, 1), (300, 7, 7, 9, 0, 0, 1), (1, 4, 4, 4, 0, 0, 4), (1, 1, 1, 1, 0, 0, 1),
          (65_600, 128, 128, 128, 0, 0, 4), (16_400, 128, 128, 128, 1, 0, 1), (0, 128, 128, 128, 0, 0, 4)]


@pytest.mark.parametrize("n,F,ldx,ldo,offx,offo,vec", _SCALE)
def test_scale_rows_both_forms_strided(raw, n, F, ldx, ldo, offx, offo, vec):
    """Both forms, strided in and out, bases 4 bytes off, past 8192 blocks in either form, n = 0 (nothing written)."""
    X, scale = EC.scale_operands(n, F, ldx)
    x, s = Arr(raw.dev, X, EC.SPARE_BITS, offx), Arr(raw.dev, scale, F_BITS)
    out = Arr(raw.dev, np.full((n, ldo), EC.SENT_F, np.float32), F_BITS, offo)
    assert EC.scale_form(F, ldx, ldo, x.ptr % 16, out.ptr % 16) == vec
    if n > 300:
        assert EC.stride_geometry(n * F // vec).capped
    st = raw.L.dgmi_scale_rows_f32(x.ptr, ldx, s.ptr, n, F, out.ptr, ldo, raw.stream)
    raw.done(st, (x, s))
    want = EC.scale_reference(X, scale, n, F)
    assert out.holds_values(_padded(want, ldo, F_BITS))
    if (n, ldx) == (300, 128) and not offx and not offo:
        assert np.array_equal(raw.T.scale_rows(raw.t(X), raw.t(scale)).cpu().numpy(), want)


@pytest.mark.parametrize("F,ld,vec", [(128, 136, 4), (7, 9, 1)])
def test_scale_rows_in_place(raw, F, ld, vec):
    """`out` may be X: the spare columns (NaN) stay as they are."""
    n = 300
    X, scale = EC.scale_operands(n, F, ld)
    x, s = Arr(raw.dev, X, EC.SPARE_BITS), Arr(raw.dev, scale, F_BITS)
    assert EC.scale_form(F, ld, ld, x.ptr % 16, x.ptr % 16) == vec
    st = raw.L.dgmi_scale_rows_f32(x.ptr, ld, s.ptr, n, F, x.ptr, ld, raw.stream)
    raw.done(st, (s,))
    want = X.copy()
    want[:, :F] = EC.scale_reference(X, scale, n, F)
    assert x.holds_values(want)


# ---------------------------------------------------------------------------------------------
# (f) row scale x multiplicity
# ---------------------------------------------------------------------------------------------
def _multiplicity(raw, indptr, vals):
    n_rows = indptr.size - 1
    ip, v = Arr(raw.dev, indptr, SENT_I), Arr(raw.dev, vals, F_BITS)
    scale = Arr(raw.dev, np.full(n_rows, EC.SENT_F, np.float32), F_BITS)
    mult = Arr(raw.dev, np.full(vals.size, SENT_I, np.int32), SENT_I)
    fail = Arr(raw.dev, np.full(1, SENT_I, np.int32), SENT_I)
    st = raw.L.dgmi_row_multiplicity_f32(ip.ptr, v.ptr, n_rows, vals.size, EC.REL_TOL, scale.ptr, mult.ptr, fail.ptr, raw.stream)
    raw.done(st, (ip, v))
    return scale, mult, fail


_MULT = EC.multiplicity_cases()


@pytest.mark.parametrize("name", sorted(_MULT))
def test_row_multiplicity_on_the_designed_rows(raw, name):
    """`row_scale`, `mult` and `fail` exact; `mult` 0 on every position of a failed row, `row_scale` 0 for empty and failed
    rows; every other row as in the case without the failed one."""
    from dream_gnn_amd import ops

    want = EC.multiplicity_case(_MULT[name])
    assert ops.MULT_REL_TOL == EC.REL_TOL
    scale, mult, fail = _multiplicity(raw, want.indptr, want.vals)
    bad = [want.names[i] for i in np.flatnonzero(scale.inner() != want.row_scale)]
    assert scale.holds_bits(want.row_scale) and not bad, bad
    assert mult.holds_bits(want.mult), [want.names[i] for i in np.unique(np.searchsorted(want.indptr, np.flatnonzero(
        mult.inner(np.int32) != want.mult), side="right") - 1)]
    assert fail.holds_bits(np.array([want.fail], np.int32))
    s2, m2, f2 = raw.T.row_multiplicity(raw.t(want.indptr), raw.t(want.vals), EC.REL_TOL)
    assert np.array_equal(s2.cpu().numpy(), want.row_scale) and np.array_equal(m2.cpu().numpy(), want.mult) and int(f2) == want.fail


def test_row_multiplicity_on_a_reference_built_adjacency_with_long_rows(raw):
    """D^-1 (A + A^T + I), every row past 64 values: the scale is the row's smallest value, `mult` the known m - 1."""
    indptr, vals, m = EC.reference_adjacency()
    scale, mult, fail = _multiplicity(raw, indptr, vals)
    assert fail.holds_bits(np.zeros(1, np.int32)) and mult.holds_bits(m - 1)
    assert scale.holds_bits(np.minimum.reduceat(vals, indptr[:-1]))


# ---------------------------------------------------------------------------------------------
# (g) selection
# ---------------------------------------------------------------------------------------------
class _Select:
    def __init__(self, raw):
        self.raw, self.L = raw, raw.L
        self.need = int(self.L.dgmi_random_subset_workspace_bytes())

    def _ws(self):
        return torch.full((self.need + BAND,), BAND_BYTE, dtype=torch.uint8, device=self.raw.dev)

    def _finish(self, st, ws, descs, n):
        torch.cuda.synchronize()
        assert st == 0, st
        assert bool((ws[self.need:] == BAND_BYTE).all()), "the call wrote past the workspace size it reports"
        got = descs.read()
        assert np.all(got[:descs.lo] == SENT_I) and np.all(got[descs.lo + 8 * n:] == SENT_I)
        return descs.inner(np.int32).reshape(n, 8)

    def one(self, E, keep, seed, off=0):
        ws, d = self._ws(), Arr(self.raw.dev, np.full(8, SENT_I, np.int32), SENT_I)
        st = self.L.dgmi_random_subset_select(E, keep, seed, off, d.ptr, ws.data_ptr(), self.need, self.raw.stream)
        return self._finish(st, ws, d, 1)[0]

    def batch(self, Es, keeps, seeds, offs, device_seeds=False):
        n = len(Es)
        ws, d = self._ws(), Arr(self.raw.dev, np.full(8 * n, SENT_I, np.int32), SENT_I)
        e, k = (ctypes.c_int64 * n)(*Es), (ctypes.c_int64 * n)(*keeps)
        s, o = (ctypes.c_uint64 * n)(*seeds), (ctypes.c_uint32 * n)(*offs)
        if device_seeds:
            sd = self.raw.t(np.array(seeds, np.uint64).view(np.int64))
            st = self.L.dgmi_random_subset_select_batch_dseed(n, ctypes.addressof(e), ctypes.addressof(k), sd.data_ptr(),
                                                              ctypes.addressof(o), d.ptr, ws.data_ptr(), self.need, self.raw.stream)
        else:
            st = self.L.dgmi_random_subset_select_batch(n, ctypes.addressof(e), ctypes.addressof(k), ctypes.addressof(s),
                                                        ctypes.addressof(o), d.ptr, ws.data_ptr(), self.need, self.raw.stream)
        return self._finish(st, ws, d, n)

    def mask(self, desc, E):
        d = Arr(self.raw.dev, desc, SENT_I)
        m = Arr(self.raw.dev, np.full(E, EC.SENT_F, np.float32), F_BITS)
        st = self.L.dgmi_keep_mask_f32(d.ptr, 1, E, m.ptr, self.raw.stream)
        self.raw.done(st, (d,))
        return m


@pytest.fixture(scope="module")
def sel(raw):
    return _Select(raw)


def _check_list(sel, E, keep, seed, with_mask):
    want = EC.select_description(E, keep, seed)
    got = sel.one(E, keep, seed)
    assert np.array_equal(got, want), (E, keep, seed, got, want)
    if with_mask:
        m = sel.mask(want, E)
        assert m.holds_bits(EC.select_mask(E, keep, seed)) and float(m.inner().sum()) == keep


@pytest.mark.parametrize("narrow", [0, 1])
@pytest.mark.parametrize("E", EC.EDGE_E)
def test_selection_on_both_sides_of_the_window_threshold(sel, E, narrow):
    """65 535 edges: the workgroup select; 65 536 and 65 537: the window passes, with keep = 1, 2, E - 2, E - 1 at the
    window's clamped ends; with `select_narrow_window` the window misses and the workgroup takes over.  Equal to the host
    `lexsort` description, and `keep_mask` sums to keep."""
    from dream_gnn_amd import _lib

    _lib.set_tuning("select_narrow_window", narrow)
    try:
        for keep in EC.edge_keeps(E):
            for seed in EC.SELECT_SEEDS:
                _check_list(sel, E, keep, seed, with_mask=not narrow and seed == EC.SELECT_SEEDS[1])
    finally:
        _lib.set_tuning("select_narrow_window", 0)


@pytest.mark.parametrize("E", EC.SMALL_WINDOW_E)
def test_selection_of_short_lists_through_the_window_passes(sel, E):
    """`select_window_min` = 2: the window is clamped at both ends of the hash space (lo = 0, bins wider than 2^20)."""
    from dream_gnn_amd import _lib

    _lib.set_tuning("select_window_min", 2)
    try:
        for keep in EC.small_window_keeps(E):
            for seed in EC.SELECT_SEEDS:
                _check_list(sel, E, keep, seed, with_mask=seed == 0)
        if E == 2:  # the keep-th key in the last bin: its upper end is clamped to 0xffffffff
            for e, keep in EC.LAST_BIN_CASES:
                _check_list(sel, e, keep, EC.LAST_BIN_SEED, with_mask=True)
    finally:
        _lib.set_tuning("select_window_min", 0)


def test_selection_batch_of_eight_with_host_and_device_seeds(sel):
    """Window lists, block lists, keep 0 and keep E in one series of launches == single calls == the host description;
    once more with the seeds in device memory, and through `ops.random_subset_select_batch` both ways."""
    from dream_gnn_amd import ops

    b = EC.BATCH
    want = np.stack([EC.select_description(*a) for a in zip(b["E"], b["keep"], b["seed"], b["off"])])
    assert np.array_equal(sel.batch(b["E"], b["keep"], b["seed"], b["off"]), want)
    assert np.array_equal(sel.batch(b["E"], b["keep"], b["seed"], b["off"], device_seeds=True), want)
    for i in range(8):
        assert np.array_equal(sel.one(b["E"][i], b["keep"][i], b["seed"][i], b["off"][i]), want[i]), i
    assert np.array_equal(ops.random_subset_select_batch(b["E"], b["keep"], b["seed"], sel.raw.dev, b["off"]).cpu().numpy(), want)
    seeds = sel.raw.t(np.array(b["seed"], np.uint64).view(np.int64))
    assert np.array_equal(ops.random_subset_select_batch(b["E"], b["keep"], seeds, sel.raw.dev, b["off"]).cpu().numpy(), want)
