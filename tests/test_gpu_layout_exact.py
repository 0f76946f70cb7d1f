"""The integer passes that build every layout, through the C ABI with buffers the test owns — ZERO tolerance:
the record radix sort (``csrc/dgmi_sort.hip``), COO -> CSR, COO -> sliced, CSR -> sliced (``csrc/dgmi_csr.hip``), the
per-step compaction (``csrc/dgmi_compact.hip``) and ``dgmi_gather_f32``, on the designed inputs of ``_layout_cases.py``.

Every call makes three assertions: every output element equals the reference; what the call must not write is still the
sentinel the buffer was filled with (``indices_out[nk:]``, ``vals_out[nk:]``, the elements past every array's end, and
with ``E = 0`` everything but the pointers); the workspace is 4 KiB larger than the size query says, the query's value is
what the call is told, and the extra 4 KiB are unchanged afterwards.  The ``ops`` wrappers are held to the raw calls once
per group.  Ids are in range everywhere (the range flag is asserted 0)."""
import ctypes

import numpy as np
import pytest
import torch

import _layout_cases as LC

pytestmark = pytest.mark.gpu

SENT = -0x2A2A2A2B   # no id, pointer or edge id is negative
BAND = 4096
BAND_BYTE = 0xA5
GUARD = 64           # elements past the end of every output array


@pytest.fixture(scope="module", autouse=True)
def _tile_order_back():
    from dream_gnn_amd import _lib

    yield
    _lib.set_tuning("sort_plain_tiles", 0)


def _t(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _out(n, dev):
    return torch.full((n + GUARD,), SENT, dtype=torch.int32, device=dev)


def _untouched(buf, n):
    return bool((buf[n:] == SENT).all())


class _Raw:
    """The five entry points with test-owned outputs and workspace."""

    def __init__(self, dev):
        from dream_gnn_amd import _lib, ops

        self.dev, self.L, self.stream = dev, _lib.lib, ops._stream(dev)

    def _finish(self, status, ws, need, outs, flag=True):
        torch.cuda.synchronize()
        assert status == 0, status
        assert bool((ws[need:] == BAND_BYTE).all()), "the call wrote past the workspace size it reports"
        if flag:
            assert int(ws[:4].view(torch.int32)) == 0  # the range flag: every id is in range
        for buf, n in outs:
            assert _untouched(buf, n), "an output was written past its end"
        return [buf[:n] for buf, n in outs]

    def _ws(self, need):
        return torch.full((need + BAND,), BAND_BYTE, dtype=torch.uint8, device=self.dev)

    def csr(self, row, col, n_rows, n_cols):
        E, need = row.numel(), ctypes.c_size_t(0)
        assert self.L.dgmi_csr_from_coo_i32(None, None, E, n_rows, n_cols, None, None, None, None, ctypes.byref(need), None) == 0
        assert need.value == LC.csr_from_coo_workspace(E, n_rows)
        ws, have = self._ws(need.value), ctypes.c_size_t(need.value)
        outs = [(_out(n_rows + 1, self.dev), n_rows + 1), (_out(E, self.dev), E), (_out(E, self.dev), E)]
        st = self.L.dgmi_csr_from_coo_i32(row.data_ptr(), col.data_ptr(), E, n_rows, n_cols, outs[0][0].data_ptr(),
                                          outs[1][0].data_ptr(), outs[2][0].data_ptr(), ws.data_ptr(), ctypes.byref(have), self.stream)
        return self._finish(st, ws, need.value, outs)

    def sliced_coo(self, row, col, n_rows, n_cols, n_slices):
        E, need = row.numel(), ctypes.c_size_t(0)
        assert self.L.dgmi_csr_sliced_from_coo_i32(None, None, E, n_rows, n_cols, n_slices, None, None, None, None,
                                                   ctypes.byref(need), None) == 0
        assert need.value == LC.sliced_from_coo_workspace(E, n_rows, n_slices)
        ws, have = self._ws(need.value), ctypes.c_size_t(need.value)
        nk = n_rows * n_slices + 1
        outs = [(_out(nk, self.dev), nk), (_out(E, self.dev), E), (_out(E, self.dev), E)]
        st = self.L.dgmi_csr_sliced_from_coo_i32(row.data_ptr(), col.data_ptr(), E, n_rows, n_cols, n_slices, outs[0][0].data_ptr(),
                                                 outs[1][0].data_ptr(), outs[2][0].data_ptr(), ws.data_ptr(), ctypes.byref(have),
                                                 self.stream)
        return self._finish(st, ws, need.value, outs)

    def sliced_csr(self, indptr, indices, eid, n_rows, n_cols, n_slices):
        E, need = indices.numel(), ctypes.c_size_t(0)
        assert self.L.dgmi_csr_sliced_from_csr_i32(None, None, None, E, n_rows, n_cols, n_slices, None, None, None, None,
                                                   ctypes.byref(need), None) == 0
        assert need.value == LC.sliced_from_csr_workspace(E, n_slices)
        ws, have = self._ws(need.value), ctypes.c_size_t(need.value)
        nk = n_rows * n_slices + 1
        outs = [(_out(nk, self.dev), nk), (_out(E, self.dev), E), (_out(E, self.dev), E)]
        st = self.L.dgmi_csr_sliced_from_csr_i32(indptr.data_ptr(), indices.data_ptr(), eid.data_ptr(), E, n_rows, n_cols, n_slices,
                                                 outs[0][0].data_ptr(), outs[1][0].data_ptr(), outs[2][0].data_ptr(), ws.data_ptr(),
                                                 ctypes.byref(have), self.stream)
        return self._finish(st, ws, need.value, outs)

    def compact(self, ptr, indices, vals, eid, table, nk):
        """(ptr_out, indices_out[:nk], vals_out[:nk] as int32 bits); everything from nk on must still be the sentinel."""
        nnz, need = indices.numel(), self.L.dgmi_compact_layout_workspace_bytes(indices.numel())
        assert need == LC.compact_workspace_bytes(nnz)
        ws = self._ws(need)
        outs = [(_out(ptr.numel(), self.dev), ptr.numel()), (_out(nnz, self.dev), nk)]
        if vals is not None:
            outs.append((_out(nnz, self.dev), nk))
        st = self.L.dgmi_compact_layout_i32(ptr.data_ptr(), ptr.numel(), indices.data_ptr(), None if vals is None else vals.data_ptr(),
                                            eid.data_ptr(), nnz, table.data_ptr(), table.shape[0], outs[0][0].data_ptr(),
                                            outs[1][0].data_ptr(), None if vals is None else outs[2][0].data_ptr(), ws.data_ptr(),
                                            need, self.stream)
        got = self._finish(st, ws, need, outs, flag=False)
        return got if vals is not None else got + [None]


@pytest.fixture(scope="module")
def raw(dev):
    return _Raw(dev)


def _same(got, want, dev, what):
    for g, w, name in zip(got, want, ("pointers", "indices", "eid")):
        w = w if torch.is_tensor(w) else _t(np.asarray(w, np.int32), dev)
        assert g.shape == w.shape and torch.equal(g, w), (what, name)


def _slices_for(n_rows):
    return (8, 3, 1, 64) if n_rows <= 2 ** 17 + 1 else (8, 3, 1)  # 64 x 2^18 keys and more: the four-pass case alone


def _check_builders(raw, oracle, dev, rows, cols, n_rows, n_cols, slices, what, wrappers=False):
    """CSR, sliced from COO and sliced from that CSR == the oracle and each other, under both tile orders."""
    from dream_gnn_amd import _lib, ops

    r, c = _t(rows, dev), _t(cols, dev)
    want_csr = oracle.csr_from_coo(rows, cols, n_rows)
    want_sl = {s: oracle.csr_sliced_from_coo(rows, cols, n_rows, n_cols, s) for s in slices}
    want_sl = {s: [_t(a, dev) for a in w] for s, w in want_sl.items()}
    for plain in (0, 1):
        _lib.set_tuning("sort_plain_tiles", plain)
        csr = raw.csr(r, c, n_rows, n_cols)
        _same(csr, want_csr, dev, (what, "csr", plain))
        for s in slices:
            a = raw.sliced_coo(r, c, n_rows, n_cols, s)
            b = raw.sliced_csr(csr[0], csr[1], csr[2], n_rows, n_cols, s)
            _same(a, want_sl[s], dev, (what, "sliced from COO", s, plain))
            _same(b, want_sl[s], dev, (what, "sliced from CSR", s, plain))
    _lib.set_tuning("sort_plain_tiles", 0)
    if wrappers:
        ip, ix, ei, flag = ops.csr_from_coo(r, c, n_rows, n_cols, return_flag=True)
        _same((ip, ix, ei), csr, dev, (what, "ops.csr_from_coo"))
        assert int(flag) == 0
        s = slices[0]
        a = ops.SlicedCSR(r, c, n_rows, n_cols, n_slices=s)
        b = ops.SlicedCSR.from_csr(ip, ix, ei, n_rows, n_cols, n_slices=s)
        for got in (a, b):
            _same((got.segptr, got.indices, got.eid), want_sl[s], dev, (what, "ops.SlicedCSR", s))
            assert int(got.range_flag) == 0


# ---------------------------------------------------------------------------------------------
# (a) the sort through all three builders
# ---------------------------------------------------------------------------------------------
_SORT_CASES = LC.sort_design_cases() + LC.sort_edge_cases()


@pytest.mark.parametrize("kind,E,n_rows,background", _SORT_CASES,
                         ids=["%s-%d-%d%s" % (k, E, n, "-bg" if bg else "") for k, E, n, bg in _SORT_CASES])
def test_sort_key_designs_through_every_builder(raw, oracle, dev, kind, E, n_rows, background):
    rows = LC.design_rows(kind, E, n_rows)
    if background:
        rows = LC.over_random(rows, n_rows, E + n_rows)
    n_cols = 50_000
    _check_builders(raw, oracle, dev, rows, LC.columns(E, n_cols), n_rows, n_cols, _slices_for(n_rows), (kind, E, n_rows),
                    wrappers=(kind, E) in (("lane_edges", 65_537), ("round_robin", 8193)))


@pytest.mark.parametrize("n_rows,p", [(n, p) for n in (1024, 2 ** 19, 2 ** 20) for p in range(len(LC.sort_passes(0, LC.bits_for(n))))])
def test_sort_one_digit_per_pass(raw, oracle, dev, n_rows, p):
    """Keys that differ in ONE pass's digit only, which takes every value 0 … 2^bits - 1 (10-, 19- and 20-bit plans; the
    row count is 2^bits so that the top digit's largest value is a row)."""
    E, n_cols = 8193, 50_000
    rows = LC.design_rows("one_digit", E, n_rows, p)
    _check_builders(raw, oracle, dev, rows, LC.columns(E, n_cols), n_rows, n_cols, (8, 3), ("one_digit", n_rows, p))


def test_sort_four_digit_passes(raw, oracle, dev):
    """64 slices x 2 100 000 rows: 134.4 M keys, 28 bits, four passes of 7.  The 538 MB segptr is compared on the device
    with ``torch.searchsorted`` over the oracle's sorted keys; ids and eid with the oracle's."""
    from dream_gnn_amd import _lib

    n_rows, n_cols, n_slices, E = (LC.FOUR_PASS[k] for k in ("n_rows", "n_cols", "n_slices", "E"))
    assert LC.sort_passes(0, LC.bits_for(n_rows * n_slices)) == [(0, 7), (7, 7), (14, 7), (21, 7)]
    rows, cols, key, order = LC.four_pass_case()
    values = torch.arange(n_rows * n_slices + 1, dtype=torch.int32, device=dev)
    want_ptr = torch.searchsorted(_t(key[order].astype(np.int32), dev), values, out_int32=True)
    del values
    want = (want_ptr, cols[order], order)
    r, c = _t(rows, dev), _t(cols, dev)
    csr = raw.csr(r, c, n_rows, n_cols)
    _same(csr, oracle.csr_from_coo(rows, cols, n_rows), dev, "csr")
    for plain in (0, 1):
        _lib.set_tuning("sort_plain_tiles", plain)
        _same(raw.sliced_coo(r, c, n_rows, n_cols, n_slices), want, dev, ("four passes, from COO", plain))
    _lib.set_tuning("sort_plain_tiles", 0)
    _same(raw.sliced_csr(csr[0], csr[1], csr[2], n_rows, n_cols, n_slices), want, dev, "from CSR")


# ---------------------------------------------------------------------------------------------
# (b) boundaries
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("first,last_gap,e_mod", [(0, 0, 63), (64, 64, 0), (70, 65, 63), (0, 300, 0)])
def test_boundaries_on_the_gap_design(raw, oracle, dev, first, last_gap, e_mod):
    """Gaps of 1, 2, 63 … 67, 129 and 5000 empty keys at every lane, three long ones inside one wave with lanes 0 and 63
    among them, a long gap at p = 0 and at p = E, E + 1 a multiple of 64 and one more."""
    n_rows, n_cols = 100_000, 50_000
    rows = LC.gap_design(n_rows, first, last_gap, e_mod)
    _check_builders(raw, oracle, dev, rows, LC.columns(rows.size, n_cols), n_rows, n_cols, (), ("gaps", first, last_gap))
    for s in (8, 3):  # an empty leading slice, empty trailing slices
        _check_builders(raw, oracle, dev, rows, LC.gap_columns(rows.size, n_cols, s), n_rows, n_cols, (s,), ("gaps", s),
                        wrappers=first == 70)


@pytest.mark.parametrize("E", [0, 1])
def test_boundaries_with_no_edge_and_one(raw, oracle, dev, E):
    """E = 0: position 0 alone fills all 100 001 (800 001) pointers wave-wide, and nothing but the pointers is written."""
    n_rows, n_cols = 100_000, 50_000
    rows, cols = np.full(E, 31_337, np.int32), np.full(E, 49_999, np.int32)
    _check_builders(raw, oracle, dev, rows, cols, n_rows, n_cols, (8, 3, 1), ("E", E), wrappers=True)


def test_from_csr_wrapper_surfaces_the_refused_shape(dev):
    """33 slices x (2^25 + 1) rows: the position key would need 32 bits.  `SlicedCSR.from_csr` raises with the status
    text, before anything is built (the COO constructor's key is slice * n_rows + row and is not affected)."""
    from dream_gnn_amd import ops

    n_rows = 2 ** 25 + 1
    indptr = torch.zeros(n_rows + 1, dtype=torch.int32, device=dev)
    none = torch.zeros(0, dtype=torch.int32, device=dev)
    with pytest.raises(RuntimeError, match=r"size query\) failed: .*\(status -2\)"):
        ops.SlicedCSR.from_csr(indptr, none, none, n_rows, 1000, n_slices=33)
    small = ops.SlicedCSR.from_csr(indptr[:1001], none, none, 1000, 1000, n_slices=33)  # the same call at an admitted shape
    assert small.segptr.numel() == 33 * 1000 + 1 and int(small.segptr.max()) == 0 and int(small.range_flag) == 0


# ---------------------------------------------------------------------------------------------
# (c) position keys
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("E", [2 ** 18 - 1, 2 ** 18, 2 ** 18 + 3])
def test_position_keys_on_the_chunk_design(raw, oracle, dev, E):
    """A row ending at every offset of an 8-chunk followed by 0 … 6 and 70 empty rows (walk of 1 … 4 steps, search beyond),
    a chunk inside a 100-edge row, an empty first row, empty last rows; 2^18 - 1 takes the one-position kernel."""
    indptr = LC.chunk_prefix(LC.chunk_design()[0], E)
    n_rows, n_cols = indptr.size - 1, 5000
    rows = LC.rows_of(indptr)
    assert rows.size == E
    _check_builders(raw, oracle, dev, rows, LC.columns(E, n_cols), n_rows, n_cols, (8, 3, 1), ("chunks", E), wrappers=E == 2 ** 18 + 3)


# ---------------------------------------------------------------------------------------------
# (d) compaction
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nnz", [1, 63, 64, 65, 4095, 4096, 4097, 12_289])
def test_compaction_on_the_word_design(raw, dev, nnz):
    """Words all kept, all dropped, bit 0 only, bit 63 only, all but those, alternating, random; a tile wholly dropped and
    one wholly kept; a partial last word; pointers on and next to every word and tile edge; values with NaN payloads, both
    zeros and infinities compared as bits; under 1, 2 and 3 descriptions and an inverted one, with and without values."""
    from dream_gnn_amd import _lib

    for kind in LC.TABLE_KINDS:
        d = LC.word_design(nnz, kind)
        ptr, idx, eid, table = _t(d.ptr, dev), _t(d.indices, dev), _t(d.eid, dev), _t(d.table, dev)
        vals = _t(d.vals.view(np.int32), dev)
        for with_vals in (False, True):
            p, i, v = raw.compact(ptr, idx, vals if with_vals else None, eid, table, d.nk)
            _same((p, i), (d.want_ptr, d.want_indices), dev, (nnz, kind, with_vals))
            if with_vals:
                assert torch.equal(v, _t(d.want_vals.view(np.int32), dev)), (nnz, kind)
    p2, i2, v2 = _lib.torch_ops.compact_layout(ptr, idx, vals.view(torch.float32), eid, table)
    assert torch.equal(p2, p) and torch.equal(i2[:d.nk], i) and torch.equal(v2.view(torch.int32)[:d.nk], v)


# ---------------------------------------------------------------------------------------------
# (e) one grid-stride and carry case per pass, at the smallest size that reaches it
# ---------------------------------------------------------------------------------------------
def test_sort_carry_across_scan_chunks_and_builder_grid_strides(raw, oracle, dev):
    """E = 8 388 609: 1025 tiles (the second chunk of `sort_bucket_scan_kernel`), above 524 288 positions (the strides of
    `slice_key_kernel` and `boundaries_kernel`) and above 4 194 304 (the stride of `position_key_kernel<8>`)."""
    E, n_rows, n_cols = 8_388_609, 100_000, 50_000
    assert LC.sort_tiles(E) == LC.SCAN_CHUNK + 1 and E > LC.GRID_CAP * LC.GRID_BLOCK * 8
    rows = LC.over_random(LC.design_rows("round_robin", E, n_rows), n_rows, 1)
    cols = LC.columns(E, n_cols)
    r, c = _t(rows, dev), _t(cols, dev)
    csr = raw.csr(r, c, n_rows, n_cols)
    _same(csr, oracle.csr_from_coo(rows, cols, n_rows), dev, "csr")
    want = oracle.csr_sliced_from_coo(rows, cols, n_rows, n_cols, 8)
    _same(raw.sliced_coo(r, c, n_rows, n_cols, 8), want, dev, "sliced from COO")
    _same(raw.sliced_csr(csr[0], csr[1], csr[2], n_rows, n_cols, 8), want, dev, "sliced from CSR")


def test_compaction_second_scan_sweep(raw, dev):
    """nnz = 33 554 433: 8193 tiles, the second sweep of `compact_scan_kernel`.  eid = position; hand-made "drop all" /
    "keep all" words over ranges that end on and next to word and tile edges and on both sides of position 8192 * 4096;
    the expectation is a concatenation of ranges made on the device, the pointers' ranks host arithmetic."""
    nnz = LC.BIG_NNZ
    assert LC.compact_geometry(nnz)["sweeps"] == 2
    pos = torch.arange(nnz, dtype=torch.int32, device=dev)
    drops, _ = LC.big_ranges(nnz)
    kept, at = [], 0
    for b, e in drops:
        kept.append(pos[at:b])
        at = e
    kept.append(pos[at:])
    want = torch.cat(kept)
    probes = LC.big_probes(nnz)
    p, i, v = raw.compact(_t(probes, dev), pos, pos, pos, _t(LC.big_table(nnz), dev), want.numel())
    assert torch.equal(p, _t(LC.big_rank(probes, nnz), dev))
    assert torch.equal(i, want) and torch.equal(v, want)
    assert int(p[-1]) == want.numel() == nnz - sum(e - b for b, e in drops)


def test_gather_f32_grid_stride(dev):
    from dream_gnn_amd import _lib, ops

    n = LC.GRID_CAP * LC.GRID_BLOCK + 77
    table = torch.randn(1000, device=dev)
    perm = _t(LC.columns(n, 1000), dev)
    out = torch.full((n + GUARD,), float("nan"), device=dev)
    assert _lib.lib.dgmi_gather_f32(table.data_ptr(), perm.data_ptr(), n, out.data_ptr(), ops._stream(dev)) == 0
    torch.cuda.synchronize()
    assert torch.equal(out[:n], table[perm.long()]) and bool(torch.isnan(out[n:]).all())
    assert torch.equal(ops.gather_f32(table, perm), out[:n])
