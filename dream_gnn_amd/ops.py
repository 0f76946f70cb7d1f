"""Graph-level layer over the ``dreamgnn_mi`` dispatcher ops (``csrc/dgmi_torch.cpp``), which in turn
are thin bindings of the C ABI (``include/dgmi.h``).

PyTorch is plumbing here: it owns device memory and the stream; the arithmetic is
``libdgmi.so``.  Every op requires HIP ("cuda") tensors and raises otherwise.  This module adds
what a functional op cannot hold: the layouts of one graph (CSR, transposed CSR, XCD-sliced, their
launch plans), built once and cached; the kernel choice per product; value and edge-dropout
views; autograd at the graph level.

Boundary being replaced (reference ``/root/reference/layers.py``):
  * ``graph.update_all(fn.copy_u('h','m'), fn.sum('m','h'))``  — layers.py:229-232
  * ``th.spmm(adj, support)``                                   — layers.py:312
"""
from __future__ import annotations

import contextlib
import ctypes
import operator
import os
import threading
from typing import Optional, Tuple

import torch

from . import _lib

_L = _lib.lib          # ctypes view of the C ABI: host-only size / geometry queries
_T = _lib.torch_ops    # torch.ops.dreamgnn_mi: the dispatcher ops the kernels are launched through
_NULLCTX = contextlib.nullcontext()
#: output epilogue of a product: (act, slope, out_mask, mask_scale) — act 0 none / 1 leaky-relu(slope);
#: out_mask: 0/1 keep mask of the output (dropout), multiplied in with mask_scale = 1 / (1 - p)
_NO_EPI = (0, 0.0, None, 1.0)

# Precision of the GATHERED operand of the XCD-local products.  float32: the table as it is; bfloat16: a
# bf16 copy made by one streaming pass (`rows_to_bf16`, source scale folded in, one round-to-nearest-even) — sums, planes
# and outputs stay float32.  A product asks with `gather_dtype=`; calls that pass none take the thread's default.
_GATHER_DTYPES = (torch.float32, torch.bfloat16)
_gather_default = threading.local()


def _check_gather_dtype(dtype):
    if dtype is not None and dtype not in _GATHER_DTYPES:
        raise ValueError("gather_dtype must be None, torch.float32 or torch.bfloat16, got %r" % (dtype,))
    return dtype


def _resolve_gather_dtype(dtype):
    """``dtype`` if given, else the default of :func:`gather_precision` on this thread, else float32."""
    if _check_gather_dtype(dtype) is not None:
        return dtype
    return getattr(_gather_default, "dtype", None) or torch.float32


@contextlib.contextmanager
def gather_precision(dtype):
    """Default ``gather_dtype`` of the products issued by THIS thread inside the block, for calls that pass none: the
    drop-in modules keep the reference's signatures, so this is how a model opts in —
    ``with gather_precision(torch.bfloat16): loss = forward_loss(...)``.  Blocks nest; ``None`` restores float32.  A
    product records the dtype it ran with, so its backward uses the same one wherever it runs."""
    _check_gather_dtype(dtype)
    prev = getattr(_gather_default, "dtype", None)
    _gather_default.dtype = dtype
    try:
        yield
    finally:
        _gather_default.dtype = prev


def rows_to_bf16(X: torch.Tensor, scale: Optional[torch.Tensor] = None) -> torch.Tensor:
    """``bf16_rne(diag(scale) X)`` in one streaming pass (``dgmi_rows_to_bf16``): the product in float32, rounded once;
    bitwise ``(scale[:, None] * X).to(torch.bfloat16)``.  ``X.shape[1]`` must be a multiple of 8."""
    _require_device(X, scale)
    return _T.rows_to_bf16(X, None if scale is None else scale.reshape(-1).contiguous())


def _ptr(t: Optional[torch.Tensor]):
    return None if t is None else t.data_ptr()


def _stream(device) -> int:
    """Raw hipStream_t of torch's current stream on ``device`` (kernels are enqueued there)."""
    return torch._C._cuda_getCurrentRawStream(device.index)


def _guard(device):
    """Make ``device`` current for the launch; free when it already is (the common case)."""
    if torch.cuda.current_device() == device.index:
        return _NULLCTX
    return torch.cuda.device(device)


def _require_device(*tensors):
    dev = None
    for t in tensors:
        if t is None:
            continue
        if not t.is_cuda:
            raise RuntimeError(
                "dream_gnn_amd ops run on the MI355X only: got a %s tensor. There is no CPU path "
                "(the CPU restatement under oracle/ is test infrastructure)." % t.device)
        if dev is None:
            dev = t.device
        elif t.device != dev:
            raise RuntimeError("tensors on different devices: %s vs %s" % (dev, t.device))
    return dev


def csr_from_coo(row: torch.Tensor, col: torch.Tensor, n_rows: int, n_cols: int = 0,
                 check_range: bool = False, return_flag: bool = False):
    """Stable COO -> CSR on the device: ``(indptr[n_rows+1], indices[E], eid[E])``, all int32.

    ``eid`` is the stable permutation (``argsort(row, kind='stable')``); duplicates are kept.
    Replaces DGL's COO->CSR behind ``dgl.heterograph`` (data_loader.py:448, augmentation.py:65).
    ``check_range=True`` reads the kernel's error flag back (one host sync) and raises if a row
    id is outside ``[0, n_rows)`` or, with ``n_cols > 0``, a column id outside ``[0, n_cols)``.
    ``return_flag=True`` appends that flag as a 1-element int32 device tensor instead (no sync), for
    callers that fold it into a readback of their own.  With the flag set the arrays are in bounds
    but meaningless: nothing may be derived from them.
    """
    _require_device(row, col)
    indptr, indices, eid, flag = _T.csr_from_coo(row, col, n_rows, n_cols)
    if check_range and int(flag.item()) != 0:
        raise RuntimeError("csr_from_coo: an id is outside [0, %d) x [0, %s)"
                           % (n_rows, n_cols if n_cols > 0 else "unchecked"))
    if return_flag:
        return indptr, indices, eid, flag
    return indptr, indices, eid


def gather_f32(values: torch.Tensor, perm: torch.Tensor) -> torch.Tensor:
    _require_device(values, perm)
    return _T.gather_f32(values, perm)


class SpmmPlan:
    """nnz-balanced launch plan of one CSR (``dgmi_spmm_plan_build``): rows longer than
    ``chunk`` edges are cut into one-wave chunks.  Depends only on ``indptr``."""

    def __init__(self, indptr: torch.Tensor, nnz: int, chunk: Optional[int] = None):
        dev = _require_device(indptr)
        self.n_rows = int(indptr.shape[0] - 1)
        self.nnz = int(nnz)
        self.chunk = int(chunk) if chunk else int(_L.dgmi_spmm_default_chunk(self.n_rows, self.nnz))
        if int(_L.dgmi_spmm_plan_bytes(self.n_rows, self.nnz, self.chunk)) == 0:
            raise RuntimeError("invalid plan parameters (chunk=%d)" % self.chunk)
        self.buf = _T.plan_build(indptr, self.nnz, self.chunk)
        self._pbytes = {}

    def partials_bytes(self, F: int) -> int:
        b = self._pbytes.get(F)
        if b is None:
            b = self._pbytes[F] = int(_L.dgmi_spmm_partials_bytes(self.nnz, self.chunk, int(F)))
        return b

    def header(self):
        """(n_items, n_long_rows, n_slots, chunk, ...) — reads the device header back (tests)."""
        return tuple(int(v) for v in self.buf[:64].view(torch.int32).tolist())


def build_plan(indptr: torch.Tensor, nnz: int, chunk: Optional[int] = None) -> SpmmPlan:
    return SpmmPlan(indptr, nnz, chunk)


def _launch_spmm(dev, indptr, indices, vals, X, src_scale, dst_scale, out, plan, n_dst, n_src, F, ldx,
                 eid=None, keep=None, epi=None):
    """One ``dreamgnn_mi::spmm_csr_raw`` / ``spmm_csr_out`` dispatch (-> ``dgmi_spmm_csr_f32`` or
    ``dgmi_spmm_csr_planned_f32`` on torch's current stream; dtype / shape / device checks, output
    and scratch allocation happen in the op).  ``keep``: (n, 8) int32 subset descriptions
    (``random_subset_select``) applied through ``eid`` on the fly."""
    args = (indptr, indices, vals, eid if keep is not None else None, keep, X, src_scale, dst_scale,
            None if plan is None else plan.buf, 0 if plan is None else plan.chunk)
    epi = epi or _NO_EPI
    if out is None:
        return _T.spmm_csr_raw(*args, *epi)
    _T.spmm_csr_out(*args, out, *epi)
    return out


def _prep_scale(s, n, name):
    if s is None:
        return None
    if s.dim() != 1:
        s = s.reshape(-1)
    if s.dtype != torch.float32 or s.shape[0] != n or not s.is_contiguous():
        if s.dtype != torch.float32:
            raise RuntimeError("%s must be float32" % name)
        if s.shape[0] != n:
            raise RuntimeError("%s has %d entries, expected %d" % (name, s.shape[0], n))
        s = s.contiguous()
    return s


def spmm_csr_raw(indptr, indices, vals, X, src_scale=None, dst_scale=None, out=None,
                 plan: Optional[SpmmPlan] = None, eid=None, keep=None) -> torch.Tensor:
    """One SpMM launch, no autograd.  X may be a row-strided 2-D view.  ``plan=None``:
    ``dgmi_spmm_csr_f32`` (a wave per row); else ``dgmi_spmm_csr_planned_f32``.  ``keep`` (with
    ``eid``): subset descriptions for edge dropout on the fly."""
    dev = _require_device(indptr, indices, vals, X, src_scale, dst_scale, out, eid, keep)
    if keep is not None:
        keep = _prep_keep(keep)
    n_dst = indptr.shape[0] - 1
    if plan is not None and (plan.n_rows != n_dst or plan.nnz != indices.shape[0]):
        raise RuntimeError("plan was built for another CSR")
    src_scale = None if src_scale is None else src_scale.reshape(-1)
    dst_scale = None if dst_scale is None else dst_scale.reshape(-1)
    return _launch_spmm(dev, indptr, indices, vals, X, src_scale, dst_scale, out, plan, n_dst, X.shape[0],
                        X.shape[1] if X.dim() == 2 else 0, 0, eid, keep)


def _prep_keep(keep):
    """Subset descriptions as an (n, 8) contiguous int32 tensor."""
    if keep.dtype != torch.int32 or keep.dim() not in (1, 2) or keep.shape[-1] != 8:
        raise RuntimeError("keep must be int32 with 8 words per description, got %s %s" % (keep.dtype, tuple(keep.shape)))
    keep = keep.reshape(-1, 8)
    if keep.shape[0] > 8:
        raise RuntimeError("at most 8 subset descriptions per product")
    return keep if keep.is_contiguous() else keep.contiguous()


def _sliced_ok(X, out) -> bool:
    """16-B alignment requirements of ``dgmi_spmm_sliced_f32``."""
    if X.dtype != torch.float32 or X.stride(1) != 1 or X.stride(0) % 4 != 0 or X.data_ptr() % 16 != 0:
        return False
    return out is None or (out.is_contiguous() and out.data_ptr() % 16 == 0)


def _sliced_bf16_ok(X, out) -> bool:
    """The same for a product that gathers bf16: a float32 ``X`` as :func:`_sliced_ok` (so that a refused request takes
    exactly today's path), a bfloat16 ``X`` with 16-B aligned rows."""
    if X.dtype == torch.float32:
        return _sliced_ok(X, out)
    if X.dtype != torch.bfloat16 or X.stride(1) != 1 or X.stride(0) % 8 != 0 or X.data_ptr() % 16 != 0:
        return False
    return out is None or (out.is_contiguous() and out.data_ptr() % 16 == 0)


class SlicedCSR:
    """Source-sliced CSR for the XCD-local SpMM (``dgmi_csr_sliced_from_coo_i32``): edges sorted
    by (slice(src), row); ``segptr`` has ``n_slices * n_dst + 1`` entries."""

    N_SLICES = 8  # one slice of X per XCD

    def __init__(self, dst, src, n_dst, n_src, vals=None, n_slices: int = N_SLICES):
        _require_device(dst, src, vals)
        self.n_dst, self.n_src, self.n_slices = int(n_dst), int(n_src), int(n_slices)
        # range_flag: 1 if an id was out of range (device tensor; callers that build from unvalidated
        # edge lists read it — CSRGraph validates before it ever builds this layout)
        self.segptr, self.indices, self.eid, self.range_flag = _T.csr_sliced_from_coo(dst, src, self.n_dst, self.n_src,
                                                                                    self.n_slices)
        self.vals = None if vals is None else gather_f32(vals, self.eid)
        self.id_mult = False  # True: the id words carry integer multiplicities (bits 28..30 = m - 1), no value stream

    @classmethod
    def from_csr(cls, indptr, indices, eid, n_dst, n_src, n_slices: int = N_SLICES):
        """The same layout derived from the CSR of the same edge list (``dgmi_csr_sliced_from_csr_i32``): one
        stable partition pass by source slice instead of a full sort; bit-identical to the constructor."""
        self = cls.__new__(cls)
        self.n_dst, self.n_src, self.n_slices = int(n_dst), int(n_src), int(n_slices)
        self.segptr, self.indices, self.eid, self.range_flag = _T.csr_sliced_from_csr(indptr, indices, eid, self.n_src,
                                                                                    self.n_slices)
        self.vals = None
        self.id_mult = False
        return self

    def compacted(self, keep, vals=None, indices=None, id_mult=False) -> "SlicedCSR":
        """This layout with the edges dropped under the subset description(s) ``keep`` REMOVED
        (``dgmi_compact_layout_i32``: four streaming launches, no sort; survivors keep their order, so it is the layout
        a rebuild from the kept edge list would give — the reference's per-iteration construction, train.py:267 ->
        augmentation.py:48-65).  ``vals``: this layout's edge values (sliced order), compacted alongside; ``indices``
        (with ``id_mult``): id words to compact instead of the layout's own — the same ids carrying multiplicities.  The
        result runs the plain kernels: no ``eid`` stream, no hash per edge and pass, column passes as usual."""
        c = SlicedCSR.__new__(SlicedCSR)
        c.n_dst, c.n_src, c.n_slices = self.n_dst, self.n_src, self.n_slices
        c.segptr, c.indices, v = _T.compact_layout(self.segptr, self.indices if indices is None else indices, vals, self.eid,
                                                   _prep_keep(keep))
        c.vals = None if vals is None else v
        c.id_mult = bool(id_mult)
        c.eid, c.range_flag = None, self.range_flag  # positions no longer map to the caller's edge order
        return c

    _DEFAULT = object()

    def _prescale_pays(self, table_bytes: int, one_pass: bool) -> bool:
        """The pass moves 2 x table bytes (3.4e-13 s per byte measured), the in-kernel scale gather costs 2.7e-12 s
        per edge and column pass: pre-scale when the table is below ~8 bytes per edge-pass (config 4: 26-51 MB against
        10 M edges x 1-2 passes; a 400 MB table with 6 M edges keeps the in-kernel gather — the kernel-choice sweep)."""
        return self._prescale_rule(table_bytes, one_pass, self.n_dst, self.n_slices, int(self.indices.shape[0]))

    @staticmethod
    def _prescale_rule(table_bytes: int, one_pass: bool, n_dst: int, n_slices: int, nnz: int) -> bool:
        if table_bytes < PRESCALE_MIN_TABLE_BYTES:
            return False
        passes = 1 if one_pass or n_dst < 32768 or table_bytes // n_slices <= (4 << 20) else 2  # the launcher's column-pass rule
        return table_bytes <= 6 * nnz * passes

    def spmm(self, X, src_scale=None, dst_scale=None, out=None, vals=_DEFAULT, keep=None, epi=None, full_width=False,
             indices=None, id_mult=None, gather_dtype=None):
        """``vals`` (in sliced order, see ``eid``) overrides the values given at construction; ``indices`` with
        ``id_mult=True``: id words carrying integer edge multiplicities (bits 28..30 = m - 1; then ``vals`` must be None);
        ``keep``: subset descriptions applied through ``eid`` (edge dropout on the fly); ``epi``: output
        epilogue (act, slope, out_mask, mask_scale) applied by the plane-reduce kernel; ``full_width``:
        never sweep the columns in two half-width passes (``column_passes = 1`` of the C ABI).

        A bfloat16 ``X`` is gathered as it is (``dgmi_spmm_sliced_bf16``: float32 sums, planes and output), without a
        ``src_scale`` — the scale belongs to the conversion.  ``gather_dtype=torch.bfloat16`` with a float32 ``X`` makes
        that table first, ``rows_to_bf16(X, src_scale)``, and gathers from it.  This method reads the keyword only, never
        the default of :func:`gather_precision`."""
        vals = self.vals if vals is SlicedCSR._DEFAULT else vals
        _check_gather_dtype(gather_dtype)
        if X.dtype == torch.bfloat16 and src_scale is not None:
            raise RuntimeError("a bfloat16 X cannot take a src_scale: the scale is applied in float32 BEFORE the one rounding "
                               "to bf16 — pass the float32 table (with gather_dtype=torch.bfloat16) or rows_to_bf16(X, src_scale)")
        if not X.is_cuda or X.device != self.segptr.device:
            _require_device(self.segptr, X)
        if X.dim() == 2 and X.shape[0] != self.n_src:
            raise RuntimeError("X has %d rows, the graph has %d source nodes" % (X.shape[0], self.n_src))
        if X.dtype == torch.bfloat16 or gather_dtype == torch.bfloat16:
            if X.dim() != 2 or X.shape[1] % 8 != 0:
                raise RuntimeError("the bf16 gather needs a 2-D table with a multiple of 8 columns, got %s" % (tuple(X.shape),))
            if X.dtype != torch.bfloat16:
                if X.dtype != torch.float32:
                    raise RuntimeError("X must be float32 or bfloat16, got %s" % X.dtype)
                X = _T.rows_to_bf16(X, None if src_scale is None else src_scale.reshape(-1).contiguous())
            id_mult = self.id_mult if id_mult is None else bool(id_mult)
            args = (self.segptr, self.indices if indices is None else indices, vals, self.eid if keep is not None else None,
                    None if keep is None else _prep_keep(keep), X, None if dst_scale is None else dst_scale.reshape(-1),
                    self.n_dst, self.n_slices)
            epi = epi or _NO_EPI
            if out is None:
                return _T.spmm_sliced_bf16_raw(*args, *epi, 1 if full_width else 0, int(id_mult))
            _T.spmm_sliced_bf16_out(*args, out, *epi, 1 if full_width else 0, int(id_mult))
            return out
        if src_scale is not None and X.dim() == 2 and self._prescale_pays(X.shape[0] * X.shape[1] * 4, keep is not None or full_width):
            # diag(src_scale) X as ONE streaming pass, then the un-scaled gather: inside the kernel the scale is a
            # random 4-byte load per edge (and per column pass) — one more cache-line request beside the row's four —
            # which costs the config-4 products 8-18 % (tools/scale_cost_ab.py: 0.326 -> 0.285 ms, 0.298 -> 0.283 ms
            # including the pass)
            X = _T.scale_rows(X, src_scale.reshape(-1).contiguous())
            src_scale = None
        id_mult = self.id_mult if id_mult is None else bool(id_mult)
        args = (self.segptr, self.indices if indices is None else indices, vals, self.eid if keep is not None else None,
                None if keep is None else _prep_keep(keep), X, None if src_scale is None else src_scale.reshape(-1),
                None if dst_scale is None else dst_scale.reshape(-1), self.n_dst, self.n_slices)
        epi = epi or _NO_EPI
        passes = 1 if full_width else 0
        if out is None:
            return _T.spmm_sliced_raw(*args, *epi, passes, int(id_mult))
        _T.spmm_sliced_out(*args, out, *epi, passes, int(id_mult))
        return out


# XCD-local path is used when the gather table is a few L2s large (8 XCDs x 4 MiB): below, X is
# L2-hot anyway; far above, a 1/8 slice no longer fits an L2 and the plane traffic is pure cost.
# Measured on MI355X (tools/explore.py slicedcap, 10 M edges, F=128): sliced/planned time ratio
# 1.0 at a 6 MB table, 1.9-2.4x at 13-51 MB, 1.2x at 102 MB, 1.0 at 205 MB; 1.55x at average
# degree 100, 0.72x at 25 (a (row, slice) segment of 3 edges is all overhead).
FORCE_KERNEL = {"planned": "planned", "sliced": "sliced"}.get(os.environ.get("DGMI_FORCE_KERNEL", ""))
# Near-complete relation slices (f3, SURVEY §9-Q3: the reference's encoder graph holds EVERY train pair, both
# labels, data_loader.py:146-150,170 — lrssl shape: 464 897 of 519 603 cells) are handled one level up, as the
# COMPLEMENT form `column sum - complement cells` over the same CSR kernels (graph.py
# HeteroGraph.fused_relations_complement): 14 us against 40 us per relation-fused product at F = 344.  The round-2
# dense form (a materialised dense matrix through torch.mm) lost to the CSR kernel in context and was retired.
# Which products take the XCD-local form: fitted to a timing sweep of every form (round 3,
# tools/kernel_choice_sweep.py -> profiles/r03_kernel_choice_sweep.csv: F in {64, 128, 256, 344}, 20k .. 1.6M sources,
# average degree 16 .. 400, uniform and Zipf(1.1) degrees).  The sliced pair's advantage is set by the edges per
# (row, slice) segment — the average degree — and shrinks as the table outgrows what 8 L2s / the Infinity Cache hold:
#   degree >= 192: up to 1.5 GB tables     degree >= 96: up to 800 MB     degree >= 48: up to 420 MB
#   32 <= degree < 48: only where a slice is about one L2 (20 .. 80 MB tables: +7 .. 18 %)
# and tables below 6 MB are L2-hot for every kernel.  Long-row graphs (cut into virtual rows of SPLIT_ROW_EDGES) are
# judged by the degree of their virtual rows; their planned kernel is slower, so the split form pays from 4 MB tables
# and up to larger ones.  Round 2's narrower rule (10-160 MB at degree >= 64) picked a form > 10 % slower than the
# best on 63 of the sweep's 336 shapes; this one on 3 (all within 18 %, at the rule's edges).
SLICED_MIN_TABLE_BYTES = 6_000_000
SLICED_TIERS = ((48, 420_000_000), (96, 800_000_000), (192, 1_500_000_000))       # (average degree >=, table bytes <=)
SLICED_LOW_DEGREE = (32, 20_000_000, 80_000_000)                                    # degree >=, table bytes in [lo, hi]
SPLIT_MIN_TABLE_BYTES = 4_000_000
PRESCALE_MIN_TABLE_BYTES = 8_000_000  # XCD-local products on tables from this size scale X in a pass of its own
# Edge-dropped views of graphs that take the XCD-local form: the layout is COMPACTED once per view (a training step
# makes one view per edge list and runs each layout 3 x forward and 3 x backward) instead of evaluating keep(eid[p])
# per edge, product and column pass.  Config 4, ms per product un-dropped / dropped on the fly / dropped after
# compaction: see bench.py `variants`.  DGMI_COMPACT_DROPPED=0 keeps the on-the-fly kernels (A/B, tests).
COMPACT_DROPPED = os.environ.get("DGMI_COMPACT_DROPPED", "1") != "0"
# Weighted graphs in the XCD-local form whose values are `row scale x small integer` — every adjacency the reference
# builds: D^-1 (A + A^T + I), data_loader.py:297-308 + utils.py:11-17 — run without a value stream: the multiplicity rides
# in the id word's spare bits, the row scale goes where dst_scale (forward) / src_scale (transpose) go.  Found once per
# weighted graph by `dgmi_row_multiplicity_f32` (one host readback, never inside a stream capture); values that have no
# such form to within 2 ulp keep the value stream.  DGMI_MULT_FORM=0 switches it off (A/B, tests).
MULT_FORM = os.environ.get("DGMI_MULT_FORM", "1") != "0"
MULT_REL_TOL = 2.4e-7
MULT_SHIFT, MULT_MAX_IDS = 28, 1 << 28
# A scale of the gathered rows that is a node constant rides in the id words as well (include/dgmi_scale.h): bits 17..27
# hold the code of its bit pattern, a table of at most 2048 patterns goes with the launch, ids are < 2^17 — for the
# products the library's owned form runs scaled (`dgmi_spmm_owned_scaled_takes`), instead of their pre-scale pass.
# DGMI_SCALE_CODES=0 switches it off (A/B, tests).
SCALE_CODES = os.environ.get("DGMI_SCALE_CODES", "1") != "0"
SCALE_SHIFT, SCALE_BITS = _lib.SCALE_CODE_SHIFT, _lib.SCALE_CODE_BITS
SCALE_MAX_IDS, SCALE_MAX_CODES = 1 << SCALE_SHIFT, 1 << SCALE_BITS
COLUMN_PASS_MIN_ROWS, LONG_ROW_MIN_DEGREE = 32768, 384                # the launcher's column-pass rule (dgmi_sliced.hip); see _few_long_rows
SPLIT_MIN_DEGREE, SPLIT_DENSE_DEGREE = 8, 300                       # average degree (edges / rows) of the whole graph
SPLIT_MAX_TABLE_BYTES, SPLIT_MAX_TABLE_BYTES_DENSE = 350_000_000, 900_000_000


def _table_cap(tiers, degree: float) -> int:
    cap = 0
    for d, c in tiers:
        if degree >= d:
            cap = c
    return cap


class _Direction:
    """One direction of a structure — the rows a product writes and the columns it gathers: the forward product
    (rows = destinations) or the transposed one (rows = sources; its CSR is built by the first use,
    :meth:`CSRGraph._built`).  Everything a product reads per direction, so that it is written once for both."""

    __slots__ = ("transposed", "suffix", "csr_key", "sliced_key", "split_key", "gathered_name", "out_name",
                 "n_rows", "n_cols", "cols_coo", "indptr", "indices", "eid", "plan", "max_deg", "regular", "sliced", "split")

    def __init__(self, suffix, n_rows, n_cols, cols_coo, regular, gathered_name, out_name):
        self.transposed, self.suffix = bool(suffix), suffix  # suffix of this direction's keys in a view's _v / _c
        self.csr_key, self.sliced_key, self.split_key = "csr" + suffix, "sliced" + suffix, "split" + suffix
        self.gathered_name, self.out_name = gathered_name, out_name  # how errors call the scales of the gathered / the output rows
        self.n_rows, self.n_cols, self.cols_coo = n_rows, n_cols, cols_coo  # cols_coo: the gathered ids in the caller's edge order
        self.indptr = self.indices = self.eid = self.plan = None
        self.max_deg = None  # longest row, once a readback has told
        self.regular = regular  # no row is extremely long (None: not known yet, CSRGraph._decide_regular)
        self.sliced = self.split = None  # the first XCD-sliced layout (others: _Structure.wide) and the split form


class _Structure:
    """Everything about a CSRGraph that depends on the edge list only (shared by value views)."""

    __slots__ = ("n_dst", "n_src", "dst", "src", "nnz", "planned", "validated", "wide", "fwd", "bwd", "scale_builds")


# the per-direction state under the names it had as loose slots: indptr .. split read the forward record, *_t the transposed
for _side, _sfx, _fields in (("fwd", "", ("indptr", "indices", "eid", "plan", "max_deg", "regular", "sliced", "split")),
                             ("bwd", "_t", ("max_deg", "regular", "sliced", "split"))):
    for _f in _fields:
        setattr(_Structure, _f + _sfx, property(operator.attrgetter(_side + "." + _f)))


# Rows longer than this are cut into virtual rows before the XCD-local kernel sees them (power-law
# graphs): a (virtual row, slice) segment is then at most SPLIT_ROW_EDGES / 8 edges long.  A lane group
# streams 8 consecutive virtual rows of a slice as one dependent chain, so this length sets the critical
# path of the launch: Zipf(1.2), 10 M edges (tools/zipf_split_probe.py) 0.477 ms at 2048, 0.443 at 1024,
# 0.418 at 512 (with the launcher's column passes), 0.439 at 256 — in round 2.  Round 4 (tools/zipf_sweep.py, after the
# touch-ahead and with the light rows out of the sliced pass): 0.374 ms at 512 (23 632 virtual rows: below the 32 768 the
# launcher wants for its column passes), 0.329 at 256, 0.336 at 192, 0.363 at 128.
SPLIT_ROW_EDGES = 256


# Rows below this many edges do not go through the XCD-local kernel of a split graph at all: a (row, slice) segment of
# 0-5 edges is all bookkeeping.  A power-law graph is mostly such rows (Zipf(1.2), 10 M edges over 50 000 rows: 42 800 rows
# hold 5 % of the edges): they are gathered by the second-stage product instead, straight from the source table.
# tools/zipf_sweep.py, virtual rows of 256 edges: 0.348 ms with every row in the sliced pass, 0.329 / 0.334 / 0.336 with the
# rows below 24 / 48 / 96 edges out of it.
SPLIT_LIGHT_ROW_EDGES = 24


class _SplitSliced:
    """XCD-local product for a graph with extremely long rows.  Every HEAVY row is cut into virtual rows of at most
    ``SPLIT_ROW_EDGES`` edges (in CSR order), the sliced kernel runs on the virtual-row graph (regular by
    construction) and writes ``Yv``; a second, small product ``Y = C · [Yv ; Xs]`` then gives every row its sum:
    ``C[row, v] = 1`` adds a heavy row's virtual rows back together in order, and — **(r4)** when at least a quarter of
    the rows are LIGHT (< ``SPLIT_LIGHT_ROW_EDGES`` edges) — the light rows' own edges point into the second half of the
    same table, the (pre-scaled) source rows ``Xs``, so that they never become (row, slice) segments of one or two edges.
    ``dst_scale`` and the epilogue are applied by that second product."""

    def __init__(self, indptr, eid, cols_coo, n_rows, n_cols):
        dev = indptr.device
        nnz = int(eid.shape[0])
        deg = (indptr[1:] - indptr[:-1]).long()
        light = deg < SPLIT_LIGHT_ROW_EDGES
        n_light = int(light.sum())  # host syncs here and below: at construction only
        self.has_light = 4 * n_light >= n_rows and n_light < n_rows
        if not self.has_light:
            light = torch.zeros_like(light)
        nv = torch.where(light, torch.zeros_like(deg), torch.clamp((deg + SPLIT_ROW_EDGES - 1) // SPLIT_ROW_EDGES, min=1))
        vptr = torch.zeros(n_rows + 1, dtype=torch.int64, device=dev)
        vptr[1:] = torch.cumsum(nv, 0)
        self.n_virtual = int(vptr[-1])
        rows_p = torch.repeat_interleave(torch.arange(n_rows, device=dev), deg, output_size=nnz)
        rank = torch.arange(nnz, device=dev) - indptr.long()[rows_p]
        vrow_p = (vptr[rows_p] + rank // SPLIT_ROW_EDGES).to(torch.int32)
        cols_p = cols_coo[eid.long()]  # CSR order
        self.n_rows, self.n_cols = n_rows, n_cols
        if not self.has_light:
            vrow_coo = torch.empty(nnz, dtype=torch.int32, device=dev)
            vrow_coo[eid.long()] = vrow_p  # CSR position -> the caller's edge order
            self.sliced = SlicedCSR(vrow_coo, cols_coo, self.n_virtual, n_cols)
            self.c_indptr = vptr.to(torch.int32)
            self.c_indices = torch.arange(self.n_virtual, dtype=torch.int32, device=dev)
            self.c_eid = self.c_light_eid = self.c_order = None
        else:
            heavy_p = ~light[rows_p]
            # the heavy rows' edges, in CSR order (a stable sort by (slice, virtual row) keeps it inside a segment); the
            # layout's eid is composed back to the caller's edge order: values and dropout descriptions index that
            self.sliced = SlicedCSR(vrow_p[heavy_p].contiguous(), cols_p[heavy_p].contiguous(), self.n_virtual, n_cols)
            self.sliced.eid = eid[heavy_p][self.sliced.eid.long()].contiguous()
            # second stage: row r <- its virtual rows (ids < n_virtual) or, for a light row, its own edges (n_virtual + source)
            light_p = ~heavy_p
            ent_row = torch.cat([torch.repeat_interleave(torch.arange(n_rows, device=dev), nv, output_size=self.n_virtual), rows_p[light_p]])
            ent_idx = torch.cat([torch.arange(self.n_virtual, dtype=torch.int32, device=dev), cols_p[light_p] + self.n_virtual])
            order = torch.sort(ent_row, stable=True).indices
            self.c_order = order
            self.c_indices = ent_idx[order].contiguous()
            cptr = torch.zeros(n_rows + 1, dtype=torch.int64, device=dev)
            cptr[1:] = torch.cumsum(torch.where(light, deg, nv), 0)
            self.c_indptr = cptr.to(torch.int32)
            self.c_light_eid = eid[light_p]  # the light edges' positions in the caller's order (values, dropout)
            # edge ids of the second stage's entries for dropout on the fly: virtual-row entries lie outside every description
            never = torch.full((self.n_virtual,), 0x7FFFFFFF, dtype=torch.int32, device=dev)
            self.c_eid = torch.cat([never, self.c_light_eid])[order].contiguous()
        self.c_plan = build_plan(self.c_indptr, int(self.c_indices.shape[0]))

    def combine_values(self, coo_vals):
        """Values of the second stage's entries for a view with edge values ``coo_vals`` (the caller's order): 1 for a
        virtual row, the edge's own value for a light row's edge.  None when there is nothing to weight."""
        if coo_vals is None or not self.has_light:
            return None
        ones = torch.ones(self.n_virtual, dtype=torch.float32, device=coo_vals.device)
        return torch.cat([ones, coo_vals[self.c_light_eid.long()]])[self.c_order].contiguous()

    def spmm(self, X, src_scale, dst_scale, out, vals, keep=None, epi=None, compacted=None, c_vals=None):
        """``compacted``: the virtual-row layout with a view's dropped edges already removed (then ``vals`` is not
        consulted: it carries its own values); ``c_vals``: :meth:`combine_values` of the view."""
        F = X.shape[1]
        if self.has_light:
            # [Yv ; Xs] in ONE table: the sliced kernel gathers from its second half and writes its first half
            buf = torch.empty((self.n_virtual + self.n_cols, F), dtype=torch.float32, device=X.device)
            xs, yv = buf[self.n_virtual:], buf[:self.n_virtual]
            if src_scale is not None:
                torch.mul(X, src_scale.reshape(-1, 1), out=xs)
            else:
                xs.copy_(X)
            if compacted is not None:
                compacted.spmm(xs, None, None, yv)
            else:
                self.sliced.spmm(xs, None, None, yv, vals=vals, keep=keep)
            table, n_table, c_keep = buf, self.n_virtual + self.n_cols, keep
        else:
            if compacted is not None:
                yv = compacted.spmm(X, src_scale, None, None)
            else:
                yv = self.sliced.spmm(X, src_scale, None, None, vals=vals, keep=keep)
            table, n_table, c_keep = yv, self.n_virtual, None
        if out is None:
            out = torch.empty((self.n_rows, F), dtype=torch.float32, device=X.device)
        return _launch_spmm(X.device, self.c_indptr, self.c_indices, c_vals, table, None, dst_scale, out, self.c_plan,
                            self.n_rows, n_table, F, F, eid=self.c_eid, keep=c_keep, epi=epi)


class CSRGraph:
    """A relation slice / sparse adjacency in the layout the kernels read.

    Structure (shared, built once): the destination-major CSR (forward ``Y = A X``), lazily the
    source-major CSR of the reversed edges (``dX = A^T dY``) and the XCD-sliced layouts, each
    with its launch plan, all made by the device COO->CSR.  Values (per view): optional per-edge
    values in the caller's COO order, permuted on demand into each layout.  Row = destination,
    col = source, as in ``th.spmm(adj, x)`` where ``adj[dst, src]``.

    ``check_range=True`` costs one host sync (id range + maximum degree readback); pass ``False``
    for edge lists derived from an already validated graph.  :meth:`with_values` gives a view of
    the same structure with other edge values — how edge dropout is applied without re-sorting
    (a 0/1 keep mask as values).
    """

    def __init__(self, dst: torch.Tensor, src: torch.Tensor, n_dst: int, n_src: int,
                 vals: Optional[torch.Tensor] = None, check_range: bool = True, planned: bool = True,
                 regular: Optional[bool] = None, regular_t: Optional[bool] = None):
        _require_device(dst, src, vals)
        S = self._S = _Structure()
        S.n_dst, S.n_src = int(n_dst), int(n_src)
        S.dst = dst.to(torch.int32).contiguous()
        S.src = src.to(torch.int32).contiguous()
        if vals is not None and vals.shape[0] != S.dst.shape[0]:
            raise RuntimeError("vals/edge-list length mismatch")
        S.planned = planned
        S.wide = {}  # (transposed, n_slices) -> an XCD-sliced layout of another slice count than sliced / sliced_t have (_layout_of)
        S.validated = bool(check_range)
        S.scale_builds = 0  # coded id words made for this structure's views (_scale_ids)
        # `regular`: no destination row is extremely long, so the XCD-local kernel (which walks a
        # (row, slice) segment sequentially) is safe to use.  Known after the one readback of a validated build
        # (below); for an unchecked build None = not known yet: decided — one readback of the maximum degree — at the
        # first product LARGE enough for the XCD-local form to be in question (a 4 MB table), never for the small
        # per-step graphs of the real datasets and never inside a stream capture.  (Until round 4 unchecked builds were
        # simply "not regular": every adjacency built by graph.similarity_graph / feature_similarity_graph — trusted by
        # construction — ran the planned kernel at scale, 0.84 ms against 0.41 ms per kNN-64 product.)
        D = S.fwd = _Direction("", S.n_dst, S.n_src, S.src, bool(regular) if regular is not None else None, "src_scale", "dst_scale")
        S.bwd = _Direction("_t", S.n_src, S.n_dst, S.dst, regular_t, "dst_scale", "src_scale")  # its CSR: _built, on first use
        D.indptr, D.indices, D.eid, flag = csr_from_coo(S.dst, S.src, S.n_dst, S.n_src, return_flag=True)
        S.nnz = int(D.indices.shape[0])
        self._set_values(None if vals is None else vals.to(torch.float32).contiguous())
        if check_range:
            # ids are checked BEFORE anything is derived from the CSR: the sort of an edge list with
            # ids outside [0, n) leaves indptr in bounds but meaningless, and a launch plan built
            # from it would be garbage (the plan kernels clamp, the product would still be wrong)
            self._validate(flag)
        D.plan = build_plan(D.indptr, S.nnz) if planned else None

    # -- values -----------------------------------------------------------------------------------
    def _set_values(self, coo_vals, keep=None):
        self._coo_vals = coo_vals
        self._v = {}  # layout name -> values permuted into that layout
        self._c = {}  # layout name -> that layout with this view's dropped edges removed (SlicedCSR.compacted)
        self._keep = keep  # (n, 8) int32 subset descriptions applied on the fly, or None
        self._mask = None  # 0/1 keep mask already multiplied into the values by masked(), COO order
        self._vals_before_mask = None  # the values masked() multiplied its mask into (undropped() restores them)

    def with_values(self, coo_vals: Optional[torch.Tensor]) -> "CSRGraph":
        """A view sharing this graph's structure (and whatever it builds later) with other per-edge
        values, given in the original COO edge order."""
        if coo_vals is not None and coo_vals.shape[0] != self.nnz:
            raise RuntimeError("expected %d edge values, got %d" % (self.nnz, coo_vals.shape[0]))
        view = object.__new__(CSRGraph)
        view._S = self._S
        view._set_values(None if coo_vals is None else coo_vals.to(torch.float32).contiguous(), self._keep)
        return view

    def masked(self, keep: torch.Tensor) -> "CSRGraph":
        """View with edge e weighted by ``keep[e]`` (0/1), times the existing values if any."""
        keep = keep.to(torch.float32)
        view = self.with_values(keep if self._coo_vals is None else self._coo_vals * keep)
        view._keep = self._keep
        view._mask = keep if self._mask is None else self._mask * keep
        view._vals_before_mask = self._vals_before_mask if self._mask is not None else self._coo_vals
        view._v["mult"] = False  # zeros among the values: no scale x multiplicity form — and no per-step detection (a readback)
        return view

    def dropped(self, desc: torch.Tensor) -> "CSRGraph":
        """View of the same structure and values with edge dropout applied ON THE FLY: ``desc`` holds
        the 8-word description(s) of the surviving subset(s) (``random_subset_select``), evaluated
        per edge inside the kernels through each layout's ``eid`` — no mask is carried into the
        layouts, nothing is re-sorted, dropped edges are skipped (not multiplied by zero).

        On a view that already carries descriptions the new ones are ANDed in (an edge covered by
        several descriptions survives only if each keeps it, ``csrc/dgmi_keep.h``): the intersection
        of independently drawn subsets.  A chained dropout that must keep an EXACT count of the
        survivors (the reference's composition, augmentation.py:113-124) draws its subset among
        :meth:`survivors` instead — ``graph.random_edge_dropout_sparse`` does."""
        desc = _prep_keep(desc)
        view = object.__new__(CSRGraph)
        view._S = self._S
        view._coo_vals, view._v = self._coo_vals, self._v  # values (and their per-layout copies) are shared
        view._c = {}  # another set of survivors: its own compacted layouts
        view._mask, view._vals_before_mask = self._mask, self._vals_before_mask
        view._keep = desc if self._keep is None else torch.cat([self._keep, desc])
        if view._keep.shape[0] > 8:
            raise RuntimeError("at most 8 subset descriptions per graph view")
        return view

    def keep_mask(self) -> Optional[torch.Tensor]:
        """float 0/1 mask over the COO edge order of the on-the-fly dropout (None if there is none)."""
        return None if self._keep is None else keep_mask(self._keep, self.nnz)

    def survivors(self) -> Optional[torch.Tensor]:
        """float 0/1 mask over the COO edge order of every dropout this view carries — the on-the-fly
        descriptions and the masks folded into the values by :meth:`masked` — or None for an
        un-dropped graph."""
        m = self.keep_mask()
        if self._mask is not None:
            m = self._mask if m is None else m * self._mask
        return m

    def undropped(self) -> "CSRGraph":
        """The view of the same structure with every dropout removed (original values)."""
        view = object.__new__(CSRGraph)
        view._S = self._S
        vals = self._coo_vals
        if self._mask is not None:
            vals = self._vals_before_mask
        view._set_values(vals)
        return view

    def _compacted(self, name: str, sliced: "SlicedCSR", mult=None) -> Optional["SlicedCSR"]:
        """The XCD-sliced layout ``name`` with this view's dropped edges removed, made on first use and kept with the
        view (None when the view drops nothing or compaction is switched off).  ``mult``: the (row scale, id words)
        of :meth:`_mult_ids` — then the id words with their multiplicities are what is compacted, and no values."""
        if self._keep is None or not COMPACT_DROPPED:
            return None
        c = self._c.get(name)
        if c is None:
            if mult is not None:
                c = sliced.compacted(self._keep, None, indices=mult[2], id_mult=True)
            else:
                c = sliced.compacted(self._keep, self._vals_for(name, sliced.eid))
            self._c[name] = c
        return c

    def _mult_form(self):
        """``(kind, scale, code_coo[nnz])`` when this view's edge values are ``scale[node] * m`` with ``m`` an integer in
        1..8 (``code = m - 1``, COO order), else None.  ``kind == "row"``: ``scale`` is indexed by the destination (row)
        — the reference's ``normalize(adj + adj.T + I)`` adjacencies, ``D^-1 M``; ``kind == "col"``: by the source
        (column) — the TRANSPOSE of such an adjacency handed in as a graph of its own (``M D^-1``).  Decided once per
        weighted graph (shared by its dropped views): one kernel + one host readback per form tried."""
        if self._coo_vals is None or not MULT_FORM or self._S.n_src > MULT_MAX_IDS or self._S.n_dst > MULT_MAX_IDS:
            return None
        m = self._v.get("mult")
        if m is None:
            if self._capturing():
                return None  # the decision needs a readback: not inside a capture (the value stream is always right)
            m = False
            for kind, D in (("row", self._S.fwd), ("col", self._S.bwd)):  # the transposed CSR is built only if "row" fails
                D = self._built(D)
                scale, code, fail = _T.row_multiplicity(D.indptr, self._vals_for(D.csr_key, D.eid), MULT_REL_TOL)
                if int(fail.item()) == 0:
                    code_coo = torch.empty_like(code)
                    code_coo[D.eid.long()] = code
                    m = (kind, scale, code_coo)
                    break
            self._v["mult"] = m
        return m or None

    def _mult_ids(self, name: str, sliced: "SlicedCSR"):
        """``(kind, scale, id words of layout `name` with the multiplicities in bits 28..30)`` or None."""
        mf = self._mult_form()
        if mf is None:
            return None
        ids = self._v.get(name + "/ids")
        if ids is None:
            ids = self._v[name + "/ids"] = sliced.indices | (mf[2][sliced.eid.long()] << MULT_SHIFT)
        return mf[0], mf[1], ids

    @staticmethod
    def _fold(scale, other):
        return scale if other is None else scale * other.reshape(-1)

    @staticmethod
    def scale_codes(scale: torch.Tensor, ids: torch.Tensor):
        """``(table, words)`` for a float32 scale vector of at most ``SCALE_MAX_IDS`` entries and id words whose low
        ``SCALE_SHIFT`` bits are ids into it: ``table`` lists the distinct BIT PATTERNS of ``scale`` (so ``-0.0``, ``+0.0``
        and every NaN payload keep a code of their own) and ``words = ids | code[id] << SCALE_SHIFT``, whatever else the
        words carry above bit ``SCALE_SHIFT + SCALE_BITS`` (the multiplicities).  ``(None, None)`` when ``scale`` has
        more than ``SCALE_MAX_CODES`` patterns.  Reads one size back."""
        if scale.dim() != 1 or scale.dtype != torch.float32 or scale.shape[0] > SCALE_MAX_IDS:
            raise RuntimeError("scale_codes takes a 1-D float32 scale of at most %d entries" % SCALE_MAX_IDS)
        bits, code = torch.unique(scale.contiguous().view(torch.int32), return_inverse=True)
        if bits.shape[0] > SCALE_MAX_CODES:
            return None, None
        words = ids | (code.to(torch.int32)[(ids & (SCALE_MAX_IDS - 1)).long()] << SCALE_SHIFT)
        return bits.view(torch.float32), words

    def _scale_ids(self, name: str, scale: torch.Tensor, ids: torch.Tensor):
        """``(table, coded id words)`` of layout ``name`` for the scale ``scale`` of its gathered rows, or None: the
        scale bound to the id words ONCE per graph and scale (a node constant in real use: a degree normalisation), so
        that the product needs no pass that scales ``X`` (include/dgmi_scale.h).  ``ids``: the layout's id words, with
        the multiplicities where the view has them.

        One entry per layout, kept with the view's values; a new scale replaces it.  The key is the scale's storage —
        pointer, length, stride and version counter, with a reference held so that the pointer cannot be reused — hence
        views of one tensor hit and an in-place update rebuilds.  Never inside a stream capture: the build reads a size
        back, and a replayed graph may refresh the scale in place without a version bump.  The same holds outside a capture
        for a scale written behind torch's back — its ``data_ptr()`` handed to a kernel through the C ABI: no version is
        bumped, the coded words stay those of the old values; such a caller passes a new tensor.  Two rebuilds without a hit in
        between (a caller that makes its scale anew per call) turn the route off for this view and layout."""
        if self._capturing() or scale.dtype != torch.float32 or not scale.is_cuda or scale.dim() != 1 or scale.shape[0] > SCALE_MAX_IDS:
            return None
        slot = name + "/scale_ids"
        entry = self._v.get(slot)
        if entry is False:
            return None
        key = (scale.data_ptr(), scale.shape[0], scale.stride(0), scale._version)
        if entry is not None and entry["key"] == key:
            entry["misses"] = 0
            return entry["coded"]
        misses = 0 if entry is None else entry["misses"] + 1
        if misses >= 2:
            self._v[slot] = False  # the second miss in a row: this caller's scale is no constant
            return None
        table, words = self.scale_codes(scale, ids)
        self._S.scale_builds += 1
        self._v[slot] = {"key": key, "ref": scale, "misses": misses, "coded": None if table is None else (table, words)}
        return self._v[slot]["coded"]

    def _combine_vals(self, name: str, split: "_SplitSliced"):
        """Second-stage values of a split layout for this view's edge values (made once per view and layout)."""
        if self._coo_vals is None or not split.has_light:
            return None
        v = self._v.get(name + "/combine")
        if v is None:
            v = self._v[name + "/combine"] = split.combine_values(self._coo_vals)
        return v

    def _vals_for(self, layout: str, eid: torch.Tensor):
        if self._coo_vals is None:
            return None
        v = self._v.get(layout)
        if v is None:
            v = self._v[layout] = gather_f32(self._coo_vals, eid)
        return v

    # -- structure accessors (kept as attributes of the public surface) ----------------------------
    n_dst = property(lambda self: self._S.n_dst)
    n_src = property(lambda self: self._S.n_src)
    indptr = property(lambda self: self._S.indptr)
    indices = property(lambda self: self._S.indices)
    eid = property(lambda self: self._S.eid)
    plan = property(lambda self: self._S.plan)
    regular = property(lambda self: self._S.regular)
    regular_t = property(lambda self: self._S.regular_t)
    _sliced = property(lambda self: self._S.sliced)
    _sliced_t = property(lambda self: self._S.sliced_t)

    @property
    def vals(self):
        """Edge values in CSR order (None for an unweighted graph)."""
        return self._vals_for("csr", self._S.fwd.eid)

    @property
    def nnz(self) -> int:
        return self._S.nnz

    @property
    def device(self):
        return self._S.fwd.indptr.device

    @staticmethod
    def _is_regular(max_deg: int, nnz: int, n_rows: int) -> bool:
        # the sliced kernel streams a (row, slice) segment sequentially in one lane group: rows up
        # to ~32x the average are a tail effect, rows of 10^5..10^6 edges (power laws) are not
        return max_deg <= max(1024, 32 * (nnz // max(n_rows, 1)))

    def _validate(self, flag: torch.Tensor):
        """One host sync: the range flag of the device COO->CSR and the maximum in-degree."""
        S, D = self._S, self._S.fwd
        if self.nnz == 0:
            D.regular = True
            return
        bad, max_deg = torch.stack([flag.reshape(()), (D.indptr[1:] - D.indptr[:-1]).max()]).tolist()
        if bad:  # error path only: say which side and by how much
            dlo, dhi, slo, shi = (int(v) for v in torch.stack([S.dst.min(), S.dst.max(), S.src.min(), S.src.max()]).tolist())
            if dlo < 0 or dhi >= S.n_dst:
                raise RuntimeError("destination id out of range [0, %d): min %d max %d" % (S.n_dst, dlo, dhi))
            raise RuntimeError("source id out of range [0, %d): min %d max %d" % (S.n_src, slo, shi))
        D.max_deg = int(max_deg)
        D.regular = self._is_regular(int(max_deg), self.nnz, S.n_dst)

    @staticmethod
    def _capturing() -> bool:
        return torch.cuda.is_available() and torch.cuda.is_current_stream_capturing()

    def _decide_regular(self, X, D: _Direction):
        """Settle ``regular`` of direction ``D`` of an unchecked build when a product large enough to care arrives."""
        small = X.dim() != 2 or D.n_cols * X.shape[1] * 4 < min(SLICED_MIN_TABLE_BYTES, SPLIT_MIN_TABLE_BYTES)
        # a VALIDATED build has synchronised once already and reads the transposed graph's longest row back whatever the
        # size (it also tells whether the planned form's second launch can be skipped: _plan_if_needed)
        if (small and not self._S.validated) or not X.is_cuda or self._capturing():
            return  # stays unknown (treated as "not regular" for this product): small tables never take the sliced form
        indptr = self._built(D).indptr
        D.max_deg = int((indptr[1:] - indptr[:-1]).max()) if self.nnz else 0
        D.regular = self._is_regular(D.max_deg, self.nnz, D.n_rows)

    def _use_sliced(self, F: int, n_rows: int, n_cols: int, regular: bool) -> bool:
        if FORCE_KERNEL is not None:  # debugging / A-B aid: DGMI_FORCE_KERNEL=planned|sliced
            return FORCE_KERNEL == "sliced" and F % 4 == 0 and n_rows * SlicedCSR.N_SLICES < 2 ** 31 - 1
        table = n_cols * F * 4
        if not (bool(regular) and F % 4 == 0 and n_rows * SlicedCSR.N_SLICES < 2 ** 31 - 1) or table < SLICED_MIN_TABLE_BYTES:
            return False
        degree = self.nnz / max(n_rows, 1)
        if table <= _table_cap(SLICED_TIERS, degree):
            return True
        lo_deg, lo, hi = SLICED_LOW_DEGREE
        return degree >= lo_deg and lo <= table <= hi

    def _use_split(self, F: int, n_rows: int, n_cols: int, regular) -> bool:
        """Long-row graphs (power laws): virtual rows for the heavy rows, the light rows through the second stage.
        Only for graphs that were validated at build (the split needs host readbacks).  Rule refitted in round 4
        (tools/kernel_choice_sweep.py, Zipf(1.1) degrees, 6.4 M edges: planned / split time 1.15-2.7 on every table up
        to 275 MB at EVERY average degree from 16 — the light-row second stage made the split form independent of the
        degree —, 1.0-1.04 at 410-550 MB, 0.7-0.9 from 800 MB unless the average degree is in the hundreds)."""
        if FORCE_KERNEL is not None or regular is not False or not self._S.validated:
            return False
        table = n_cols * F * 4
        n_virtual_bound = n_rows + self.nnz // SPLIT_ROW_EDGES
        if F % 4 != 0 or n_virtual_bound * SlicedCSR.N_SLICES >= 2 ** 31 - 1 or table < SPLIT_MIN_TABLE_BYTES:
            return False
        degree = self.nnz / max(n_rows, 1)
        if degree < SPLIT_MIN_DEGREE:
            return False
        return table <= (SPLIT_MAX_TABLE_BYTES_DENSE if degree >= SPLIT_DENSE_DEGREE else SPLIT_MAX_TABLE_BYTES)

    def _few_long_rows(self, F: int, n_rows: int, n_cols: int) -> bool:
        """A REGULAR graph of few, long rows whose XCD slices of the table exceed an L2 (a config-5 edge-scaled shard:
        6 250 rows of 1 600 edges over 100 000 sources): below 32 768 rows the launcher keeps one full-width pass (half-
        width groups would leave too few waves), so the slice spills — cut into 256-edge virtual rows there are enough rows
        for the column passes again (tools/long_rows_probe.py: 0.371 -> 0.322 ms, 0.345 -> 0.302, 0.339 -> 0.308; no gain
        where a slice already fits: 0.247 -> 0.254)."""
        if FORCE_KERNEL is not None or not self._S.validated or n_rows >= COLUMN_PASS_MIN_ROWS:
            return False
        slice_bytes = (n_cols + SlicedCSR.N_SLICES - 1) // SlicedCSR.N_SLICES * F * 4
        return self.nnz >= LONG_ROW_MIN_DEGREE * max(n_rows, 1) and slice_bytes > (4 << 20)

    @staticmethod
    def _plan_if_needed(plan, max_deg):
        """A plan only cuts rows longer than its chunk; when a readback has told that none is (every kNN-4 graph, every
        small slice), the wave-per-row launch does the same work in ONE launch — the planned form's second kernel,
        which adds the chunks of long rows, would start, find none and leave: 4-5 us each, 16 of them per training step
        at the reference's dataset sizes."""
        if plan is not None and max_deg is not None and max_deg <= plan.chunk:
            return None
        return plan

    def _built(self, D: _Direction) -> _Direction:
        """``D`` with its CSR (and plan) in place: the transposed direction's is made by its first use."""
        if D.indptr is None:
            S = self._S
            D.indptr, D.indices, D.eid = csr_from_coo(S.src, S.dst, S.n_src)
            D.plan = build_plan(D.indptr, S.nnz) if S.planned else None
        return D

    def _t_struct(self):
        T = self._built(self._S.bwd)
        return T.indptr, T.indices, T.eid, T.plan

    def transposed(self):
        """(indptr_t, indices_t, vals_t, plan_t): CSR of the reversed edges, rows = source nodes."""
        T = self._built(self._S.bwd)
        return T.indptr, T.indices, self._vals_for(T.csr_key, T.eid), T.plan

    def _run(self, D: _Direction, X, col_scale, row_scale, out, epi):
        """The planned or (no plan, or no row longer than its chunk) the wave-per-row product of direction ``D``."""
        dev = D.indptr.device
        if not X.is_cuda or X.device != dev:
            _require_device(D.indptr, X)
        if X.dim() == 2 and X.shape[0] != D.n_cols:
            raise RuntimeError("X has %d rows, the graph has %d source nodes" % (X.shape[0], D.n_cols))
        return _launch_spmm(dev, D.indptr, D.indices, self._vals_for(D.csr_key, D.eid), X,
                            None if col_scale is None else col_scale.reshape(-1),
                            None if row_scale is None else row_scale.reshape(-1), out, self._plan_if_needed(D.plan, D.max_deg),
                            D.n_rows, D.n_cols, 0, 0, D.eid if self._keep is not None else None, self._keep, epi)

    # -- bf16 gather ------------------------------------------------------------------
    def _bf16_gather_reason(self, F: int, D: _Direction) -> Optional[str]:
        """None when a product of width ``F`` in direction ``D`` gathers bf16 on request, else why it does not.  The form
        rule (``_use_sliced``) keeps judging the FLOAT32 table bytes: its thresholds were fitted to 4-byte rows."""
        if F % 8 != 0:
            return "F = %d is not a multiple of 8 (a lane loads 8 bf16 columns)" % F
        if (bool(D.regular) and self._few_long_rows(F, D.n_rows, D.n_cols)) or not self._use_sliced(F, D.n_rows, D.n_cols, D.regular):
            return ("a %d x %d product at F = %d does not take the plain XCD-local form (it runs the planned, wave-per-row "
                    "or split kernels, which gather float32 only)" % (D.n_rows, D.n_cols, F))
        return None

    def takes_bf16_gather(self, F: int, transposed: bool = False) -> bool:
        """Whether ``spmm`` (``transposed=True``: ``spmm_t``) honours ``gather_dtype=torch.bfloat16`` at width ``F``:
        the product takes the plain XCD-local form and ``F % 8 == 0``.  Otherwise a float32 ``X`` silently takes the
        float32 path and a bfloat16 ``X`` raises."""
        D = self._S.bwd if transposed else self._S.fwd
        if D.regular is None:
            self._decide_regular(torch.empty((0, int(F)), dtype=torch.float32, device=self.device), D)
        return self._bf16_gather_reason(int(F), D) is None

    def _bf16_request(self, X, out, gather_dtype, D: _Direction) -> bool:
        """True: gather bf16 on the plain XCD-local form.  False: the float32 product.  Raises for a bfloat16 ``X`` that
        cannot be gathered."""
        if X.dtype != torch.bfloat16 and _resolve_gather_dtype(gather_dtype) != torch.bfloat16:
            return False
        if X.dim() != 2:
            reason = "X is not 2-D"
        else:
            reason = self._bf16_gather_reason(X.shape[1], D)
            if reason is None and not _sliced_bf16_ok(X, out):
                reason = "the rows of X (or out) are not contiguous and 16-byte aligned"
        if reason is not None and X.dtype == torch.bfloat16:
            raise RuntimeError("a bfloat16 X is only taken by the XCD-local bf16 gather, and %s: pass the float32 table" % reason)
        return reason is None

    def _plain_layout(self, D: _Direction, F: int, gathered_scale):
        """``(name, layout)`` of the plain float32 XCD-local product of width ``F``; ``name`` keys this view's per-layout
        values, id words and compacted copies.

        The library says how many source slices the layout of a product should have (``dgmi_sliced_layout_slices``: 8
        unless the product is of the class the workgroup-owned form runs faster on 16, or ``sliced_owned_slices``
        forces a count).  Only a product that form can take is asked about: unit values or multiplicities in the id
        words, no edge dropout evaluated inside the kernel (a compacted view runs the plain kernels), and a scale on
        the gathered rows only where the pre-scale pass takes it out of the kernel.  Every other product runs the pair on
        the 8-slice layout; the bf16 gather stays on that layout too (there the library runs its owned form for the
        measured bf16 classes), as does every shape the library answers 8 for.  Which layout a
        product runs on depends on the product alone, never on what the graph has built before (:meth:`_layout_of`)."""
        n = SlicedCSR.N_SLICES
        mf = self._mult_form()
        if (self._coo_vals is None or mf is not None) and (self._keep is None or COMPACT_DROPPED):
            n = _lib.sliced_layout_slices(D.n_rows, D.n_cols, F, mf is not None)
            scaled = gathered_scale is not None or (mf is not None and (mf[0] == "row") == D.transposed)
            if n != SlicedCSR.N_SLICES and scaled and not SlicedCSR._prescale_rule(D.n_cols * F * 4, False, D.n_rows, n, self.nnz):
                n = SlicedCSR.N_SLICES  # the scale would be gathered inside the kernel: the pair's product
        return self._layout_of(D, n)

    def _layout_of(self, D, n_slices: int = SlicedCSR.N_SLICES):
        """``(name, layout)``: the XCD-sliced layout of ``n_slices`` source slices of direction ``D`` (the record, or
        whether it is the transposed one), built on first use.  The first layout a graph builds per direction sits in
        the record (``sliced`` / ``sliced_t``, name ``"sliced"`` / ``"sliced_t"``), one of another slice count beside
        it in ``wide`` (name ``"sliced/<n>"``): a graph whose products all run on one layout holds one."""
        if D.__class__ is not _Direction:
            D = self._S.bwd if D else self._S.fwd
        first = D.sliced
        if first is not None and first.n_slices == n_slices:
            return D.sliced_key, first
        layout = None if first is None else self._S.wide.get((D.transposed, n_slices))
        if layout is None:
            self._built(D)
            layout = SlicedCSR.from_csr(D.indptr, D.indices, D.eid, D.n_rows, D.n_cols, n_slices)  # one partition pass, no sort
            if first is not None:
                self._S.wide[(D.transposed, n_slices)] = layout
            else:
                D.sliced = layout
        return (D.sliced_key if first is None else "%s/%d" % (D.sliced_key, n_slices)), layout

    def _product(self, D: _Direction, X, gathered_scale, out_scale, out, epi, gather_dtype):
        """``diag(out_scale) M diag(gathered_scale) X`` with ``M`` the matrix of direction ``D`` (``A`` or ``A^T``): every
        route decision of :meth:`spmm` and :meth:`spmm_t`.  ``gathered_scale`` multiplies the gathered rows (with a bf16
        gather it is folded into the conversion of a float32 ``X``), ``out_scale`` the output rows."""
        if D.regular is None:  # one-time readback of this direction's maximum degree, when it can matter
            self._decide_regular(X, D)
        two_d = X.dim() == 2
        F = X.shape[1] if two_d else 0
        bf16 = self._bf16_request(X, out, gather_dtype, D)  # True: the plain XCD-local form, checked for this X and out
        long_rows = not bf16 and two_d and bool(D.regular) and self._few_long_rows(F, D.n_rows, D.n_cols)
        if bf16 or (two_d and not long_rows and self._use_sliced(F, D.n_rows, D.n_cols, D.regular) and _sliced_ok(X, out)):
            # the bf16 gather stays on the pair's 8 slices: the library runs its owned form on them where it wins
            name, layout = self._layout_of(D) if bf16 else self._plain_layout(D, F, gathered_scale)
            mult = self._mult_ids(name, layout)
            stable = None if gathered_scale is None else gathered_scale.reshape(-1)  # ONE tensor that outlives the call, or None
            if mult is not None:
                # values = scale x multiplicity.  The scale is indexed by the destination ("row": D^-1 M) or by the source
                # ("col": M D^-1): the output rows of one direction, the gathered rows of the other
                if (mult[0] == "row") != D.transposed:
                    out_scale = self._fold(mult[1], out_scale)
                else:
                    stable = mult[1] if gathered_scale is None else None  # folded anew per call: no constant
                    gathered_scale = self._fold(mult[1], gathered_scale)
            gd = None
            if bf16:
                if X.dtype != torch.bfloat16:
                    gd = torch.bfloat16
                elif gathered_scale is not None:
                    raise RuntimeError("a bfloat16 X cannot take a scale on the gathered rows (src_scale, or the row scale of this "
                                       "graph's `scale x multiplicity` values): it is applied in float32 before the one rounding — "
                                       "pass the float32 table")
            c = self._compacted(name, layout, mult)
            if c is not None:
                return c.spmm(X, gathered_scale, out_scale, out, epi=epi, gather_dtype=gd)
            if stable is not None and not bf16 and self._keep is None and (mult is not None or self._coo_vals is None):
                y = self._scaled_product(name, layout, X, stable, mult, out_scale, out, epi)
                if y is not None:
                    return y
            if mult is not None:
                return layout.spmm(X, gathered_scale, out_scale, out, vals=None, keep=self._keep, epi=epi, indices=mult[2],
                                   id_mult=True, gather_dtype=gd)
            return layout.spmm(X, gathered_scale, out_scale, out, vals=self._vals_for(name, layout.eid), keep=self._keep, epi=epi,
                               gather_dtype=gd)
        if two_d and _sliced_ok(X, out) and (self._use_split(F, D.n_rows, D.n_cols, D.regular) or (
                long_rows and self._use_sliced(F, D.n_rows, D.n_cols, D.regular))):
            split = D.split
            if split is None:
                split = D.split = _SplitSliced(D.indptr, D.eid, D.cols_coo, D.n_rows, D.n_cols)
            c = self._compacted(D.split_key, split.sliced)
            return split.spmm(X, _prep_scale(gathered_scale, D.n_cols, D.gathered_name), _prep_scale(out_scale, D.n_rows, D.out_name),
                              out, None if c is not None else self._vals_for(D.split_key, split.sliced.eid), keep=self._keep,
                              epi=epi, compacted=c, c_vals=self._combine_vals(D.split_key, split))
        return self._run(D, X, gathered_scale, out_scale, out, epi)

    def _scaled_product(self, name, layout, X, scale, mult, out_scale, out, epi):
        """The plain float32 product of ``layout`` with the single stable ``scale`` on its gathered rows through the
        owned form's scaled kernel and coded id words (:meth:`_scale_ids`), or None — the caller then runs the pre-scale
        pass and the plain product, as for every product the library declines (``dgmi_spmm_owned_scaled_takes``), for a
        scale of too many patterns, inside a capture, and where the pass would not have been made either."""
        F = X.shape[1]
        if not SCALE_CODES or layout.n_src > SCALE_MAX_IDS or scale.shape[0] != layout.n_src or X.shape[0] != layout.n_src:
            return None
        if not X.is_cuda or X.device != layout.segptr.device or scale.device != X.device:
            return None  # the plain path raises its error for operands on another device
        if self._v.get(name + "/scale_ids") is False or not layout._prescale_pays(layout.n_src * F * 4, False):
            return None
        takes = lambda n: _lib.owned_scaled_takes(layout.n_dst, layout.n_src, F, X.stride(0), layout.n_slices, mult is not None, n)
        if not takes(1):
            return None
        act, slope, mask, mask_scale = epi or _NO_EPI
        if mask is not None and not (mask.dtype == torch.float32 and mask.dim() == 2 and tuple(mask.shape) == (layout.n_dst, F)
                                     and mask.device == X.device and mask.stride(1) == 1 and mask.stride(0) % 4 == 0
                                     and mask.data_ptr() % 16 == 0):
            return None
        coded = self._scale_ids(name, scale, layout.indices if mult is None else mult[2])
        if coded is None or not takes(coded[0].shape[0]):
            return None
        ds = _prep_scale(out_scale, layout.n_dst, "dst_scale")
        if ds is not None and (not ds.is_cuda or ds.device != X.device):
            return None
        y = torch.empty((layout.n_dst, F), dtype=torch.float32, device=X.device) if out is None else out
        if tuple(y.shape) != (layout.n_dst, F) or y.dtype != torch.float32 or y.device != X.device:
            return None
        if not _lib.spmm_owned_scaled(layout.segptr, coded[1], X, coded[0], ds, y, layout.n_src, layout.n_slices,
                                      mult is not None, (act, slope, mask, mask_scale)):
            return None
        return y

    def spmm(self, X, src_scale=None, dst_scale=None, out=None, epi=None, gather_dtype=None):
        """``diag(dst_scale) A diag(src_scale) X`` (no autograd).  Picks the XCD-local sliced kernel when the
        feature table is a few L2s large and the graph is regular, else the planned kernel.  ``epi``: output epilogue
        (act, slope, out_mask, mask_scale), fused into the kernel that writes the result.  ``gather_dtype`` (default:
        :func:`gather_precision`'s): ``torch.bfloat16`` gathers from a bf16 copy of ``diag(src_scale) X`` where
        :meth:`takes_bf16_gather` holds, and is the float32 product elsewhere."""
        return self._product(self._S.fwd, X, src_scale, dst_scale, out, epi, gather_dtype)

    def spmm_t(self, dY, src_scale=None, dst_scale=None, out=None, gather_dtype=None):
        """``diag(src_scale) A^T diag(dst_scale) dY`` — the backward of :meth:`spmm`.  With a bf16 gather ``dst_scale``
        is folded into the conversion of ``dY`` and ``src_scale`` is applied by the plane reduce."""
        return self._product(self._built(self._S.bwd), dY, dst_scale, src_scale, out, None, gather_dtype)


class _SpMM(torch.autograd.Function):
    @staticmethod
    def forward(ctx, X, g: CSRGraph, src_scale, dst_scale, gather_dtype=torch.float32):
        ctx.g, ctx.gather_dtype = g, gather_dtype  # the backward may run outside a gather_precision block
        ctx.save_for_backward(src_scale, dst_scale)
        return g.spmm(X, src_scale, dst_scale, gather_dtype=gather_dtype)

    @staticmethod
    def backward(ctx, dY):
        src_scale, dst_scale = ctx.saved_tensors
        dX = None
        if ctx.needs_input_grad[0]:
            # dX = diag(src_scale) A^T diag(dst_scale) dY : the same kernel on the reversed
            # edges with the two scales swapped.  (An expanded / strided gradient — `y.sum().backward()` hands one over —
            # is made dense first: the XCD-local form needs 16-B aligned rows, and a 51 MB copy is 20 us against the 0.4 ms
            # the planned kernel would lose.)
            if not dY.is_contiguous():
                dY = dY.contiguous()
            dX = ctx.g.spmm_t(dY, src_scale, dst_scale, gather_dtype=ctx.gather_dtype)
        return dX, None, None, None, None


class _SpMMEpilogue(torch.autograd.Function):
    """``mask * mask_scale * act(diag(ds) A diag(ss) X)`` with the activation and the dropout mask
    applied by the kernel that writes the product (f3, reference layers.py:134-138)."""

    @staticmethod
    def forward(ctx, X, g: CSRGraph, src_scale, dst_scale, act, slope, mask, mask_scale, gather_dtype=torch.float32):
        y = g.spmm(X, src_scale, dst_scale, epi=(act, slope, mask, mask_scale), gather_dtype=gather_dtype)
        ctx.g, ctx.epi, ctx.gather_dtype = g, (act, slope, mask_scale), gather_dtype
        ctx.save_for_backward(src_scale, dst_scale, y, mask)
        return y

    @staticmethod
    def backward(ctx, dY):
        src_scale, dst_scale, y, mask = ctx.saved_tensors
        act, slope, mask_scale = ctx.epi
        dX = None
        if ctx.needs_input_grad[0]:
            g_pre = epilogue_backward(dY.contiguous(), y, mask, act, slope, mask_scale)
            dX = ctx.g.spmm_t(g_pre, src_scale, dst_scale, gather_dtype=ctx.gather_dtype)
        return dX, None, None, None, None, None, None, None, None


def colsum_rows_(feat_ext, coef, n: int, R: int, i0: int):
    """In place: rows ``[n*R, n*R + B)`` of ``feat_ext`` <- ``coef @ feat_ext[i0::R][:n]`` — the per-block column sums of
    the complement form (``dgmi_weighted_colsum_f32``)."""
    _require_device(feat_ext, coef)
    _T.colsum_rows_(feat_ext, coef, n, R, i0)
    return feat_ext


def colsum_rows_backward_(gf, coef, gs, n: int, R: int, i0: int):
    """In place: ``gf[i0::R] += coef^T @ gs`` (``dgmi_rank_add_f32``)."""
    _require_device(gf, coef, gs)
    _T.colsum_rows_backward_(gf, coef, gs, n, R, i0)
    return gf


def epilogue_backward(dY, Y, mask, act, slope, mask_scale):
    """``dY * act'(Y) * mask * mask_scale`` in one pass (``dgmi_epilogue_backward_f32``)."""
    _require_device(dY, Y, mask)
    return _T.epilogue_backward(dY, Y, mask, act, slope, mask_scale)


def spmm_csr_act_dropout(g: CSRGraph, X, src_scale=None, dst_scale=None, act: int = 0, slope: float = 0.0,
                         mask: Optional[torch.Tensor] = None, mask_scale: float = 1.0, gather_dtype=None) -> torch.Tensor:
    """:func:`spmm_csr` followed by ``leaky_relu`` (``act=1``) and a dropout keep ``mask`` (0/1 floats of
    the output's shape, scaled by ``mask_scale``), both inside the product's last kernel."""
    if src_scale is not None and src_scale.requires_grad or dst_scale is not None and dst_scale.requires_grad:
        raise RuntimeError("spmm_csr: gradients w.r.t. the diagonal scales are not part of the path")
    return _SpMMEpilogue.apply(X, g, src_scale, dst_scale, act, slope, mask, mask_scale, _resolve_gather_dtype(gather_dtype))


def spmm_csr(g: CSRGraph, X: torch.Tensor, src_scale: Optional[torch.Tensor] = None,
             dst_scale: Optional[torch.Tensor] = None, gather_dtype=None) -> torch.Tensor:
    """``Y = diag(dst_scale) · A · diag(src_scale) · X`` with autograd w.r.t. ``X`` only.

    The reference needs no other gradient: adjacency values are constants (utils.py:24-27,
    augmentation.py:124) and ``ci``/``cj`` are non-learnable node data (data_loader.py:487-488).
    ``gather_dtype`` (default: :func:`gather_precision`'s): see :meth:`CSRGraph.spmm`; the backward,
    ``dX = diag(ss) A^T diag(ds) dY``, gathers ``dY`` in the same precision wherever it runs.
    """
    if src_scale is not None and src_scale.requires_grad or dst_scale is not None and dst_scale.requires_grad:
        raise RuntimeError("spmm_csr: gradients w.r.t. the diagonal scales are not part of the path")
    return _SpMM.apply(X, g, src_scale, dst_scale, _resolve_gather_dtype(gather_dtype))


# ---------------------------------------------------------------------------------------------
# (f2) decoder edge gather-concat: graph.apply_edges(udf_u_mul_e) — layers.py:364,378-379
# ---------------------------------------------------------------------------------------------
def _check_tables(A, B, n_src, n_dst):
    """The feature tables must cover the id ranges the edge list was validated against
    (``EdgePairs``): DGL would raise on a node-data / node-count mismatch; reading past a short
    table on the GPU must not be an option."""
    if n_src is not None and A.shape[0] < n_src:
        raise RuntimeError("source feature table has %d rows, the edge list addresses %d source nodes" % (A.shape[0], n_src))
    if n_dst is not None and B.shape[0] < n_dst:
        raise RuntimeError("destination feature table has %d rows, the edge list addresses %d destination nodes"
                           % (B.shape[0], n_dst))


def gather_concat_raw(src, dst, A, B, out=None, n_src=None, n_dst=None) -> torch.Tensor:
    """``out[e] = cat(A[src[e]], B[dst[e]])`` through ``dgmi_gather_concat_f32`` (no autograd).
    ``n_src`` / ``n_dst``: the node counts ``src`` / ``dst`` ids were range-checked against."""
    _require_device(src, dst, A, B, out)
    _check_tables(A, B, n_src, n_dst)
    y = _T.gather_concat_raw(src, dst, A, B)
    if out is not None:
        out.copy_(y)
        return out
    return y


class EdgePairs:
    """The decoder graph's edge list (data_loader.py:492-509) in the layout the kernels read:
    int32 ``src``/``dst`` ids plus, built lazily for the backward, the two CSRs whose
    ``indices`` are *edge ids* grouped by source node and by destination node (so that
    ``copy_e -> sum`` is the SpMM kernel gathering rows of d_out)."""

    def __init__(self, src: torch.Tensor, dst: torch.Tensor, n_src: int, n_dst: int, check_range: bool = True):
        _require_device(src, dst)
        self.src = src.to(torch.int32).contiguous()
        self.dst = dst.to(torch.int32).contiguous()
        self.n_src, self.n_dst = int(n_src), int(n_dst)
        self.E = int(self.src.shape[0])
        if check_range and self.E:
            lo = torch.stack([self.src.min(), self.dst.min()]).min()
            hi_s, hi_d = self.src.max(), self.dst.max()
            lo, hi_s, hi_d = (int(v) for v in torch.stack([lo, hi_s, hi_d]).tolist())
            if lo < 0 or hi_s >= self.n_src or hi_d >= self.n_dst:
                raise RuntimeError("decoder edge id out of range")
        self._by_src = self._by_dst = None

    def _group(self, key, n):
        iota = torch.arange(self.E, dtype=torch.int32, device=key.device)
        # every row of the gathered (E, F) matrix is used exactly ONCE (the column ids are a permutation of the edge
        # ids): no reuse for the XCD-local form to keep in L2 — vouch "not regular" so that it is never chosen
        g = CSRGraph(key, iota, n, self.E, check_range=False, regular=False, regular_t=False)
        return g

    def by_src(self) -> "CSRGraph":
        if self._by_src is None:
            self._by_src = self._group(self.src, self.n_src)
        return self._by_src

    def by_dst(self) -> "CSRGraph":
        if self._by_dst is None:
            self._by_dst = self._group(self.dst, self.n_dst)
        return self._by_dst


class _GatherConcat(torch.autograd.Function):
    @staticmethod
    def forward(ctx, A, B, pairs: EdgePairs):
        ctx.pairs = pairs
        ctx.Fa, ctx.Fb = A.shape[1], B.shape[1]
        return gather_concat_raw(pairs.src, pairs.dst, A, B, n_src=pairs.n_src, n_dst=pairs.n_dst)

    @staticmethod
    def backward(ctx, dOut):
        pairs, Fa, Fb = ctx.pairs, ctx.Fa, ctx.Fb
        dOut = dOut.contiguous()
        dA = dB = None
        if ctx.needs_input_grad[0]:  # dA[u] = sum over edges leaving u of d_out[e, :Fa]
            dA = pairs.by_src().spmm(dOut[:, :Fa])
        if ctx.needs_input_grad[1]:  # dB[v] = sum over edges entering v of d_out[e, Fa:]
            dB = pairs.by_dst().spmm(dOut[:, Fa:])
        return dA, dB, None


def gather_concat(pairs: EdgePairs, A: torch.Tensor, B: torch.Tensor) -> torch.Tensor:
    """Differentiable ``cat(A[src], B[dst])`` over the decoder edges."""
    return _GatherConcat.apply(A, B, pairs)


def gather_add_raw(src, dst, A, B, bias=None, out=None, n_src=None, n_dst=None, act: int = 0) -> torch.Tensor:
    """``out[e] = A[src[e]] + B[dst[e]] (+ bias)`` through ``dgmi_gather_add_f32`` (no autograd); ``act=1``: relu of it,
    in the same pass."""
    _require_device(src, dst, A, B, bias, out)
    _check_tables(A, B, n_src, n_dst)
    y = _T.gather_add_raw(src, dst, A, B, bias, int(act))
    if out is not None:
        out.copy_(y)
        return out
    return y


class _GatherAdd(torch.autograd.Function):
    @staticmethod
    def forward(ctx, A, B, bias, pairs: EdgePairs):
        ctx.pairs = pairs
        return gather_add_raw(pairs.src, pairs.dst, A, B, bias, n_src=pairs.n_src, n_dst=pairs.n_dst)

    @staticmethod
    def backward(ctx, dOut):
        pairs = ctx.pairs
        dOut = dOut.contiguous()
        dA = pairs.by_src().spmm(dOut) if ctx.needs_input_grad[0] else None
        dB = pairs.by_dst().spmm(dOut) if ctx.needs_input_grad[1] else None
        dbias = dOut.sum(0) if ctx.needs_input_grad[2] else None
        return dA, dB, dbias, None


def gather_add(pairs: EdgePairs, A: torch.Tensor, B: torch.Tensor, bias: Optional[torch.Tensor] = None):
    """Differentiable ``A[src] + B[dst] (+ bias)`` over the decoder edges."""
    return _GatherAdd.apply(A, B, bias, pairs)


class _GatherAddReluDropout(torch.autograd.Function):
    """``dropout(relu(A[src] + B[dst] + bias))`` — the decoder's first stage (layers.py:364-367 with ``lin1`` folded
    into the node tables).  Forward: the relu rides in the gather-add kernel's store (one E x F pass less), the dropout
    is torch's own (same RNG consumption as ``nn.Dropout`` on that shape).  Backward: ONE gating pass from the output
    (``y > 0`` exactly where the sum was positive and the element was kept: ``dgmi_epilogue_backward_f32`` act 2), then
    the two segment sums of :class:`_GatherAdd`."""

    @staticmethod
    def forward(ctx, A, B, bias, pairs: EdgePairs, p: float):
        y = gather_add_raw(pairs.src, pairs.dst, A, B, bias, n_src=pairs.n_src, n_dst=pairs.n_dst, act=1)
        y = torch.nn.functional.dropout(y, p, True)
        ctx.pairs, ctx.scale = pairs, 1.0 / (1.0 - p)
        ctx.save_for_backward(y)
        return y

    @staticmethod
    def backward(ctx, dY):
        (y,) = ctx.saved_tensors
        pairs = ctx.pairs
        dZ = epilogue_backward(dY.contiguous(), y, None, 2, 0.0, ctx.scale)
        dA = pairs.by_src().spmm(dZ) if ctx.needs_input_grad[0] else None
        dB = pairs.by_dst().spmm(dZ) if ctx.needs_input_grad[1] else None
        dbias = dZ.sum(0) if ctx.needs_input_grad[2] else None
        return dA, dB, dbias, None, None


def gather_add_relu_dropout(pairs: EdgePairs, A, B, bias, p: float):
    """Differentiable ``dropout(relu(A[src] + B[dst] + bias), p)`` in training mode (``0 < p < 1``)."""
    return _GatherAddReluDropout.apply(A, B, bias, pairs, float(p))


# ---------------------------------------------------------------------------------------------
# (f4) cosine-similarity kNN — data_loader.py:312-344 without the N x N similarity matrix
# ---------------------------------------------------------------------------------------------
def knn_cosine_supported(N: int, D: int, k: int) -> bool:
    """Whether the fused MFMA kNN kernel takes this shape (``dgmi_knn_cosine_supported``)."""
    return bool(_L.dgmi_knn_cosine_supported(int(N), int(D), int(k)))


def knn_cosine_topk(xn: torch.Tensor, k: int) -> torch.Tensor:
    """``(N, k)`` int32 ids of the k largest cosine similarities per row of the row-normalised ``xn``
    (self included, descending) — ``dgmi_knn_cosine_topk_f32``: fp32-MFMA similarity tiles reduced to
    a running top-k on chip.

    Non-finite rows (``include/dgmi.h``): a row that holds a NaN is in no other row's list and its own list is ``k``
    times ``-1``; a finite row's list is its top ``min(k, #finite rows)`` finite rows followed by ``-1`` (the only
    filler), the same rows the call returns on the finite rows alone; rows with ``+-inf`` elements get valid-or-``-1``
    distinct ids in unspecified order.  No bit pattern in ``xn`` makes the search read or write outside ``xn``, the
    result and its workspace.  The call does not synchronise and does not look at the lists: a caller that gathers with
    them checks for ``-1`` first (``graph.feature_similarity_graph`` refuses non-finite features before it calls)."""
    _require_device(xn)
    return _T.knn_cosine_topk(xn, int(k))


# ---------------------------------------------------------------------------------------------
# all-pairs decoder top-k — the scoring loop of train.py:26-151 without the pair list
# ---------------------------------------------------------------------------------------------
PAIR_TOPK_MAX_K = _lib.PAIR_TOPK_MAX_K


def pair_mlp_topk(P: torch.Tensor, Q: torch.Tensor, W2: torch.Tensor, b2: torch.Tensor, w3: torch.Tensor,
                  b3: torch.Tensor, known_drug: Optional[torch.Tensor], known_dis: Optional[torch.Tensor],
                  k: int) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """The ``min(k, #candidates)`` pairs ``(i, j)`` not in ``(known_drug, known_dis)`` with the largest
    ``logit = b3 + w3 . relu(W2 relu(P[i] + Q[j]) + b2)`` (``dgmi_pair_mlp_topk_f32``), ordered by logit descending,
    ties by ``(i, j)`` ascending, NaN last.  ``P`` (n_drug x 128), ``Q`` (n_dis x 128); ``W2`` (64 x 128), ``b2``,
    ``w3`` (64), ``b3`` (1).  Returns int64 drug ids, int64 disease ids and fp32 logits on the device; the only
    host sync is reading the count.  Raises ``ValueError`` for ``k`` outside 1..1024 and ``RuntimeError`` when a
    known id is out of range."""
    k = int(k)
    if not 1 <= k <= PAIR_TOPK_MAX_K:
        raise ValueError("k must be in 1..%d (the on-chip top-k limit), got %d" % (PAIR_TOPK_MAX_K, k))
    _require_device(P, Q, W2, b2, w3, b3, known_drug, known_dis)
    drug, dis, logit, info = _T.pair_mlp_topk(P, Q, W2, b2.reshape(-1), w3.reshape(-1), b3.reshape(-1), known_drug,
                                              known_dis, k)
    n, bad = (int(v) for v in info.tolist())
    if bad:
        raise RuntimeError("pair_mlp_topk: a known (drug, disease) id is outside [0, %d) x [0, %d)"
                           % (P.shape[0], Q.shape[0]))
    return drug[:n].long(), dis[:n].long(), logit[:n]


ROW_TOPK_MAX_K = _lib.ROW_TOPK_MAX_K


def pair_mlp_row_topk(X: torch.Tensor, C: torch.Tensor, W2: torch.Tensor, b2: torch.Tensor, w3: torch.Tensor,
                      b3: torch.Tensor, known_query: Optional[torch.Tensor], known_cand: Optional[torch.Tensor],
                      k: int) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """For every query row ``q`` of ``X``, the ``min(k, #candidates of q)`` rows ``c`` of ``C`` with ``(q, c)`` not in
    ``(known_query, known_cand)`` and the largest ``logit = b3 + w3 . relu(W2 relu(X[q] + C[c]) + b2)``
    (``dgmi_pair_mlp_row_topk_f32``), ordered by logit descending, ties by ``c`` ascending, NaN last.  Per-disease lists
    take ``X = Q``, ``C = P``; per-drug lists ``X = P``, ``C = Q``; every logit is bit-identical to
    :func:`pair_mlp_topk`'s for the same pair.  Returns int64 candidate ids ``(n_query, k)`` (-1 past a row's count), fp32
    logits ``(n_query, k)`` (NaN past the count) and int32 counts ``(n_query,)`` on the device; the only host sync is
    reading the flag.  Raises ``ValueError`` for ``k`` outside 1..128 and ``RuntimeError`` when a known id is out of
    range."""
    k = int(k)
    if not 1 <= k <= ROW_TOPK_MAX_K:
        raise ValueError("k must be in 1..%d (the per-row on-chip top-k limit), got %d" % (ROW_TOPK_MAX_K, k))
    _require_device(X, C, W2, b2, w3, b3, known_query, known_cand)
    cand, logit, count, info = _T.pair_mlp_row_topk(X, C, W2, b2.reshape(-1), w3.reshape(-1), b3.reshape(-1), known_query,
                                                    known_cand, k)
    if int(info[1]):
        raise RuntimeError("pair_mlp_row_topk: a known (query, candidate) id is outside [0, %d) x [0, %d)"
                           % (X.shape[0], C.shape[0]))
    return cand.long(), logit, count


# ---------------------------------------------------------------------------------------------
# every novel pair at or above a cut — the list a top-k cannot give, and the carrier of k > 1024
# ---------------------------------------------------------------------------------------------
PAIR_EMIT_MAX_RECORDS = _lib.PAIR_EMIT_MAX_RECORDS


class TooManyPairs(RuntimeError):
    """More pairs reach the cut than the caller allowed: ``count`` (exact) > ``max_pairs``.  Nothing is returned."""

    def __init__(self, count: int, max_pairs: int):
        super().__init__("%d novel pairs reach the cut, more than max_pairs = %d: raise the cut or max_pairs"
                         % (count, max_pairs))
        self.count = int(count)
        self.max_pairs = int(max_pairs)


def _check_max_pairs(max_pairs) -> int:
    max_pairs = int(max_pairs)
    if not 1 <= max_pairs <= PAIR_EMIT_MAX_RECORDS:
        raise ValueError("max_pairs must be in 1..%d (the record buffer limit), got %d" % (PAIR_EMIT_MAX_RECORDS, max_pairs))
    return max_pairs


def _pair_emit(P, Q, W2, b2, w3, b3, known_drug, known_dis, min_logit, capacity):
    """One emit pass into fresh record tensors of ``capacity`` slots: ``(drug, dis, logit, count)`` with the exact
    count as a Python int (the one host sync).  The records are unsorted; ``count`` may exceed ``capacity``."""
    _require_device(P, Q, W2, b2, w3, b3, known_drug, known_dis)
    drug = torch.empty(capacity, dtype=torch.int32, device=P.device)
    dis = torch.empty_like(drug)
    logit = torch.empty(capacity, dtype=torch.float32, device=P.device)
    count, info = _T.pair_mlp_emit(P, Q, W2, b2.reshape(-1), w3.reshape(-1), b3.reshape(-1), known_drug, known_dis,
                                   float(min_logit), drug, dis, logit)
    n, _, bad = (int(v) for v in torch.cat([count, info.long()]).tolist())  # one read for both
    if bad:
        raise RuntimeError("pair_mlp_emit: a known (drug, disease) id is outside [0, %d) x [0, %d)"
                           % (P.shape[0], Q.shape[0]))
    return drug, dis, logit, n


def pair_mlp_above(P: torch.Tensor, Q: torch.Tensor, W2: torch.Tensor, b2: torch.Tensor, w3: torch.Tensor,
                   b3: torch.Tensor, known_drug: Optional[torch.Tensor], known_dis: Optional[torch.Tensor],
                   min_logit: float, max_pairs: int = 1 << 20) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor, int]:
    """EVERY pair ``(i, j)`` not in ``(known_drug, known_dis)`` whose logit (that of :func:`pair_mlp_topk`, the same
    bits) is at or above ``min_logit`` (``dgmi_pair_mlp_emit_f32`` then ``dgmi_pair_records_sort_f32``), ordered by
    logit descending, ties by ``(i, j)`` ascending, NaN last.  The cut is inclusive in fp32, -0 and +0 are one value, a
    NaN logit reaches no numeric cut (-inf included); ``min_logit = NaN`` selects every novel pair, NaN logits included.
    Returns int64 drug ids, int64 disease ids, fp32 logits on the device and the exact count (their length); the only
    host sync is reading the count and the flag.  Raises :class:`TooManyPairs` (with the exact ``count``) when more
    than ``max_pairs`` pairs qualify, ``ValueError`` for ``max_pairs`` outside 1..2**24 and ``RuntimeError`` when a
    known id is out of range."""
    max_pairs = _check_max_pairs(max_pairs)
    drug, dis, logit, n = _pair_emit(P, Q, W2, b2, w3, b3, known_drug, known_dis, min_logit, max_pairs)
    if n > max_pairs:
        raise TooManyPairs(n, max_pairs)
    _T.pair_records_sort(drug, dis, logit, n)
    return drug[:n].long(), dis[:n].long(), logit[:n], n


def pair_mlp_count_above(P: torch.Tensor, Q: torch.Tensor, W2: torch.Tensor, b2: torch.Tensor, w3: torch.Tensor,
                         b3: torch.Tensor, known_drug: Optional[torch.Tensor], known_dis: Optional[torch.Tensor],
                         min_logit: float) -> int:
    """How many pairs :func:`pair_mlp_above` would list at this cut, without storing any (capacity 0): exact, no limit."""
    return _pair_emit(P, Q, W2, b2, w3, b3, known_drug, known_dis, min_logit, 0)[3]


# ---------------------------------------------------------------------------------------------
# given pairs — the logit of a listed pair and its filtered position in its row (hits@k, MRR)
# ---------------------------------------------------------------------------------------------
def _pair_list(pair_query, pair_cand):
    """The two id lists of a pair list, checked on the host: 1-D integer tensors of equal length (``ValueError``)."""
    for name, t in (("pair_query", pair_query), ("pair_cand", pair_cand)):
        if not isinstance(t, torch.Tensor) or t.dim() != 1 or t.dtype not in (torch.int32, torch.int64):
            raise ValueError("%s must be a 1-D int32 / int64 tensor of ids" % name)
    if pair_query.numel() != pair_cand.numel():
        raise ValueError("pair id lists differ in length: %d vs %d" % (pair_query.numel(), pair_cand.numel()))


def pair_mlp_score_list(X: torch.Tensor, C: torch.Tensor, W2: torch.Tensor, b2: torch.Tensor, w3: torch.Tensor,
                        b3: torch.Tensor, pair_query: torch.Tensor, pair_cand: torch.Tensor) -> torch.Tensor:
    """``logit = b3 + w3 . relu(W2 relu(X[q] + C[c]) + b2)`` of every listed pair ``(q, c) = (pair_query[e],
    pair_cand[e])`` (``dgmi_pair_mlp_score_list_f32``): fp32 on the device, in the caller's order, every logit
    bit-identical to the one :func:`pair_mlp_topk`, :func:`pair_mlp_row_topk` and :func:`pair_mlp_above` return for the
    pair.  Duplicates are allowed.  The only host sync is reading the flag.  Raises ``ValueError`` for id lists that
    are not 1-D integer tensors of equal length and ``RuntimeError`` when a listed id is out of range."""
    _pair_list(pair_query, pair_cand)
    _require_device(X, C, W2, b2, w3, b3, pair_query, pair_cand)
    logit, info = _T.pair_mlp_score_list(X, C, W2, b2.reshape(-1), w3.reshape(-1), b3.reshape(-1), pair_query, pair_cand)
    if int(info[0]):
        raise RuntimeError("pair_mlp_score_list: a listed (query, candidate) id is outside [0, %d) x [0, %d)"
                           % (X.shape[0], C.shape[0]))
    return logit


class _PairMlpTrain(torch.autograd.Function):
    """The decoder MLP on the training pair list, fused (``dgmi_pairs_train.hip``).  Forward: one kernel, saves the
    operands (node tables, parameters, the seed) and nothing per pair.  Backward: the kernels recompute the hidden layers
    with the same masks and return ``dZ1`` (E x 128) and the parameter gradients; ``dP`` / ``dQ`` are the two segment
    sums of :class:`_GatherAdd`."""

    @staticmethod
    def forward(ctx, P, Q, W2, b2, w3, b3, pairs: EdgePairs, p: float, seed):
        _check_tables(P, Q, pairs.n_src, pairs.n_dst)
        logit, _ = _T.pair_mlp_train_forward(P, Q, W2, b2.reshape(-1), w3.reshape(-1), b3.reshape(-1), pairs.src, pairs.dst,
                                             p, seed)
        ctx.pairs, ctx.p = pairs, p
        ctx.save_for_backward(P, Q, W2, b2, w3, b3, seed)
        return logit

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, dlogit):
        P, Q, W2, b2, w3, b3, seed = ctx.saved_tensors
        pairs = ctx.pairs
        dZ1, dW2, db2, dw3, db3, _ = _T.pair_mlp_train_backward(P, Q, W2, b2.reshape(-1), w3.reshape(-1), b3.reshape(-1),
                                                                pairs.src, pairs.dst, ctx.p, seed, dlogit.contiguous())
        need = ctx.needs_input_grad
        if pairs.E == 0:  # nothing to sum: no segment layout of an empty list is built
            dP, dQ = (torch.zeros_like(P) if need[0] else None), (torch.zeros_like(Q) if need[1] else None)
        else:
            dP = pairs.by_src().spmm(dZ1) if need[0] else None
            dQ = pairs.by_dst().spmm(dZ1) if need[1] else None
        return (dP, dQ, dW2 if need[2] else None, db2.reshape(b2.shape) if need[3] else None,
                dw3.reshape(w3.shape) if need[4] else None, db3.reshape(b3.shape) if need[5] else None, None, None, None)


def pair_mlp_train(P: torch.Tensor, Q: torch.Tensor, W2: torch.Tensor, b2: torch.Tensor, w3: torch.Tensor, b3: torch.Tensor,
                   pairs: EdgePairs, p: float, seed: Optional[torch.Tensor] = None) -> torch.Tensor:
    """``logit[e] = b3 + w3 . m2 relu(W2 (m1 relu(P[src_e] + Q[dst_e])) + b2)`` over the decoder's pair list, in training:
    ``m1`` / ``m2`` are dropout factors (``1 / (1 - p)`` or 0) drawn by a hash of ``(seed, layer, e, unit)``
    (``csrc/dgmi_pair_dropout.h``) — NOT torch's RNG stream.  One HIP kernel forward; the backward recomputes the hidden
    layers, so autograd keeps no ``E x H`` tensor.  Differentiable once in ``P``, ``Q`` and the four parameters; all sums
    are free of float atomics (bit-identical from run to run for one seed).  With ``p = 0`` every logit is
    :func:`pair_mlp_score_list`'s, bit for bit.

    ``seed``: a 1-element int64 device tensor, used as is (the kernels read it from device memory, so a captured step
    follows whatever the tensor holds at replay); ``None`` draws one on the device from torch's graph-aware generator.
    The tensor used is kept in ``pair_mlp_train.last_seed``.  The ids were range-checked by :class:`EdgePairs`; nothing
    here synchronises."""
    if not isinstance(pairs, EdgePairs):
        raise TypeError("pairs must be an ops.EdgePairs, got %s" % type(pairs).__name__)
    p = float(p)
    if not 0.0 <= p < 1.0:
        raise ValueError("dropout p must be in [0, 1), got %r" % (p,))
    _require_device(P, Q, W2, b2, w3, b3, seed)
    if seed is None:
        seed = torch.randint(0, 2 ** 62, (1,), dtype=torch.int64, device=P.device)
    elif seed.dtype != torch.int64 or seed.numel() != 1:
        raise ValueError("seed must be a 1-element int64 device tensor")
    seed = seed.reshape(1)
    pair_mlp_train.last_seed = seed
    return _PairMlpTrain.apply(P, Q, W2, b2, w3, b3, pairs, p, seed)


pair_mlp_train.last_seed = None


#: rows of one block and the largest grid of the attention kernels (``DGMI_ATTN_BLOCK_ROWS`` / ``DGMI_ATTN_MAX_WORKGROUPS``
#: of ``include/dgmi_attn.h``): block ``b`` belongs to workgroup ``b mod grid``, which fixes the order of the parameter sums
ATTN_FUSE_BLOCK_ROWS = 64
ATTN_FUSE_MAX_WORKGROUPS = 1024
_ATTN_HIDDEN = 16


class _AttentionFuse(torch.autograd.Function):
    """The two-channel attention fusion (``dgmi_attn.hip``).  Forward: one kernel; saves its inputs and nothing else.
    Backward: a recompute kernel and a fixed-order reduce.  ``b is None``: ``a`` is the stacked ``(n, 2, F)`` tensor, its
    two halves go to the kernels by leading dimension ``2 F`` and the backward writes both halves of one ``dz``."""

    @staticmethod
    def forward(ctx, a, b, W1, b1, w2, mult):
        A, B = (a[:, 0], a[:, 1]) if b is None else (a, b)
        out, beta = _T.attn_fuse_forward(A, B, mult, W1, b1.reshape(-1), w2.reshape(-1))
        ctx.stacked = b is None
        ctx.save_for_backward(a, b, W1, b1, w2, mult)
        ctx.mark_non_differentiable(beta)
        return out, beta

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, dout, _dbeta):
        a, b, W1, b1, w2, mult = ctx.saved_tensors
        A, B = (a[:, 0], a[:, 1]) if ctx.stacked else (a, b)
        dA, dB, dW1, db1, dw2 = _T.attn_fuse_backward(A, B, mult, W1, b1.reshape(-1), w2.reshape(-1), dout)
        need = ctx.needs_input_grad
        if ctx.stacked:
            n, F = dA.shape
            if n > 0 and dA.stride(0) == 2 * F and dB.data_ptr() == dA.data_ptr() + 4 * F:
                da = dA.as_strided((n, 2, F), (2 * F, F, 1))  # the op wrote the two halves of one tensor
            else:  # the op copied a misaligned view (or n = 0): two tables came back
                da = torch.stack([dA, dB], 1)
            db = None
        else:
            da, db = dA, dB
        return (da if need[0] else None, db if need[1] else None, dW1 if need[2] else None,
                db1.reshape(b1.shape) if need[3] else None, dw2.reshape(w2.shape) if need[4] else None, None)


def _check_attention(A, B, W1, b1, w2, mult):
    if A.dim() != 2 or B.dim() != 2 or A.shape != B.shape:
        raise ValueError("a and b must be two (n, F) tables of one shape, got %s and %s" % (tuple(A.shape), tuple(B.shape)))
    n, F = A.shape
    if F % 4 != 0 or not 4 <= F <= 512:
        raise ValueError("the width must be a multiple of 4 in [4, 512], got %d" % F)
    if W1.dim() != 2 or W1.shape[0] != _ATTN_HIDDEN or b1.numel() != _ATTN_HIDDEN or w2.numel() != _ATTN_HIDDEN:
        raise ValueError("only hidden size %d is supported: W1 %s, b1 %s, w2 %s"
                         % (_ATTN_HIDDEN, tuple(W1.shape), tuple(b1.shape), tuple(w2.shape)))
    if W1.shape[1] != F:
        raise ValueError("W1 must be (%d, %d), got %s" % (_ATTN_HIDDEN, F, tuple(W1.shape)))
    if mult is not None and tuple(mult.shape) != (n, 2):
        raise ValueError("mult must be (%d, 2), got %s" % (n, tuple(mult.shape)))
    for name, t in (("a", A), ("b", B), ("W1", W1), ("b1", b1), ("w2", w2), ("mult", mult)):
        if t is not None and t.dtype != torch.float32:
            raise ValueError("%s must be float32, got %s" % (name, t.dtype))


def attention_fuse(a: torch.Tensor, b: torch.Tensor, W1: torch.Tensor, b1: torch.Tensor, w2: torch.Tensor,
                   mult: Optional[torch.Tensor] = None):
    """``(out, beta)`` of the encoder's two-channel attention fusion, one HIP kernel (``include/dgmi_attn.h``)::

        s_c = w2 . tanh(W1 z_c + b1),  beta = softmax(s_0, s_1) * mult[n],  out[n] = beta_0 a[n] + beta_1 b[n]

    ``a``, ``b``: ``(n, F)`` fp32, ``F`` a multiple of 4 in [4, 512], rows contiguous (row-strided views are consumed in
    place); ``W1`` ``(16, F)``, ``b1`` and ``w2`` 16 entries; ``mult`` an optional ``(n, 2)`` multiplier (the dropout
    factors of the two weights; a constant).  ``b=None`` takes ``a`` as the stacked ``(n, 2, F)`` tensor.  ``out`` is
    ``(n, F)``, ``beta`` ``(n, 2)`` (after the multiplier) and NOT differentiable.  Differentiable once in ``a``, ``b``,
    ``W1``, ``b1``, ``w2``: the backward recomputes the hidden layer and the softmax, autograd keeps the inputs only, and
    every sum is free of float atomics (bit-identical from run to run).  Nothing here synchronises.

    Operand forms: a table that is column-strided, whose rows are no multiple of 4 floats apart or that starts off a
    16-byte boundary is copied by the op (the stacked form then gets its gradient as one stacked copy); a non-contiguous
    ``W1``, ``b1``, ``w2`` or ``mult`` (``lin.weight.t()`` of a transposed leaf, a column slice) is made contiguous here,
    and its gradient reaches the leaf in the leaf's layout; the upstream gradient may have any strides."""
    _require_device(a, b, W1, b1, w2, mult)
    if mult is not None and not mult.is_contiguous():
        mult = mult.contiguous()
    W1, b1, w2 = (t if t.is_contiguous() else t.contiguous() for t in (W1, b1, w2))
    if b is None:
        if a.dim() != 3 or a.shape[1] != 2:
            raise ValueError("the stacked form takes an (n, 2, F) tensor, got %s" % (tuple(a.shape),))
        _check_attention(a[:, 0], a[:, 1], W1, b1, w2, mult)
    else:
        _check_attention(a, b, W1, b1, w2, mult)
    return _AttentionFuse.apply(a, b, W1, b1, w2, mult)


def pair_mlp_rank_list(X: torch.Tensor, C: torch.Tensor, W2: torch.Tensor, b2: torch.Tensor, w3: torch.Tensor,
                       b3: torch.Tensor, pair_query: torch.Tensor, pair_cand: torch.Tensor,
                       known_query: Optional[torch.Tensor] = None,
                       known_cand: Optional[torch.Tensor] = None) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """``(logit, above, total)`` of every listed pair ``(q, c)`` (``dgmi_pair_mlp_rank_list_f32``): the logit of
    :func:`pair_mlp_score_list`, and over the candidates ``c' != c`` with ``(q, c')`` not in ``(known_query,
    known_cand)``: ``total``, how many there are, and ``above``, how many of them rank before ``(q, c)`` in the order of
    :func:`pair_mlp_row_topk` (logit descending, ties by candidate id ascending, NaN last).  ``above + 1`` is the pair's
    filtered rank among ``total + 1``.  The listed pair never counts itself, and whether it is in the known list changes
    nothing; duplicates get equal results.  int32 ``above`` / ``total`` on the device, in the caller's order.

    Cost: every listed pair scans its whole row, ``n_pairs x n_cand`` scores.  The only host sync is reading the
    flags.  Raises ``ValueError`` as :func:`pair_mlp_score_list` and ``RuntimeError`` when a listed or a known id is
    out of range."""
    _pair_list(pair_query, pair_cand)
    _require_device(X, C, W2, b2, w3, b3, pair_query, pair_cand, known_query, known_cand)
    logit, above, total, info = _T.pair_mlp_rank_list(X, C, W2, b2.reshape(-1), w3.reshape(-1), b3.reshape(-1), pair_query,
                                                      pair_cand, known_query, known_cand)
    bad_pair, bad_known = (int(v) for v in info.tolist())
    if bad_pair:
        raise RuntimeError("pair_mlp_rank_list: a listed (query, candidate) id is outside [0, %d) x [0, %d)"
                           % (X.shape[0], C.shape[0]))
    if bad_known:
        raise RuntimeError("pair_mlp_rank_list: a known (query, candidate) id is outside [0, %d) x [0, %d)"
                           % (X.shape[0], C.shape[0]))
    return logit, above, total


# ---------------------------------------------------------------------------------------------
# curve areas — exact AUROC / AUPR of scored samples on the device (evaluation.py:55-65)
# ---------------------------------------------------------------------------------------------
_CURVE_FLAGS = ("a score is NaN", "a label is neither 0 nor 1", "a segment id is out of range")


class CurveStats:
    """What :func:`curve_areas` returns, all on the device, one entry per segment (one entry without segments):
    int64 ``P``, ``N`` (positives, negatives), ``tp``, ``fp`` (those with ``score >= threshold``), ``groups`` (distinct
    scores), ``u2`` (twice the Mann-Whitney count), float64 ``auroc``, ``aupr`` and the int32 flag word ``info``
    (bit 0 NaN score, bit 1 label not 0 / 1, bit 2 segment id out of range).  Nothing here reads a value back."""

    def __init__(self, count: torch.Tensor, area: torch.Tensor, info: torch.Tensor):
        self.count, self.area, self.info = count, area, info
        self.P, self.N, self.tp, self.fp, self.groups, self.u2 = count.unbind(1)
        self.auroc, self.aupr = area.unbind(1)

    def accuracy(self) -> torch.Tensor:
        """``(TP + TN) / (P + N)`` at the threshold (evaluation.py:68), float64 per segment; NaN for an empty one."""
        return (self.tp + (self.N - self.fp)).double() / (self.P + self.N).double()

    def f1(self) -> torch.Tensor:
        """``2 TP / (2 TP + FP + FN)`` at the threshold (evaluation.py:70), float64 per segment; NaN where that is 0 / 0."""
        return (2 * self.tp).double() / (self.tp + self.fp + self.P).double()

    def macro(self) -> Tuple[torch.Tensor, torch.Tensor]:
        """``nanmean`` of ``auroc`` and of ``aupr`` over the segments: two float64 scalars on the device."""
        return torch.nanmean(self.auroc), torch.nanmean(self.aupr)


def curve_areas(score: torch.Tensor, label: torch.Tensor, segment: Optional[torch.Tensor] = None, n_segments: int = 0,
                threshold: float = 0.0, check: bool = True) -> CurveStats:
    """Exact trapezoid AUROC and AUPR of ``score`` (fp32, any shape) against ``label`` (fp32, bool or integer; positive
    iff != 0), computed on the device by a sort and a scan (``dgmi_curve_areas_f32``, definition in
    ``include/dgmi_curve.h``): what ``harness.auroc_aupr`` computes on the host, with ties between scores handled as one
    threshold.  With ``segment`` (int32 / int64 ids in ``[0, n_segments)``) every segment gets its own statistics, e.g.
    per disease.  ``threshold`` is the logit cut of ``tp`` / ``fp`` (0 is probability 0.5).

    ``check=True`` reads the flag word, which synchronises once, and raises ``RuntimeError`` naming a set flag.
    ``check=False`` reads nothing back: the form to queue between replays of a captured training step; the flags stay
    in ``CurveStats.info``.  Not differentiable."""
    _require_device(score, label, segment)
    n_segments = int(n_segments)
    if (segment is None) != (n_segments == 0):
        raise ValueError("segment ids and n_segments > 0 go together")
    stats = CurveStats(*_T.curve_areas(score.detach(), label, segment, n_segments, float(threshold)))
    if check:
        flags = int(stats.info[0])
        if flags:
            raise RuntimeError("curve_areas: " + "; ".join(m for b, m in enumerate(_CURVE_FLAGS) if flags >> b & 1))
    return stats

# ---------------------------------------------------------------------------------------------
# (D3) edge-dropout selection — augmentation.py:48-52, 114-118
# ---------------------------------------------------------------------------------------------
def random_subset_select(E: int, keep: int, seed: int, device, e_offset: int = 0) -> torch.Tensor:
    """The 8-word description (int32 tensor on ``device``) of a uniformly random subset of exactly
    ``keep`` of ``E`` edges, a deterministic function of ``(seed, E, keep)``
    (``dgmi_random_subset_select``): what ``CSRGraph.dropped`` and the kernels consume.  Nothing of
    size E is written and nothing synchronises."""
    device = torch.device(device)
    if device.type != "cuda":
        raise RuntimeError("dream_gnn_amd ops run on the MI355X only: got device %s" % device)
    return _T.random_subset_select(torch.empty(0, device=device), E, keep, _signed64(seed), e_offset)


def _signed64(seed: int) -> int:
    seed &= 0xFFFFFFFFFFFFFFFF
    return seed - (1 << 64) if seed >= 1 << 63 else seed


def random_subset_select_batch(Es, keeps, seeds, device, e_offsets=None) -> torch.Tensor:
    """``random_subset_select`` for several edge lists at once: ``(n, 8)`` descriptions from ONE series
    of launches per 8 lists (``dgmi_random_subset_select_batch``) — the training step drops edges on
    4 relations and 4 similarity graphs together (train.py:267), and at dataset scale the launches
    are the cost of the selection."""
    device = torch.device(device)
    if device.type != "cuda":
        raise RuntimeError("dream_gnn_amd ops run on the MI355X only: got device %s" % device)
    n = len(Es)
    offs = [0] * n if e_offsets is None else list(e_offsets)
    if isinstance(seeds, torch.Tensor):
        # seeds in device memory (int64, one per list), read by the kernels (``dgmi_random_subset_select_batch_dseed``):
        # no host value goes into the launches, so the call can sit inside a captured HIP graph and still select new
        # subsets on every replay
        _require_device(seeds)
        seeds = seeds.reshape(-1).to(torch.int64).contiguous()
        parts = [_T.random_subset_select_batch_dseed(seeds[i:i + 8], list(Es[i:i + 8]), list(keeps[i:i + 8]), offs[i:i + 8])
                 for i in range(0, n, 8)]
        return parts[0] if len(parts) == 1 else torch.cat(parts)
    like = torch.empty(0, device=device)
    parts = [_T.random_subset_select_batch(like, list(Es[i:i + 8]), list(keeps[i:i + 8]),
                                           [_signed64(s) for s in seeds[i:i + 8]], offs[i:i + 8])
             for i in range(0, n, 8)]
    return parts[0] if len(parts) == 1 else torch.cat(parts)


def keep_mask(desc: torch.Tensor, E: int) -> torch.Tensor:
    """float 0/1 mask over edges [0, E) under the subset description(s) ``desc`` (``dgmi_keep_mask_f32``)."""
    _require_device(desc)
    return _T.keep_mask(_prep_keep(desc), E)


def random_subset_mask(E: int, keep: int, seed: int, device) -> torch.Tensor:
    """float 0/1 mask over E edges with exactly ``keep`` ones, a uniformly random subset that is a
    deterministic function of ``(seed, E, keep)`` (``dgmi_random_subset_mask_f32``)."""
    device = torch.device(device)
    if device.type != "cuda":
        raise RuntimeError("dream_gnn_amd ops run on the MI355X only: got device %s" % device)
    mask = torch.empty(E, dtype=torch.float32, device=device)
    nbytes = int(_L.dgmi_random_subset_workspace_bytes())
    ws = torch.empty(nbytes, dtype=torch.uint8, device=device)
    with _guard(device):
        _lib.check(_L.dgmi_random_subset_mask_f32(E, keep, seed & 0xFFFFFFFFFFFFFFFF, _ptr(mask), _ptr(ws), nbytes,
                                                  _stream(device)), "dgmi_random_subset_mask_f32")
    return mask
