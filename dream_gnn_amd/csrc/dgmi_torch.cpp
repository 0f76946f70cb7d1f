// dgmi_torch.cpp — the torch operator layer of SURVEY.md §8(b): `dreamgnn_mi::*` dispatcher ops over
// the C ABI of libdgmi.so (include/dgmi.h).  Built for ROCm only (ROCm torch's HIP stream / device guard —
// its tensors carry the device type "cuda", hence the *MasqueradingAsCUDA names; there is no CUDA branch
// and no CPU kernel: the product path has no fallback).
//
// What they replace inside the dispatcher:
//   dreamgnn_mi::spmm_csr      graph.update_all(fn.copy_u('h','m'), fn.sum('m','h'))  (reference layers.py:229-232,
//                              with the cj / ci scalings of :224-225,234 fused) and th.spmm(adj, support)
//                              (layers.py:312); autograd registered: dX = diag(ss) A^T diag(ds) dY through the
//                              same kernels on the transposed CSR.
//   dreamgnn_mi::csr_from_coo  DGL's COO->CSR behind dgl.heterograph (data_loader.py:448, augmentation.py:65)
//   the *_raw ops              one C-ABI entry point each, no autograd: what dream_gnn_amd/ops.py (layout caches,
//                              kernel choice, graph-level autograd) is written in.
// Every op validates dtype / device / contiguity with TORCH_CHECK (-> RuntimeError), makes the inputs'
// device current, takes torch's current HIP stream, allocates outputs from the caching allocator and
// kernel scratch from a per-(device, stream) cache, and never synchronises.
#include <ATen/ATen.h>
#include <ATen/hip/impl/HIPGuardImplMasqueradingAsCUDA.h>
#include <ATen/hip/impl/HIPStreamMasqueradingAsCUDA.h>
#include <torch/autograd.h>
#include <torch/library.h>

#include <mutex>
#include <tuple>
#include <unordered_map>

#include "dgmi.h"
#include "dgmi_above.h"
#include "dgmi_attn.h"
#include "dgmi_bf16.h"
#include "dgmi_curve.h"
#include "dgmi_given.h"
#include "dgmi_pairs.h"
#include "dgmi_rank.h"
#include "dgmi_train.h"

namespace {

using at::Tensor;
using OptTensor = c10::optional<Tensor>;

void check_status(int rc, const char* what) {
  TORCH_CHECK(rc == DGMI_OK, what, " failed: ", dgmi_status_string(rc), " (status ", rc, ")");
}

void check_dev(const Tensor& t, const char* name) {
  TORCH_CHECK(t.is_cuda(), "dream_gnn_amd ops run on the MI355X only: ", name, " is a ", t.device().str(),
              " tensor. There is no CPU path (the CPU restatement under oracle/ is test infrastructure).");
}

void check(const Tensor& t, at::ScalarType dt, int64_t dim, const char* name, const Tensor& like) {
  check_dev(t, name);
  TORCH_CHECK(t.scalar_type() == dt, name, " must be ", c10::toString(dt), ", got ", c10::toString(t.scalar_type()));
  TORCH_CHECK(t.dim() == dim, name, " must be ", dim, "-D, got ", t.dim(), "-D");
  TORCH_CHECK(t.is_contiguous(), name, " must be contiguous");
  TORCH_CHECK(t.device() == like.device(), "tensors on different devices: ", name, " on ", t.device().str(), " vs ",
              like.device().str());
}

const void* optptr(const OptTensor& t) { return t.has_value() && t->defined() ? t->data_ptr() : nullptr; }

void check_opt(const OptTensor& t, at::ScalarType dt, int64_t n, const char* name, const Tensor& like) {
  if (!t.has_value() || !t->defined()) return;
  check(*t, dt, 1, name, like);
  TORCH_CHECK(n < 0 || t->numel() == n, name, " has ", t->numel(), " entries, expected ", n);
}

dgmi_stream_t stream_of(const Tensor& t) { return c10::hip::getCurrentHIPStreamMasqueradingAsCUDA(t.device().index()).stream(); }

// Kernel scratch (chunk partials, partial planes, builder workspaces): one buffer per (device, stream,
// kind), grown on demand.  Products issued on one stream are ordered, so they can share it; nothing is
// allocated per call and contents are never read across calls.
Tensor scratch(const Tensor& like, size_t nbytes, int kind) {
  static std::mutex mu;
  static std::unordered_map<uint64_t, Tensor> cache;
  const auto s = c10::hip::getCurrentHIPStreamMasqueradingAsCUDA(like.device().index());
  const uint64_t key = (reinterpret_cast<uint64_t>(s.stream()) * 31u + (uint64_t)like.device().index()) * 8u + (uint64_t)kind;
  std::lock_guard<std::mutex> lock(mu);
  auto it = cache.find(key);
  if (it == cache.end() || (size_t)it->second.numel() < nbytes) {
    Tensor buf = at::empty({(int64_t)(nbytes < 16 ? 16 : nbytes)}, like.options().dtype(at::kByte));
    cache[key] = buf;
    return buf;
  }
  return it->second;
}
enum { kPartials = 0, kPlanes = 1, kBuilder = 2, kPairs = 3, kTrain = 4, kAttn = 5 };

struct Keep {
  const int32_t* eid = nullptr;
  const uint32_t* table = nullptr;
  int32_t n = 0;
};

// `for_product`: the descriptions go to a product launch.  A layout without edges has nothing to drop, and its empty eid
// tensor has no storage — a null pointer, which the C ABI refuses beside a description: such a product runs un-dropped (a
// row shard that owns no edge, dropped by the step's description like every other).
Keep keep_of(const OptTensor& eid, const OptTensor& keep, int64_t nnz, const Tensor& like, bool for_product = true) {
  Keep k;
  if (!keep.has_value() || !keep->defined()) return k;
  TORCH_CHECK(keep->scalar_type() == at::kInt && keep->is_contiguous() && keep->dim() == 2 && keep->size(1) == 8,
              "keep must be a contiguous (n, 8) int32 tensor of subset descriptions");
  TORCH_CHECK(keep->size(0) <= 8, "at most 8 subset descriptions per product");
  TORCH_CHECK(eid.has_value() && eid->defined(), "edge dropout on the fly needs the layout's eid array");
  check(*eid, at::kInt, 1, "eid", like);
  check_dev(*keep, "keep");
  TORCH_CHECK(eid->numel() == nnz, "eid has ", eid->numel(), " entries, the layout has ", nnz, " edges");
  if (for_product && nnz == 0) return k;
  k.eid = eid->data_ptr<int32_t>();
  k.table = reinterpret_cast<const uint32_t*>(keep->data_ptr<int32_t>());
  k.n = (int32_t)keep->size(0);
  return k;
}

// output epilogue: Y = out_mask * mask_scale * act(dst_scale * sum); act 0 none, 1 leaky-relu(slope)
struct Epi {
  int32_t act = 0;
  float slope = 0.f;
  const float* mask = nullptr;
  int64_t ldm = 0;
  float mscale = 1.f;
};

Epi epi_of(int64_t act, double slope, const OptTensor& out_mask, double mask_scale, int64_t rows, int64_t F, const Tensor& like) {
  Epi e;
  TORCH_CHECK(act == 0 || act == 1, "act must be 0 (none) or 1 (leaky-relu)");
  e.act = (int32_t)act;
  e.slope = (float)slope;
  e.mscale = (float)mask_scale;
  if (out_mask.has_value() && out_mask->defined()) {
    check_dev(*out_mask, "out_mask");
    TORCH_CHECK(out_mask->scalar_type() == at::kFloat && out_mask->dim() == 2 && out_mask->size(0) == rows &&
                    out_mask->size(1) == F && out_mask->stride(1) == 1 && out_mask->device() == like.device(),
                "out_mask must be a float32 (", rows, ", ", F, ") tensor with contiguous rows on ", like.device().str());
    e.mask = out_mask->data_ptr<float>();
    e.ldm = rows > 1 ? out_mask->stride(0) : (F > 0 ? F : 1);
  }
  return e;
}

struct Dense {
  Tensor t;
  int64_t rows, F, ld;
};

// a 2-D fp32 matrix whose rows are contiguous (a row-strided view is consumed in place)
Dense dense_of(const Tensor& X, const char* name) {
  check_dev(X, name);
  TORCH_CHECK(X.scalar_type() == at::kFloat && X.dim() == 2, name, " must be a 2-D float32 tensor");
  Tensor t = X;
  if (X.stride(1) != 1 || (X.size(0) > 1 && X.stride(0) < X.size(1))) t = X.contiguous();
  const int64_t F = t.size(1);
  return {t, t.size(0), F, t.size(0) > 1 ? t.stride(0) : (F > 0 ? F : 1)};
}

inline bool rows_16b_aligned(const Tensor& t, int64_t ld) {
  return (reinterpret_cast<uintptr_t>(t.data_ptr()) & 15) == 0 && ld % 4 == 0;
}

// dense_of for the kernels that read rows as float4 (the pair rankings): a view whose rows do not start on 16-B
// boundaries (X[:, 1:129] of a wider tensor, an odd leading dimension) is copied, as a column-strided one is
Dense dense16_of(const Tensor& X, const char* name) {
  Dense d = dense_of(X, name);
  if (!rows_16b_aligned(d.t, d.ld)) {
    d.t = d.t.clone(at::MemoryFormat::Contiguous);
    d.ld = d.F > 0 ? d.F : 1;
  }
  return d;
}

// a contiguous copy-or-alias of a parameter that starts on a 16-B boundary
Tensor contiguous16(const Tensor& t) {
  Tensor c = t.contiguous();
  return (reinterpret_cast<uintptr_t>(c.data_ptr()) & 15) == 0 ? c : c.clone(at::MemoryFormat::Contiguous);
}

Tensor out_of(const OptTensor& out, int64_t rows, int64_t F, const Tensor& like) {
  if (out.has_value() && out->defined()) {
    TORCH_CHECK(out->scalar_type() == at::kFloat && out->dim() == 2 && out->size(0) == rows && out->size(1) == F &&
                    out->is_contiguous() && out->device() == like.device(),
                "out must be a contiguous float32 (", rows, ", ", F, ") tensor on ", like.device().str());
    return *out;
  }
  return at::empty({rows, F}, like.options().dtype(at::kFloat));
}

// ---------------------------------------------------------------------------------------------
std::tuple<Tensor, Tensor, Tensor, Tensor> csr_from_coo(const Tensor& row, const Tensor& col, int64_t n_rows, int64_t n_cols) {
  check(row, at::kInt, 1, "row", row);
  check(col, at::kInt, 1, "col", row);
  TORCH_CHECK(row.numel() == col.numel(), "row/col length mismatch");
  TORCH_CHECK(n_rows >= 0, "n_rows must be >= 0");
  c10::hip::HIPGuardMasqueradingAsCUDA guard(row.device());
  const int64_t E = row.numel();
  Tensor indptr = at::empty({n_rows + 1}, row.options()), indices = at::empty({E}, row.options()),
         eid = at::empty({E}, row.options());
  size_t need = 0;
  check_status(dgmi_csr_from_coo_i32(row.data_ptr<int32_t>(), col.data_ptr<int32_t>(), E, n_rows, n_cols, nullptr, nullptr,
                                     nullptr, nullptr, &need, nullptr), "dgmi_csr_from_coo_i32(size query)");
  Tensor ws = scratch(row, need < 256 ? 256 : need, kBuilder);
  size_t have = (size_t)ws.numel();
  check_status(dgmi_csr_from_coo_i32(row.data_ptr<int32_t>(), col.data_ptr<int32_t>(), E, n_rows, n_cols,
                                     indptr.data_ptr<int32_t>(), indices.data_ptr<int32_t>(), eid.data_ptr<int32_t>(),
                                     ws.data_ptr(), &have, stream_of(row)), "dgmi_csr_from_coo_i32");
  // the range flag leaves the shared workspace before the next builder call overwrites it
  Tensor flag = ws.narrow(0, 0, 4).view(at::kInt).clone();
  return {indptr, indices, eid, flag};
}

std::tuple<Tensor, Tensor, Tensor, Tensor> csr_sliced_from_coo(const Tensor& row, const Tensor& col, int64_t n_rows,
                                                               int64_t n_cols, int64_t n_slices) {
  check(row, at::kInt, 1, "row", row);
  check(col, at::kInt, 1, "col", row);
  TORCH_CHECK(row.numel() == col.numel(), "row/col length mismatch");
  c10::hip::HIPGuardMasqueradingAsCUDA guard(row.device());
  const int64_t E = row.numel();
  Tensor segptr = at::empty({n_slices * n_rows + 1}, row.options()), indices = at::empty({E}, row.options()),
         eid = at::empty({E}, row.options());
  size_t need = 0;
  check_status(dgmi_csr_sliced_from_coo_i32(row.data_ptr<int32_t>(), col.data_ptr<int32_t>(), E, n_rows, n_cols,
                                            (int32_t)n_slices, nullptr, nullptr, nullptr, nullptr, &need, nullptr),
               "dgmi_csr_sliced_from_coo_i32(size query)");
  Tensor ws = scratch(row, need < 256 ? 256 : need, kBuilder);
  size_t have = (size_t)ws.numel();
  check_status(dgmi_csr_sliced_from_coo_i32(row.data_ptr<int32_t>(), col.data_ptr<int32_t>(), E, n_rows, n_cols,
                                            (int32_t)n_slices, segptr.data_ptr<int32_t>(), indices.data_ptr<int32_t>(),
                                            eid.data_ptr<int32_t>(), ws.data_ptr(), &have, stream_of(row)),
               "dgmi_csr_sliced_from_coo_i32");
  Tensor flag = ws.narrow(0, 0, 4).view(at::kInt).clone();
  return {segptr, indices, eid, flag};
}

std::tuple<Tensor, Tensor, Tensor, Tensor> csr_sliced_from_csr(const Tensor& indptr, const Tensor& indices, const Tensor& eid,
                                                               int64_t n_cols, int64_t n_slices) {
  check(indptr, at::kInt, 1, "indptr", indptr);
  check(indices, at::kInt, 1, "indices", indptr);
  check(eid, at::kInt, 1, "eid", indptr);
  TORCH_CHECK(indices.numel() == eid.numel(), "indices/eid length mismatch");
  TORCH_CHECK(indptr.numel() >= 1, "indptr is empty");
  c10::hip::HIPGuardMasqueradingAsCUDA guard(indptr.device());
  const int64_t E = indices.numel(), n_rows = indptr.numel() - 1;
  size_t need = 0;  // the size query first: a shape the ABI refuses is reported before anything is allocated for it
  check_status(dgmi_csr_sliced_from_csr_i32(nullptr, nullptr, nullptr, E, n_rows, n_cols, (int32_t)n_slices, nullptr, nullptr,
                                            nullptr, nullptr, &need, nullptr),
               "dgmi_csr_sliced_from_csr_i32(size query)");
  Tensor segptr = at::empty({n_slices * n_rows + 1}, indptr.options()), s_indices = at::empty({E}, indptr.options()),
         s_eid = at::empty({E}, indptr.options());
  Tensor ws = scratch(indptr, need < 256 ? 256 : need, kBuilder);
  size_t have = (size_t)ws.numel();
  check_status(dgmi_csr_sliced_from_csr_i32(indptr.data_ptr<int32_t>(), indices.data_ptr<int32_t>(), eid.data_ptr<int32_t>(), E,
                                            n_rows, n_cols, (int32_t)n_slices, segptr.data_ptr<int32_t>(),
                                            s_indices.data_ptr<int32_t>(), s_eid.data_ptr<int32_t>(), ws.data_ptr(), &have,
                                            stream_of(indptr)),
               "dgmi_csr_sliced_from_csr_i32");
  Tensor flag = ws.narrow(0, 0, 4).view(at::kInt).clone();
  return {segptr, s_indices, s_eid, flag};
}

Tensor plan_build(const Tensor& indptr, int64_t nnz, int64_t chunk) {
  check(indptr, at::kInt, 1, "indptr", indptr);
  c10::hip::HIPGuardMasqueradingAsCUDA guard(indptr.device());
  const int64_t n_rows = indptr.numel() - 1;
  const size_t nbytes = dgmi_spmm_plan_bytes(n_rows, nnz, (int32_t)chunk);
  TORCH_CHECK(nbytes > 0, "invalid plan parameters (chunk=", chunk, ")");
  Tensor plan = at::empty({(int64_t)nbytes}, indptr.options().dtype(at::kByte));
  size_t need = 0;
  check_status(dgmi_spmm_plan_build(indptr.data_ptr<int32_t>(), n_rows, nnz, (int32_t)chunk, nullptr, 0, nullptr, &need, nullptr),
               "dgmi_spmm_plan_build(size query)");
  Tensor ws = scratch(indptr, need < 256 ? 256 : need, kBuilder);
  size_t have = (size_t)ws.numel();
  check_status(dgmi_spmm_plan_build(indptr.data_ptr<int32_t>(), n_rows, nnz, (int32_t)chunk, plan.data_ptr(), nbytes,
                                    ws.data_ptr(), &have, stream_of(indptr)), "dgmi_spmm_plan_build");
  return plan;
}

// plan undefined: dgmi_spmm_csr_f32 (a wave per row); else dgmi_spmm_csr_planned_f32
Tensor spmm_csr_raw(const Tensor& indptr, const Tensor& indices, const OptTensor& vals, const OptTensor& eid,
                    const OptTensor& keep, const Tensor& X, const OptTensor& src_scale, const OptTensor& dst_scale,
                    const OptTensor& plan, int64_t chunk, const OptTensor& out, int64_t act = 0, double slope = 0.0,
                    const OptTensor& out_mask = c10::nullopt, double mask_scale = 1.0) {
  check(indptr, at::kInt, 1, "indptr", indptr);
  check(indices, at::kInt, 1, "indices", indptr);
  Dense x = dense_of(X, "X");
  TORCH_CHECK(x.t.device() == indptr.device(), "X and the graph are on different devices");
  const int64_t n_dst = indptr.numel() - 1, nnz = indices.numel();
  check_opt(vals, at::kFloat, nnz, "vals", indptr);
  check_opt(src_scale, at::kFloat, x.rows, "src_scale", indptr);
  check_opt(dst_scale, at::kFloat, n_dst, "dst_scale", indptr);
  const Keep k = keep_of(eid, keep, nnz, indptr);
  c10::hip::HIPGuardMasqueradingAsCUDA guard(indptr.device());
  Tensor y = out_of(out, n_dst, x.F, indptr);
  const int64_t ldy = x.F > 0 ? x.F : 1;
  const Epi e = epi_of(act, slope, out_mask, mask_scale, n_dst, x.F, indptr);
  if (!plan.has_value() || !plan->defined()) {
    check_status(dgmi_spmm_csr_f32(indptr.data_ptr<int32_t>(), indices.data_ptr<int32_t>(), (const float*)optptr(vals), k.eid,
                                   k.table, k.n, x.t.data_ptr<float>(), x.ld, (const float*)optptr(src_scale),
                                   (const float*)optptr(dst_scale), y.data_ptr<float>(), ldy, n_dst, x.rows, x.F, e.act,
                                   e.slope, e.mask, e.ldm, e.mscale, stream_of(indptr)), "dgmi_spmm_csr_f32");
    return y;
  }
  const size_t pbytes = dgmi_spmm_partials_bytes(nnz, (int32_t)chunk, x.F);
  Tensor partials = scratch(indptr, pbytes, kPartials);
  check_status(dgmi_spmm_csr_planned_f32(indptr.data_ptr<int32_t>(), indices.data_ptr<int32_t>(), (const float*)optptr(vals),
                                         k.eid, k.table, k.n, x.t.data_ptr<float>(), x.ld, (const float*)optptr(src_scale),
                                         (const float*)optptr(dst_scale), y.data_ptr<float>(), ldy, n_dst, x.rows, x.F, nnz,
                                         (int32_t)chunk, plan->data_ptr(), partials.data_ptr(), pbytes, e.act, e.slope, e.mask,
                                         e.ldm, e.mscale, stream_of(indptr)),
               "dgmi_spmm_csr_planned_f32");
  return y;
}

Tensor spmm_sliced_raw(const Tensor& segptr, const Tensor& indices, const OptTensor& vals, const OptTensor& eid,
                       const OptTensor& keep, const Tensor& X, const OptTensor& src_scale, const OptTensor& dst_scale,
                       int64_t n_dst, int64_t n_slices, const OptTensor& out, int64_t act = 0, double slope = 0.0,
                       const OptTensor& out_mask = c10::nullopt, double mask_scale = 1.0, int64_t column_passes = 0,
                       int64_t id_mult = 0) {
  check(segptr, at::kInt, 1, "segptr", segptr);
  check(indices, at::kInt, 1, "indices", segptr);
  TORCH_CHECK(segptr.numel() == n_slices * n_dst + 1, "segptr has ", segptr.numel(), " entries, expected n_slices * n_dst + 1");
  Dense x = dense_of(X, "X");
  TORCH_CHECK(x.t.device() == segptr.device(), "X and the graph are on different devices");
  const int64_t nnz = indices.numel();
  check_opt(vals, at::kFloat, nnz, "vals", segptr);
  check_opt(src_scale, at::kFloat, x.rows, "src_scale", segptr);
  check_opt(dst_scale, at::kFloat, n_dst, "dst_scale", segptr);
  const Keep k = keep_of(eid, keep, nnz, segptr);
  c10::hip::HIPGuardMasqueradingAsCUDA guard(segptr.device());
  Tensor y = out_of(out, n_dst, x.F, segptr);
  const Epi e = epi_of(act, slope, out_mask, mask_scale, n_dst, x.F, segptr);
  const size_t pbytes = dgmi_spmm_sliced_planes_bytes(n_dst, (int32_t)n_slices, x.F);
  Tensor planes = scratch(segptr, pbytes, kPlanes);
  check_status(dgmi_spmm_sliced_f32(segptr.data_ptr<int32_t>(), indices.data_ptr<int32_t>(), (const float*)optptr(vals), k.eid,
                                    k.table, k.n, x.t.data_ptr<float>(), x.ld, (const float*)optptr(src_scale),
                                    (const float*)optptr(dst_scale), y.data_ptr<float>(), x.F, n_dst, x.rows, x.F,
                                    (int32_t)n_slices, (int32_t)column_passes, (int32_t)id_mult, planes.data_ptr(), pbytes, e.act,
                                    e.slope, e.mask,
                                    e.ldm, e.mscale, stream_of(segptr)), "dgmi_spmm_sliced_f32");
  return y;
}

Tensor gather_f32(const Tensor& values, const Tensor& perm) {
  check(values, at::kFloat, 1, "values", values);
  check(perm, at::kInt, 1, "perm", values);
  c10::hip::HIPGuardMasqueradingAsCUDA guard(values.device());
  Tensor out = at::empty({perm.numel()}, values.options());
  check_status(dgmi_gather_f32(values.data_ptr<float>(), perm.data_ptr<int32_t>(), perm.numel(), out.data_ptr<float>(),
                               stream_of(values)), "dgmi_gather_f32");
  return out;
}

Tensor gather_concat_raw(const Tensor& src, const Tensor& dst, const Tensor& A, const Tensor& B) {
  check(src, at::kInt, 1, "src", src);
  check(dst, at::kInt, 1, "dst", src);
  TORCH_CHECK(src.numel() == dst.numel(), "src/dst length mismatch");
  Dense a = dense_of(A, "A"), b = dense_of(B, "B");
  TORCH_CHECK(a.t.device() == src.device() && b.t.device() == src.device(), "tensors on different devices");
  c10::hip::HIPGuardMasqueradingAsCUDA guard(src.device());
  const int64_t E = src.numel(), W = a.F + b.F;
  Tensor out = at::empty({E, W}, a.t.options());
  check_status(dgmi_gather_concat_f32(src.data_ptr<int32_t>(), dst.data_ptr<int32_t>(), E, a.t.data_ptr<float>(), a.ld, a.F,
                                      b.t.data_ptr<float>(), b.ld, b.F, out.data_ptr<float>(), W > 0 ? W : 1, stream_of(src)),
               "dgmi_gather_concat_f32");
  return out;
}

Tensor gather_add_raw(const Tensor& src, const Tensor& dst, const Tensor& A, const Tensor& B, const OptTensor& bias, int64_t act) {
  TORCH_CHECK(act == 0 || act == 1, "act must be 0 (none) or 1 (relu)");
  check(src, at::kInt, 1, "src", src);
  check(dst, at::kInt, 1, "dst", src);
  TORCH_CHECK(src.numel() == dst.numel(), "src/dst length mismatch");
  Dense a = dense_of(A, "A"), b = dense_of(B, "B");
  TORCH_CHECK(a.F == b.F, "A and B must have the same width, got ", a.F, " and ", b.F);
  TORCH_CHECK(a.t.device() == src.device() && b.t.device() == src.device(), "tensors on different devices");
  check_opt(bias, at::kFloat, a.F, "bias", src);
  c10::hip::HIPGuardMasqueradingAsCUDA guard(src.device());
  const int64_t E = src.numel();
  Tensor out = at::empty({E, a.F}, a.t.options());
  check_status(dgmi_gather_add_f32(src.data_ptr<int32_t>(), dst.data_ptr<int32_t>(), E, a.t.data_ptr<float>(), a.ld,
                                   b.t.data_ptr<float>(), b.ld, (const float*)optptr(bias), a.F, out.data_ptr<float>(),
                                   a.F > 0 ? a.F : 1, (int32_t)act, stream_of(src)), "dgmi_gather_add_f32");
  return out;
}

Tensor epilogue_backward(const Tensor& dY, const Tensor& Y, const OptTensor& mask, int64_t act, double slope, double mask_scale) {
  check_dev(dY, "dY");
  TORCH_CHECK(dY.scalar_type() == at::kFloat && dY.is_contiguous(), "dY must be contiguous float32");
  TORCH_CHECK(Y.scalar_type() == at::kFloat && Y.is_contiguous() && Y.numel() == dY.numel() && Y.device() == dY.device(),
              "Y must be contiguous float32 of dY's size, on its device");
  if (mask.has_value() && mask->defined())
    TORCH_CHECK(mask->scalar_type() == at::kFloat && mask->is_contiguous() && mask->numel() == dY.numel() &&
                    mask->device() == dY.device(), "mask must be contiguous float32 of dY's size, on its device");
  c10::hip::HIPGuardMasqueradingAsCUDA guard(dY.device());
  Tensor out = at::empty_like(dY);
  check_status(dgmi_epilogue_backward_f32(dY.data_ptr<float>(), Y.data_ptr<float>(), (const float*)optptr(mask), dY.numel(),
                                          (int32_t)act, (float)slope, (float)mask_scale, out.data_ptr<float>(), stream_of(dY)),
               "dgmi_epilogue_backward_f32");
  return out;
}

// diag(scale) X in one streaming pass (ahead of an XCD-local product, see include/dgmi.h)
Tensor scale_rows(const Tensor& X, const Tensor& scale) {
  Dense x = dense_of(X, "X");
  check(scale, at::kFloat, 1, "scale", x.t);
  TORCH_CHECK(scale.numel() == x.rows, "scale has ", scale.numel(), " entries, X has ", x.rows, " rows");
  c10::hip::HIPGuardMasqueradingAsCUDA guard(x.t.device());
  Tensor out = at::empty({x.rows, x.F}, x.t.options());
  check_status(dgmi_scale_rows_f32(x.t.data_ptr<float>(), x.ld, scale.data_ptr<float>(), x.rows, x.F, out.data_ptr<float>(), x.F,
                                   stream_of(x.t)), "dgmi_scale_rows_f32");
  return out;
}

// (f3 complement form) rows [n*R, n*R + B) of `feat_ext` <- coef @ feat_ext[u*R + i0, :] (column sums per block), in place
void colsum_rows_(Tensor feat_ext, const Tensor& coef, int64_t n, int64_t R, int64_t i0) {
  check(feat_ext, at::kFloat, 2, "feat_ext", feat_ext);
  check(coef, at::kFloat, 2, "coef", feat_ext);
  const int64_t B = coef.size(0), W = feat_ext.size(1);
  TORCH_CHECK(coef.size(1) == n && feat_ext.size(0) == n * R + B && i0 >= 0 && i0 < R && B <= 64,
              "colsum_rows_: feat_ext must have n*R + B rows, coef (B, n)");
  c10::hip::HIPGuardMasqueradingAsCUDA guard(feat_ext.device());
  if (n == 0) {  // sums over no row: coef is (B, 0), an empty tensor whose null pointer the C ABI refuses
    feat_ext.zero_();
    return;
  }
  float* base = feat_ext.data_ptr<float>();
  check_status(dgmi_weighted_colsum_f32(base + i0 * W, R * W, coef.data_ptr<float>(), n, n, W, (int32_t)B, base + n * R * W, W,
                                        stream_of(feat_ext)), "dgmi_weighted_colsum_f32");
}

// its backward: gf[u*R + i0, :] += coef[:, u]^T @ gs, in place on the (n*R, W) gradient of the transform
void colsum_rows_backward_(Tensor gf, const Tensor& coef, const Tensor& gs, int64_t n, int64_t R, int64_t i0) {
  check(gf, at::kFloat, 2, "gf", gf);
  check(coef, at::kFloat, 2, "coef", gf);
  check(gs, at::kFloat, 2, "gs", gf);
  const int64_t B = coef.size(0), W = gf.size(1);
  TORCH_CHECK(coef.size(1) == n && gf.size(0) == n * R && gs.size(0) == B && gs.size(1) == W && i0 >= 0 && i0 < R && B <= 64,
              "colsum_rows_backward_: shape mismatch");
  c10::hip::HIPGuardMasqueradingAsCUDA guard(gf.device());
  check_status(dgmi_rank_add_f32(gf.data_ptr<float>() + i0 * W, R * W, coef.data_ptr<float>(), n, gs.data_ptr<float>(), W, n, W,
                                 (int32_t)B, stream_of(gf)), "dgmi_rank_add_f32");
}

// (f4) (N, k) int32 neighbours of the k largest cosine similarities per row of a row-normalised matrix
Tensor knn_cosine_topk(const Tensor& Xn, int64_t k) {
  Dense x = dense_of(Xn, "Xn");
  TORCH_CHECK(x.ld % 4 == 0 && (reinterpret_cast<uintptr_t>(x.t.data_ptr()) & 15) == 0, "Xn rows must be 16-B aligned");
  TORCH_CHECK(dgmi_knn_cosine_supported(x.rows, x.F, k) == 1, "shape not supported by the fused kNN kernel: N=", x.rows,
              " D=", x.F, " k=", k);
  c10::hip::HIPGuardMasqueradingAsCUDA guard(x.t.device());
  Tensor nbr = at::empty({x.rows, k}, x.t.options().dtype(at::kInt));
  const size_t wbytes = dgmi_knn_cosine_workspace_bytes(x.rows, x.F, (int32_t)k);
  // per call, from the caching allocator (reused on the same stream, returned by empty_cache()): the screened search
  // needs 2-6 GB at N = 100 000, which a one-off graph construction must not pin for the life of the process
  Tensor ws = at::empty({(int64_t)(wbytes < 16 ? 16 : wbytes)}, x.t.options().dtype(at::kByte));
  check_status(dgmi_knn_cosine_topk_f32(x.t.data_ptr<float>(), x.ld, x.rows, x.F, (int32_t)k, nbr.data_ptr<int32_t>(),
                                        ws.data_ptr(), (size_t)ws.numel(), stream_of(x.t)), "dgmi_knn_cosine_topk_f32");
  return nbr;
}

// the k best novel drug-disease pairs under the decoder MLP (dgmi_pairs.hip): (drug, disease, logit) of k slots each, and
// info = [number returned, out-of-range flag].  int64 known ids are clamped into [-1, INT32_MAX] on the device, so an id
// beyond int32 still reads as out of range; nothing here synchronises.
std::tuple<Tensor, Tensor, Tensor, Tensor> pair_mlp_topk(const Tensor& P, const Tensor& Q, const Tensor& W2, const Tensor& b2,
                                                         const Tensor& w3, const Tensor& b3, const OptTensor& known_drug,
                                                         const OptTensor& known_dis, int64_t k) {
  Dense p = dense16_of(P, "P"), q = dense16_of(Q, "Q");
  TORCH_CHECK(p.F == 128 && q.F == 128, "P and Q must have 128 columns (the decoder's lin1 width), got ", p.F, " and ", q.F);
  check(W2, at::kFloat, 2, "W2", P);
  TORCH_CHECK(W2.size(0) == 64 && W2.size(1) == 128, "W2 must be (64, 128), got (", W2.size(0), ", ", W2.size(1), ")");
  check(b2, at::kFloat, 1, "b2", P);
  check(w3, at::kFloat, 1, "w3", P);
  check(b3, at::kFloat, 1, "b3", P);
  TORCH_CHECK(b2.numel() == 64 && w3.numel() == 64 && b3.numel() == 1, "b2 / w3 / b3 must have 64 / 64 / 1 entries");
  TORCH_CHECK(k >= 1 && k <= DGMI_PAIR_TOPK_MAX_K, "k must be in 1..", DGMI_PAIR_TOPK_MAX_K, ", got ", k);
  const bool has_known = known_drug.has_value() && known_drug->defined();
  TORCH_CHECK(has_known == (known_dis.has_value() && known_dis->defined()), "known_drug and known_dis go together");
  c10::hip::HIPGuardMasqueradingAsCUDA guard(p.t.device());
  Tensor kd, ks;
  if (has_known) {
    for (const Tensor* t : {&*known_drug, &*known_dis}) {
      check_dev(*t, "known ids");
      TORCH_CHECK(t->dim() == 1 && (t->scalar_type() == at::kInt || t->scalar_type() == at::kLong) && t->device() == P.device(),
                  "known ids must be 1-D int32 / int64 tensors on ", P.device().str());
    }
    TORCH_CHECK(known_drug->numel() == known_dis->numel(), "known_drug / known_dis length mismatch");
    auto i32 = [](const Tensor& t) {
      return t.scalar_type() == at::kInt ? t.contiguous() : t.clamp(-1, (int64_t)INT32_MAX).to(at::kInt).contiguous();
    };
    kd = i32(*known_drug);
    ks = i32(*known_dis);
  }
  const int64_t n_known = has_known ? kd.numel() : 0;
  auto opts = p.t.options();
  Tensor out_drug = at::empty({k}, opts.dtype(at::kInt)), out_dis = at::empty({k}, opts.dtype(at::kInt));
  Tensor out_logit = at::empty({k}, opts.dtype(at::kFloat));
  Tensor info = at::zeros({2}, opts.dtype(at::kInt));
  if (p.rows == 0 || q.rows == 0) return {out_drug, out_dis, out_logit, info};
  Tensor W2c = contiguous16(W2), b2c = b2.contiguous(), w3c = w3.contiguous(), b3c = b3.contiguous();
  TORCH_CHECK(rows_16b_aligned(p.t, p.ld) && rows_16b_aligned(q.t, q.ld), "P and Q rows must be 16-B aligned");
  const size_t wbytes = dgmi_pair_topk_workspace_bytes(p.rows, q.rows, (int32_t)k);
  Tensor ws = at::empty({(int64_t)(wbytes < 16 ? 16 : wbytes)}, opts.dtype(at::kByte));
  check_status(dgmi_pair_mlp_topk_f32(p.t.data_ptr<float>(), p.ld, p.rows, q.t.data_ptr<float>(), q.ld, q.rows, 128, 64,
                                      W2c.data_ptr<float>(), b2c.data_ptr<float>(), w3c.data_ptr<float>(), b3c.data_ptr<float>(),
                                      has_known ? kd.data_ptr<int32_t>() : nullptr, has_known ? ks.data_ptr<int32_t>() : nullptr,
                                      n_known, (int32_t)k, out_drug.data_ptr<int32_t>(), out_dis.data_ptr<int32_t>(),
                                      out_logit.data_ptr<float>(), info.data_ptr<int32_t>(), ws.data_ptr(), (size_t)ws.numel(),
                                      stream_of(p.t)),
               "dgmi_pair_mlp_topk_f32");
  return {out_drug, out_dis, out_logit, info};
}

// the k best novel candidates of every query row under the decoder MLP (dgmi_pairs_rows.hip): candidate ids and logits
// (n_query x k, padded with -1 / NaN), per-row counts and info = [sum of counts, out-of-range flag].  X is the query side
// (Q for per-disease lists, P for per-drug lists), C the candidate side.  int64 known ids are clamped into
// [-1, INT32_MAX] on the device, as in pair_mlp_topk; nothing here synchronises.
std::tuple<Tensor, Tensor, Tensor, Tensor> pair_mlp_row_topk(const Tensor& X, const Tensor& C, const Tensor& W2, const Tensor& b2,
                                                             const Tensor& w3, const Tensor& b3, const OptTensor& known_query,
                                                             const OptTensor& known_cand, int64_t k) {
  Dense x = dense16_of(X, "X"), c = dense16_of(C, "C");
  TORCH_CHECK(x.F == 128 && c.F == 128, "X and C must have 128 columns (the decoder's lin1 width), got ", x.F, " and ", c.F);
  check(W2, at::kFloat, 2, "W2", X);
  TORCH_CHECK(W2.size(0) == 64 && W2.size(1) == 128, "W2 must be (64, 128), got (", W2.size(0), ", ", W2.size(1), ")");
  check(b2, at::kFloat, 1, "b2", X);
  check(w3, at::kFloat, 1, "w3", X);
  check(b3, at::kFloat, 1, "b3", X);
  TORCH_CHECK(b2.numel() == 64 && w3.numel() == 64 && b3.numel() == 1, "b2 / w3 / b3 must have 64 / 64 / 1 entries");
  TORCH_CHECK(k >= 1 && k <= DGMI_ROW_TOPK_MAX_K, "k must be in 1..", DGMI_ROW_TOPK_MAX_K, ", got ", k);
  const bool has_known = known_query.has_value() && known_query->defined();
  TORCH_CHECK(has_known == (known_cand.has_value() && known_cand->defined()), "known_query and known_cand go together");
  c10::hip::HIPGuardMasqueradingAsCUDA guard(x.t.device());
  Tensor kq, kc;
  if (has_known) {
    for (const Tensor* t : {&*known_query, &*known_cand}) {
      check_dev(*t, "known ids");
      TORCH_CHECK(t->dim() == 1 && (t->scalar_type() == at::kInt || t->scalar_type() == at::kLong) && t->device() == X.device(),
                  "known ids must be 1-D int32 / int64 tensors on ", X.device().str());
    }
    TORCH_CHECK(known_query->numel() == known_cand->numel(), "known_query / known_cand length mismatch");
    auto i32 = [](const Tensor& t) {
      return t.scalar_type() == at::kInt ? t.contiguous() : t.clamp(-1, (int64_t)INT32_MAX).to(at::kInt).contiguous();
    };
    kq = i32(*known_query);
    kc = i32(*known_cand);
  }
  const int64_t n_known = has_known ? kq.numel() : 0;
  auto opts = x.t.options();
  Tensor out_cand = at::empty({x.rows, k}, opts.dtype(at::kInt));
  Tensor out_logit = at::empty({x.rows, k}, opts.dtype(at::kFloat));
  Tensor out_count = at::empty({x.rows}, opts.dtype(at::kInt));
  Tensor info = at::zeros({2}, opts.dtype(at::kInt));
  if (x.rows == 0) return {out_cand, out_logit, out_count, info};
  Tensor W2c = contiguous16(W2), b2c = b2.contiguous(), w3c = w3.contiguous(), b3c = b3.contiguous();
  TORCH_CHECK(rows_16b_aligned(x.t, x.ld) && rows_16b_aligned(c.t, c.ld), "X and C rows must be 16-B aligned");
  // per call, from the caching allocator, as pair_mlp_topk
  const size_t wbytes = dgmi_row_topk_workspace_bytes(x.rows, c.rows, (int32_t)k);
  Tensor ws = at::empty({(int64_t)(wbytes < 16 ? 16 : wbytes)}, opts.dtype(at::kByte));
  check_status(dgmi_pair_mlp_row_topk_f32(x.t.data_ptr<float>(), x.ld, x.rows, c.t.data_ptr<float>(), c.ld, c.rows, 128, 64,
                                          W2c.data_ptr<float>(), b2c.data_ptr<float>(), w3c.data_ptr<float>(), b3c.data_ptr<float>(),
                                          has_known ? kq.data_ptr<int32_t>() : nullptr, has_known ? kc.data_ptr<int32_t>() : nullptr,
                                          n_known, (int32_t)k, out_cand.data_ptr<int32_t>(), out_logit.data_ptr<float>(),
                                          out_count.data_ptr<int32_t>(), info.data_ptr<int32_t>(), ws.data_ptr(), (size_t)ws.numel(),
                                          stream_of(x.t)),
               "dgmi_pair_mlp_row_topk_f32");
  return {out_cand, out_logit, out_count, info};
}

// the decoder MLP on GIVEN (query, candidate) pairs (dgmi_pairs_given.hip).  rank = false: logits only; rank = true: also
// above / total, the pair's position among the candidates of its query row that are not known (n_pairs x n_cand scores).
// info = [a listed id is out of range, a known id is out of range]; a pair out of range gets NaN / -1 / -1 and the others
// their results.  int64 ids are clamped into [-1, INT32_MAX] on the device, as in pair_mlp_topk; nothing here synchronises.
struct GivenOut {
  Tensor logit, above, total, info;
};

GivenOut pair_mlp_given(const Tensor& X, const Tensor& C, const Tensor& W2, const Tensor& b2, const Tensor& w3, const Tensor& b3,
                        const Tensor& pair_query, const Tensor& pair_cand, const OptTensor& known_query,
                        const OptTensor& known_cand, bool rank) {
  Dense x = dense16_of(X, "X"), c = dense16_of(C, "C");
  TORCH_CHECK(x.F == 128 && c.F == 128, "X and C must have 128 columns (the decoder's lin1 width), got ", x.F, " and ", c.F);
  check(W2, at::kFloat, 2, "W2", X);
  TORCH_CHECK(W2.size(0) == 64 && W2.size(1) == 128, "W2 must be (64, 128), got (", W2.size(0), ", ", W2.size(1), ")");
  check(b2, at::kFloat, 1, "b2", X);
  check(w3, at::kFloat, 1, "w3", X);
  check(b3, at::kFloat, 1, "b3", X);
  TORCH_CHECK(b2.numel() == 64 && w3.numel() == 64 && b3.numel() == 1, "b2 / w3 / b3 must have 64 / 64 / 1 entries");
  const bool has_known = known_query.has_value() && known_query->defined();
  TORCH_CHECK(has_known == (known_cand.has_value() && known_cand->defined()), "known_query and known_cand go together");
  c10::hip::HIPGuardMasqueradingAsCUDA guard(x.t.device());
  auto ids_ok = [&](const Tensor& t, const char* what) {
    check_dev(t, what);
    TORCH_CHECK(t.dim() == 1 && (t.scalar_type() == at::kInt || t.scalar_type() == at::kLong) && t.device() == X.device(), what,
                " must be 1-D int32 / int64 tensors on ", X.device().str());
  };
  auto i32 = [](const Tensor& t) {
    return t.scalar_type() == at::kInt ? t.contiguous() : t.clamp(-1, (int64_t)INT32_MAX).to(at::kInt).contiguous();
  };
  ids_ok(pair_query, "pair ids");
  ids_ok(pair_cand, "pair ids");
  TORCH_CHECK(pair_query.numel() == pair_cand.numel(), "pair_query / pair_cand length mismatch");
  Tensor pq = i32(pair_query), pc = i32(pair_cand), kq, kc;
  if (has_known) {
    ids_ok(*known_query, "known ids");
    ids_ok(*known_cand, "known ids");
    TORCH_CHECK(known_query->numel() == known_cand->numel(), "known_query / known_cand length mismatch");
    kq = i32(*known_query);
    kc = i32(*known_cand);
  }
  const int64_t n_pairs = pq.numel(), n_known = has_known ? kq.numel() : 0;
  auto opts = x.t.options();
  GivenOut o;
  o.logit = at::empty({n_pairs}, opts.dtype(at::kFloat));
  o.above = at::empty({rank ? n_pairs : 0}, opts.dtype(at::kInt));
  o.total = at::empty({rank ? n_pairs : 0}, opts.dtype(at::kInt));
  o.info = at::zeros({2}, opts.dtype(at::kInt));
  if (n_pairs == 0) return o;
  Tensor W2c = contiguous16(W2), b2c = b2.contiguous(), w3c = w3.contiguous(), b3c = b3.contiguous();
  TORCH_CHECK(rows_16b_aligned(x.t, x.ld) && rows_16b_aligned(c.t, c.ld), "X and C rows must be 16-B aligned");
  if (!rank) {
    check_status(dgmi_pair_mlp_score_list_f32(x.t.data_ptr<float>(), x.ld, x.rows, c.t.data_ptr<float>(), c.ld, c.rows, 128, 64,
                                              W2c.data_ptr<float>(), b2c.data_ptr<float>(), w3c.data_ptr<float>(),
                                              b3c.data_ptr<float>(), pq.data_ptr<int32_t>(), pc.data_ptr<int32_t>(), n_pairs,
                                              o.logit.data_ptr<float>(), o.info.data_ptr<int32_t>(), stream_of(x.t)),
                 "dgmi_pair_mlp_score_list_f32");
    return o;
  }
  // per call, from the caching allocator, as pair_mlp_topk
  const size_t wbytes = dgmi_pair_rank_workspace_bytes(x.rows, c.rows, n_pairs);
  Tensor ws = at::empty({(int64_t)(wbytes < 16 ? 16 : wbytes)}, opts.dtype(at::kByte));
  check_status(dgmi_pair_mlp_rank_list_f32(x.t.data_ptr<float>(), x.ld, x.rows, c.t.data_ptr<float>(), c.ld, c.rows, 128, 64,
                                           W2c.data_ptr<float>(), b2c.data_ptr<float>(), w3c.data_ptr<float>(),
                                           b3c.data_ptr<float>(), pq.data_ptr<int32_t>(), pc.data_ptr<int32_t>(), n_pairs,
                                           has_known ? kq.data_ptr<int32_t>() : nullptr,
                                           has_known ? kc.data_ptr<int32_t>() : nullptr, n_known, o.logit.data_ptr<float>(),
                                           o.above.data_ptr<int32_t>(), o.total.data_ptr<int32_t>(), o.info.data_ptr<int32_t>(),
                                           ws.data_ptr(), (size_t)ws.numel(), stream_of(x.t)),
               "dgmi_pair_mlp_rank_list_f32");
  return o;
}

std::tuple<Tensor, Tensor> pair_mlp_score_list(const Tensor& X, const Tensor& C, const Tensor& W2, const Tensor& b2,
                                               const Tensor& w3, const Tensor& b3, const Tensor& pair_query,
                                               const Tensor& pair_cand) {
  GivenOut o = pair_mlp_given(X, C, W2, b2, w3, b3, pair_query, pair_cand, c10::nullopt, c10::nullopt, false);
  return {o.logit, o.info};
}

std::tuple<Tensor, Tensor, Tensor, Tensor> pair_mlp_rank_list(const Tensor& X, const Tensor& C, const Tensor& W2, const Tensor& b2,
                                                              const Tensor& w3, const Tensor& b3, const Tensor& pair_query,
                                                              const Tensor& pair_cand, const OptTensor& known_query,
                                                              const OptTensor& known_cand) {
  GivenOut o = pair_mlp_given(X, C, W2, b2, w3, b3, pair_query, pair_cand, known_query, known_cand, true);
  return {o.logit, o.above, o.total, o.info};
}

// the decoder MLP on the TRAINING pair list (dgmi_pairs_train.hip): logits with dropout keyed by `seed` (one int64 on the
// device, read by the kernels), and every gradient from a recompute.  int32 ids as EdgePairs keeps them; info[0] = a
// listed id is out of range.  The backward's workspace (dZ2 and the workgroups' partial sums) is the per-(device, stream)
// scratch; nothing here synchronises, so both ops can be captured.
struct TrainOperands {
  Dense x, c;
  Tensor W2, b2, w3, b3, pq, pc, seed;
  int64_t n_pairs;
  float p;
};

TrainOperands train_operands(const Tensor& X, const Tensor& C, const Tensor& W2, const Tensor& b2, const Tensor& w3,
                             const Tensor& b3, const Tensor& pair_query, const Tensor& pair_cand, double p, const Tensor& seed) {
  TrainOperands o;
  o.x = dense16_of(X, "X");
  o.c = dense16_of(C, "C");
  TORCH_CHECK(o.x.F == 128 && o.c.F == 128, "X and C must have 128 columns (the decoder's lin1 width), got ", o.x.F, " and ", o.c.F);
  TORCH_CHECK(C.device() == X.device(), "tensors on different devices: C on ", C.device().str(), " vs ", X.device().str());
  check(W2, at::kFloat, 2, "W2", X);
  TORCH_CHECK(W2.size(0) == 64 && W2.size(1) == 128, "W2 must be (64, 128), got (", W2.size(0), ", ", W2.size(1), ")");
  check(b2, at::kFloat, 1, "b2", X);
  check(w3, at::kFloat, 1, "w3", X);
  check(b3, at::kFloat, 1, "b3", X);
  TORCH_CHECK(b2.numel() == 64 && w3.numel() == 64 && b3.numel() == 1, "b2 / w3 / b3 must have 64 / 64 / 1 entries");
  check(pair_query, at::kInt, 1, "pair_query", X);
  check(pair_cand, at::kInt, 1, "pair_cand", X);
  TORCH_CHECK(pair_query.numel() == pair_cand.numel(), "pair_query / pair_cand length mismatch");
  TORCH_CHECK(pair_query.numel() <= (int64_t)INT32_MAX, "at most 2^31 - 1 listed pairs");
  check(seed, at::kLong, 1, "seed", X);
  TORCH_CHECK(seed.numel() == 1, "seed must hold ONE int64, got ", seed.numel());
  TORCH_CHECK(p >= 0.0 && p < 1.0, "dropout p must be in [0, 1), got ", p);
  o.W2 = contiguous16(W2), o.b2 = b2, o.w3 = w3, o.b3 = b3, o.pq = pair_query, o.pc = pair_cand, o.seed = seed;
  o.n_pairs = pair_query.numel();
  o.p = (float)p;
  return o;
}

std::tuple<Tensor, Tensor> pair_mlp_train_forward(const Tensor& X, const Tensor& C, const Tensor& W2, const Tensor& b2,
                                                  const Tensor& w3, const Tensor& b3, const Tensor& pair_query,
                                                  const Tensor& pair_cand, double p, const Tensor& seed) {
  TrainOperands o = train_operands(X, C, W2, b2, w3, b3, pair_query, pair_cand, p, seed);
  c10::hip::HIPGuardMasqueradingAsCUDA guard(o.x.t.device());
  auto opts = o.x.t.options();
  Tensor logit = at::empty({o.n_pairs}, opts.dtype(at::kFloat));
  Tensor info = at::zeros({2}, opts.dtype(at::kInt));
  if (o.n_pairs == 0) return {logit, info};
  check_status(dgmi_pair_mlp_train_forward_f32(o.x.t.data_ptr<float>(), o.x.ld, o.x.rows, o.c.t.data_ptr<float>(), o.c.ld, o.c.rows,
                                               128, 64, o.W2.data_ptr<float>(), o.b2.data_ptr<float>(), o.w3.data_ptr<float>(),
                                               o.b3.data_ptr<float>(), o.pq.data_ptr<int32_t>(), o.pc.data_ptr<int32_t>(),
                                               o.n_pairs, o.p, o.seed.data_ptr<int64_t>(), logit.data_ptr<float>(),
                                               info.data_ptr<int32_t>(), stream_of(o.x.t)),
               "dgmi_pair_mlp_train_forward_f32");
  return {logit, info};
}

std::tuple<Tensor, Tensor, Tensor, Tensor, Tensor, Tensor> pair_mlp_train_backward(
    const Tensor& X, const Tensor& C, const Tensor& W2, const Tensor& b2, const Tensor& w3, const Tensor& b3,
    const Tensor& pair_query, const Tensor& pair_cand, double p, const Tensor& seed, const Tensor& dlogit) {
  TrainOperands o = train_operands(X, C, W2, b2, w3, b3, pair_query, pair_cand, p, seed);
  check(dlogit, at::kFloat, 1, "dlogit", X);
  TORCH_CHECK(dlogit.numel() == o.n_pairs, "dlogit has ", dlogit.numel(), " entries, the list has ", o.n_pairs, " pairs");
  c10::hip::HIPGuardMasqueradingAsCUDA guard(o.x.t.device());
  auto opts = o.x.t.options().dtype(at::kFloat);
  Tensor dz1 = at::empty({o.n_pairs, 128}, opts);
  Tensor info = at::zeros({2}, opts.dtype(at::kInt));
  if (o.n_pairs == 0) return {dz1, at::zeros({64, 128}, opts), at::zeros({64}, opts), at::zeros({64}, opts), at::zeros({1}, opts), info};
  Tensor dW2 = at::empty({64, 128}, opts), db2 = at::empty({64}, opts), dw3 = at::empty({64}, opts), db3 = at::empty({1}, opts);
  const size_t wbytes = dgmi_pair_mlp_train_workspace_bytes(o.n_pairs);
  Tensor ws = scratch(o.x.t, wbytes < 256 ? 256 : wbytes, kTrain);
  check_status(dgmi_pair_mlp_train_backward_f32(o.x.t.data_ptr<float>(), o.x.ld, o.x.rows, o.c.t.data_ptr<float>(), o.c.ld, o.c.rows,
                                                128, 64, o.W2.data_ptr<float>(), o.b2.data_ptr<float>(), o.w3.data_ptr<float>(),
                                                o.b3.data_ptr<float>(), o.pq.data_ptr<int32_t>(), o.pc.data_ptr<int32_t>(),
                                                o.n_pairs, o.p, o.seed.data_ptr<int64_t>(), dlogit.data_ptr<float>(),
                                                dz1.data_ptr<float>(), 128, dW2.data_ptr<float>(), db2.data_ptr<float>(),
                                                dw3.data_ptr<float>(), db3.data_ptr<float>(), info.data_ptr<int32_t>(),
                                                ws.data_ptr(), (size_t)ws.numel(), stream_of(o.x.t)),
               "dgmi_pair_mlp_train_backward_f32");
  return {dz1, dW2, db2, dw3, db3, info};
}

// the two-channel attention fusion in training (dgmi_attn.hip): out = beta'_0 A + beta'_1 B with beta = softmax over the two
// channels of w2 . tanh(W1 z + b1) and M the caller's (n, 2) dropout factors, and every gradient from a recompute.  A and
// B are consumed in place by leading dimension (the two halves z[:, 0] / z[:, 1] of a stacked (n, 2, F) tensor included);
// when they ARE such halves the backward writes dA / dB as the halves of one (n, 2, F) tensor.  The backward's workspace
// (the workgroups' partial sums) is the per-(device, stream) scratch; nothing here synchronises, so both ops can be captured.
struct AttnOperands {
  Dense a, b;
  Tensor W1, b1, w2, M;
  const float* m = nullptr;
};

AttnOperands attn_operands(const Tensor& A, const Tensor& B, const OptTensor& M, const Tensor& W1, const Tensor& b1, const Tensor& w2) {
  AttnOperands o;
  o.a = dense16_of(A, "A");
  o.b = dense16_of(B, "B");
  TORCH_CHECK(B.device() == A.device(), "tensors on different devices: B on ", B.device().str(), " vs ", A.device().str());
  TORCH_CHECK(o.a.rows == o.b.rows && o.a.F == o.b.F, "A and B must have one shape, got (", o.a.rows, ", ", o.a.F, ") and (",
              o.b.rows, ", ", o.b.F, ")");
  TORCH_CHECK(o.a.F >= 4 && o.a.F <= 512 && o.a.F % 4 == 0, "the width must be a multiple of 4 in [4, 512], got ", o.a.F);
  TORCH_CHECK(o.a.rows <= (int64_t)INT32_MAX, "at most 2^31 - 1 rows");
  check(W1, at::kFloat, 2, "W1", A);
  TORCH_CHECK(W1.size(0) == 16 && W1.size(1) == o.a.F, "W1 must be (16, ", o.a.F, "), got (", W1.size(0), ", ", W1.size(1), ")");
  check(b1, at::kFloat, 1, "b1", A);
  check(w2, at::kFloat, 1, "w2", A);
  TORCH_CHECK(b1.numel() == 16 && w2.numel() == 16, "b1 / w2 must have 16 entries");
  o.W1 = contiguous16(W1), o.b1 = b1, o.w2 = w2;
  if (M.has_value() && M->defined()) {
    check(*M, at::kFloat, 2, "M", A);
    TORCH_CHECK(M->size(0) == o.a.rows && M->size(1) == 2, "M must be (", o.a.rows, ", 2)");
    o.M = *M;
    o.m = o.M.data_ptr<float>();
  }
  return o;
}

std::tuple<Tensor, Tensor> attn_fuse_forward(const Tensor& A, const Tensor& B, const OptTensor& M, const Tensor& W1,
                                             const Tensor& b1, const Tensor& w2) {
  AttnOperands o = attn_operands(A, B, M, W1, b1, w2);
  c10::hip::HIPGuardMasqueradingAsCUDA guard(o.a.t.device());
  auto opts = o.a.t.options().dtype(at::kFloat);
  Tensor out = at::empty({o.a.rows, o.a.F}, opts), beta = at::empty({o.a.rows, 2}, opts);
  if (o.a.rows == 0) return {out, beta};
  check_status(dgmi_attn_fuse_forward_f32(o.a.t.data_ptr<float>(), o.a.ld, o.b.t.data_ptr<float>(), o.b.ld, o.a.rows, (int32_t)o.a.F,
                                          16, o.W1.data_ptr<float>(), o.b1.data_ptr<float>(), o.w2.data_ptr<float>(), o.m,
                                          out.data_ptr<float>(), o.a.F, beta.data_ptr<float>(), stream_of(o.a.t)),
               "dgmi_attn_fuse_forward_f32");
  return {out, beta};
}

std::tuple<Tensor, Tensor, Tensor, Tensor, Tensor> attn_fuse_backward(const Tensor& A, const Tensor& B, const OptTensor& M,
                                                                      const Tensor& W1, const Tensor& b1, const Tensor& w2,
                                                                      const Tensor& dout) {
  AttnOperands o = attn_operands(A, B, M, W1, b1, w2);
  Dense g = dense16_of(dout, "dout");
  TORCH_CHECK(dout.device() == A.device(), "tensors on different devices: dout on ", dout.device().str(), " vs ", A.device().str());
  TORCH_CHECK(g.rows == o.a.rows && g.F == o.a.F, "dout must be (", o.a.rows, ", ", o.a.F, "), got (", g.rows, ", ", g.F, ")");
  c10::hip::HIPGuardMasqueradingAsCUDA guard(o.a.t.device());
  auto opts = o.a.t.options().dtype(at::kFloat);
  const int64_t n = o.a.rows, F = o.a.F;
  Tensor dA, dB;
  int64_t ldd = F;
  if (n > 0 && o.a.ld == 2 * F && o.b.ld == 2 * F && o.b.t.data_ptr<float>() == o.a.t.data_ptr<float>() + F) {
    Tensor dz = at::empty({n, 2, F}, opts);  // the halves of one stacked tensor: one dz, no stack in the caller
    dA = dz.select(1, 0), dB = dz.select(1, 1), ldd = 2 * F;
  } else {
    dA = at::empty({n, F}, opts), dB = at::empty({n, F}, opts);
  }
  if (n == 0) return {dA, dB, at::zeros({16, F}, opts), at::zeros({16}, opts), at::zeros({16}, opts)};
  Tensor dW1 = at::empty({16, F}, opts), db1 = at::empty({16}, opts), dw2 = at::empty({16}, opts);
  const size_t wbytes = dgmi_attn_fuse_workspace_bytes(n, (int32_t)F);
  Tensor ws = scratch(o.a.t, wbytes < 256 ? 256 : wbytes, kAttn);
  check_status(dgmi_attn_fuse_backward_f32(o.a.t.data_ptr<float>(), o.a.ld, o.b.t.data_ptr<float>(), o.b.ld, n, (int32_t)F, 16,
                                           o.W1.data_ptr<float>(), o.b1.data_ptr<float>(), o.w2.data_ptr<float>(), o.m,
                                           g.t.data_ptr<float>(), g.ld, dA.data_ptr<float>(), ldd, dB.data_ptr<float>(), ldd,
                                           dW1.data_ptr<float>(), db1.data_ptr<float>(), dw2.data_ptr<float>(), ws.data_ptr(),
                                           (size_t)ws.numel(), stream_of(o.a.t)),
               "dgmi_attn_fuse_backward_f32");
  return {dA, dB, dW1, db1, dw2};
}

// exact AUROC / AUPR of scored samples, overall (n_segments = 0) or per segment (dgmi_curve.hip): count = (S, 6) int64
// rows (P, N, TP at the threshold, FP at the threshold, groups, U2), area = (S, 2) float64 rows (auroc, aupr), info =
// [flag word] (bit 0 NaN score, bit 1 label not 0 / 1, bit 2 segment id out of range).  Any shape of score (flattened);
// labels of bool / integer dtype become fp32, segments int32; the inputs are not modified.  The workspace comes from
// the caching allocator per call, as pair_mlp_topk; nothing synchronises.  Not differentiable.
std::tuple<Tensor, Tensor, Tensor> curve_areas(const Tensor& score, const Tensor& label, const OptTensor& segment,
                                               int64_t n_segments, double threshold) {
  check_dev(score, "score");
  check_dev(label, "label");
  TORCH_CHECK(score.scalar_type() == at::kFloat, "score must be float32, got ", c10::toString(score.scalar_type()));
  TORCH_CHECK(label.device() == score.device(), "tensors on different devices: label on ", label.device().str(), " vs ",
              score.device().str());
  const auto lt = label.scalar_type();
  TORCH_CHECK(lt == at::kFloat || lt == at::kBool || c10::isIntegralType(lt, false), "label must be float32, bool or an integer dtype, got ",
              c10::toString(lt));
  TORCH_CHECK(n_segments >= 0 && n_segments <= DGMI_CURVE_MAX_SEGMENTS, "n_segments must be in 0..", DGMI_CURVE_MAX_SEGMENTS,
              ", got ", n_segments);
  const bool has_seg = segment.has_value() && segment->defined();
  TORCH_CHECK(has_seg == (n_segments > 0), "segment ids and n_segments > 0 go together");
  c10::hip::HIPGuardMasqueradingAsCUDA guard(score.device());
  Tensor sc = score.reshape({-1}).contiguous();
  Tensor lb = label.reshape({-1}).to(at::kFloat).contiguous();
  const int64_t n = sc.numel();
  TORCH_CHECK(lb.numel() == n, "score has ", n, " entries, label has ", lb.numel());
  TORCH_CHECK(n <= (int64_t)INT32_MAX, "at most 2^31 - 1 samples, got ", n);
  Tensor sg;
  if (has_seg) {
    check_dev(*segment, "segment");
    const auto st = segment->scalar_type();
    TORCH_CHECK((st == at::kInt || st == at::kLong) && segment->device() == score.device(),
                "segment must be an int32 / int64 tensor on ", score.device().str());
    Tensor flat = segment->reshape({-1});
    TORCH_CHECK(flat.numel() == n, "score has ", n, " entries, segment has ", flat.numel());
    sg = st == at::kInt ? flat.contiguous() : flat.clamp(-1, (int64_t)INT32_MAX).to(at::kInt).contiguous();
  }
  const int64_t S = n_segments > 0 ? n_segments : 1;
  auto opts = sc.options();
  Tensor count = at::empty({S, 6}, opts.dtype(at::kLong)), area = at::empty({S, 2}, opts.dtype(at::kDouble));
  Tensor info = at::empty({1}, opts.dtype(at::kInt));
  const size_t wbytes = dgmi_curve_areas_workspace_bytes(n, n_segments);
  Tensor ws = at::empty({(int64_t)(wbytes < 16 ? 16 : wbytes)}, opts.dtype(at::kByte));
  check_status(dgmi_curve_areas_f32(n ? sc.data_ptr<float>() : nullptr, n ? lb.data_ptr<float>() : nullptr,
                                    // an empty tensor has no storage; with n = 0 no id is read, any non-null pointer does
                                    has_seg ? (n ? sg.data_ptr<int32_t>() : reinterpret_cast<const int32_t*>(ws.data_ptr())) : nullptr,
                                    n, n_segments, (float)threshold, count.data_ptr<int64_t>(), area.data_ptr<double>(),
                                    info.data_ptr<int32_t>(), ws.data_ptr(), (size_t)ws.numel(), stream_of(sc)),
               "dgmi_curve_areas_f32");
  return {count, area, info};
}

// every novel pair whose decoder logit reaches `min_logit` (dgmi_pairs_above.hip), appended in scheduling order to the
// caller's record tensors (capacity = their length; 0 = count only): returns count = [the exact int64 number of
// qualifying pairs, which may exceed the capacity] and info = [0, out-of-range flag].  Nothing is written past the
// capacity.  Known ids as in pair_mlp_topk; the bitmap lives in the per-(device, stream) scratch; nothing synchronises.
std::tuple<Tensor, Tensor> pair_mlp_emit(const Tensor& P, const Tensor& Q, const Tensor& W2, const Tensor& b2, const Tensor& w3,
                                         const Tensor& b3, const OptTensor& known_drug, const OptTensor& known_dis,
                                         double min_logit, Tensor out_drug, Tensor out_dis, Tensor out_logit) {
  Dense p = dense16_of(P, "P"), q = dense16_of(Q, "Q");
  TORCH_CHECK(p.F == 128 && q.F == 128, "P and Q must have 128 columns (the decoder's lin1 width), got ", p.F, " and ", q.F);
  check(W2, at::kFloat, 2, "W2", P);
  TORCH_CHECK(W2.size(0) == 64 && W2.size(1) == 128, "W2 must be (64, 128), got (", W2.size(0), ", ", W2.size(1), ")");
  check(b2, at::kFloat, 1, "b2", P);
  check(w3, at::kFloat, 1, "w3", P);
  check(b3, at::kFloat, 1, "b3", P);
  TORCH_CHECK(b2.numel() == 64 && w3.numel() == 64 && b3.numel() == 1, "b2 / w3 / b3 must have 64 / 64 / 1 entries");
  check(out_drug, at::kInt, 1, "out_drug", P);
  check(out_dis, at::kInt, 1, "out_dis", P);
  check(out_logit, at::kFloat, 1, "out_logit", P);
  const int64_t capacity = out_drug.numel();
  TORCH_CHECK(out_dis.numel() == capacity && out_logit.numel() == capacity, "out_drug / out_dis / out_logit length mismatch");
  TORCH_CHECK(capacity <= DGMI_PAIR_EMIT_MAX_RECORDS, "at most ", DGMI_PAIR_EMIT_MAX_RECORDS, " records per pass, got ", capacity);
  const bool has_known = known_drug.has_value() && known_drug->defined();
  TORCH_CHECK(has_known == (known_dis.has_value() && known_dis->defined()), "known_drug and known_dis go together");
  c10::hip::HIPGuardMasqueradingAsCUDA guard(p.t.device());
  Tensor kd, ks;
  if (has_known) {
    for (const Tensor* t : {&*known_drug, &*known_dis}) {
      check_dev(*t, "known ids");
      TORCH_CHECK(t->dim() == 1 && (t->scalar_type() == at::kInt || t->scalar_type() == at::kLong) && t->device() == P.device(),
                  "known ids must be 1-D int32 / int64 tensors on ", P.device().str());
    }
    TORCH_CHECK(known_drug->numel() == known_dis->numel(), "known_drug / known_dis length mismatch");
    auto i32 = [](const Tensor& t) {
      return t.scalar_type() == at::kInt ? t.contiguous() : t.clamp(-1, (int64_t)INT32_MAX).to(at::kInt).contiguous();
    };
    kd = i32(*known_drug);
    ks = i32(*known_dis);
  }
  const int64_t n_known = has_known ? kd.numel() : 0;
  auto opts = p.t.options();
  Tensor count = at::zeros({1}, opts.dtype(at::kLong)), info = at::zeros({2}, opts.dtype(at::kInt));
  if (p.rows == 0 || q.rows == 0) return {count, info};
  Tensor W2c = contiguous16(W2), b2c = b2.contiguous(), w3c = w3.contiguous(), b3c = b3.contiguous();
  TORCH_CHECK(rows_16b_aligned(p.t, p.ld) && rows_16b_aligned(q.t, q.ld), "P and Q rows must be 16-B aligned");
  const size_t wbytes = dgmi_pair_emit_workspace_bytes(p.rows, q.rows);
  Tensor ws = scratch(p.t, wbytes < 256 ? 256 : wbytes, kPairs);
  check_status(dgmi_pair_mlp_emit_f32(p.t.data_ptr<float>(), p.ld, p.rows, q.t.data_ptr<float>(), q.ld, q.rows, 128, 64,
                                      W2c.data_ptr<float>(), b2c.data_ptr<float>(), w3c.data_ptr<float>(), b3c.data_ptr<float>(),
                                      has_known ? kd.data_ptr<int32_t>() : nullptr, has_known ? ks.data_ptr<int32_t>() : nullptr,
                                      n_known, (float)min_logit, capacity, capacity ? out_drug.data_ptr<int32_t>() : nullptr,
                                      capacity ? out_dis.data_ptr<int32_t>() : nullptr,
                                      capacity ? out_logit.data_ptr<float>() : nullptr, count.data_ptr<int64_t>(),
                                      info.data_ptr<int32_t>(), ws.data_ptr(), (size_t)ws.numel(), stream_of(p.t)),
               "dgmi_pair_mlp_emit_f32");
  return {count, info};
}

// the first n records of (drug, dis, logit) into the ranking order, in place (dgmi_pair_records_sort_f32): logit
// descending, ties by (drug, dis) ascending, NaN last
void pair_records_sort(Tensor drug, Tensor dis, Tensor logit, int64_t n) {
  check(drug, at::kInt, 1, "drug", drug);
  check(dis, at::kInt, 1, "dis", drug);
  check(logit, at::kFloat, 1, "logit", drug);
  TORCH_CHECK(n >= 0 && n <= drug.numel() && n <= dis.numel() && n <= logit.numel(), "n = ", n, " is outside the record tensors");
  TORCH_CHECK(n <= DGMI_PAIR_EMIT_MAX_RECORDS, "at most ", DGMI_PAIR_EMIT_MAX_RECORDS, " records per sort, got ", n);
  if (n == 0) return;
  c10::hip::HIPGuardMasqueradingAsCUDA guard(drug.device());
  const size_t wbytes = dgmi_pair_records_sort_workspace_bytes(n);
  Tensor ws = scratch(drug, wbytes < 256 ? 256 : wbytes, kPairs);
  check_status(dgmi_pair_records_sort_f32(drug.data_ptr<int32_t>(), dis.data_ptr<int32_t>(), logit.data_ptr<float>(), n,
                                          ws.data_ptr(), (size_t)ws.numel(), stream_of(drug)),
               "dgmi_pair_records_sort_f32");
}

// `like`: any tensor on the target device (the op needs a device to allocate on)
Tensor random_subset_select(const Tensor& like, int64_t E, int64_t keep, int64_t seed, int64_t e_offset) {
  check_dev(like, "like");
  c10::hip::HIPGuardMasqueradingAsCUDA guard(like.device());
  Tensor desc = at::empty({8}, like.options().dtype(at::kInt));
  const size_t nbytes = dgmi_random_subset_workspace_bytes();
  Tensor ws = at::empty({(int64_t)nbytes}, like.options().dtype(at::kByte));  // own buffer: selections of one step overlap
  check_status(dgmi_random_subset_select(E, keep, (uint64_t)seed, (uint32_t)e_offset,
                                         reinterpret_cast<uint32_t*>(desc.data_ptr<int32_t>()), ws.data_ptr(), nbytes,
                                         stream_of(like)), "dgmi_random_subset_select");
  return desc;
}

// n <= 8 subsets with one series of launches; returns (n, 8) descriptions
Tensor random_subset_select_batch(const Tensor& like, at::IntArrayRef E, at::IntArrayRef keep, at::IntArrayRef seed,
                                  at::IntArrayRef e_offset) {
  check_dev(like, "like");
  const int64_t n = (int64_t)E.size();
  TORCH_CHECK(n >= 1 && n <= 8 && (int64_t)keep.size() == n && (int64_t)seed.size() == n &&
                  (e_offset.empty() || (int64_t)e_offset.size() == n),
              "random_subset_select_batch: 1..8 subsets, E / keep / seed (/ e_offset) of equal length");
  c10::hip::HIPGuardMasqueradingAsCUDA guard(like.device());
  Tensor descs = at::empty({n, 8}, like.options().dtype(at::kInt));
  const size_t nbytes = dgmi_random_subset_workspace_bytes();
  Tensor ws = at::empty({(int64_t)nbytes}, like.options().dtype(at::kByte));
  uint64_t seeds[8];
  uint32_t offs[8];
  for (int64_t i = 0; i < n; ++i) {
    seeds[i] = (uint64_t)seed[i];
    offs[i] = e_offset.empty() ? 0u : (uint32_t)e_offset[i];
  }
  check_status(dgmi_random_subset_select_batch((int32_t)n, E.data(), keep.data(), seeds, offs,
                                               reinterpret_cast<uint32_t*>(descs.data_ptr<int32_t>()), ws.data_ptr(), nbytes,
                                               stream_of(like)), "dgmi_random_subset_select_batch");
  return descs;
}

// the same with the seeds in a device tensor (int64, n entries): nothing host-side goes into the launches but the
// list lengths, so the call can sit inside a captured HIP graph and still select new subsets on every replay
Tensor random_subset_select_batch_dseed(const Tensor& seeds, at::IntArrayRef E, at::IntArrayRef keep, at::IntArrayRef e_offset) {
  check_dev(seeds, "seeds");
  const int64_t n = (int64_t)E.size();
  TORCH_CHECK(n >= 1 && n <= 8 && (int64_t)keep.size() == n && (e_offset.empty() || (int64_t)e_offset.size() == n),
              "random_subset_select_batch_dseed: 1..8 subsets, E / keep (/ e_offset) of equal length");
  TORCH_CHECK(seeds.scalar_type() == at::kLong && seeds.is_contiguous() && seeds.numel() == n,
              "seeds must be a contiguous int64 tensor with one entry per subset");
  c10::hip::HIPGuardMasqueradingAsCUDA guard(seeds.device());
  Tensor descs = at::empty({n, 8}, seeds.options().dtype(at::kInt));
  const size_t nbytes = dgmi_random_subset_workspace_bytes();
  Tensor ws = at::empty({(int64_t)nbytes}, seeds.options().dtype(at::kByte));
  uint32_t offs[8];
  for (int64_t i = 0; i < n; ++i) offs[i] = e_offset.empty() ? 0u : (uint32_t)e_offset[i];
  check_status(dgmi_random_subset_select_batch_dseed((int32_t)n, E.data(), keep.data(),
                                                     reinterpret_cast<const uint64_t*>(seeds.data_ptr<int64_t>()), offs,
                                                     reinterpret_cast<uint32_t*>(descs.data_ptr<int32_t>()), ws.data_ptr(), nbytes,
                                                     stream_of(seeds)), "dgmi_random_subset_select_batch_dseed");
  return descs;
}

Tensor keep_mask(const Tensor& keep, int64_t E) {
  check_dev(keep, "keep");
  TORCH_CHECK(keep.scalar_type() == at::kInt && keep.is_contiguous() && keep.dim() == 2 && keep.size(1) == 8 && keep.size(0) <= 8,
              "keep must be a contiguous (n <= 8, 8) int32 tensor of subset descriptions");
  c10::hip::HIPGuardMasqueradingAsCUDA guard(keep.device());
  Tensor mask = at::empty({E}, keep.options().dtype(at::kFloat));
  check_status(dgmi_keep_mask_f32(reinterpret_cast<const uint32_t*>(keep.data_ptr<int32_t>()), (int32_t)keep.size(0), E,
                                  mask.data_ptr<float>(), stream_of(keep)), "dgmi_keep_mask_f32");
  return mask;
}

// (D3) the layout with the edges dropped under `keep` removed: (ptr_out, indices_out[, vals_out]); indices_out / vals_out
// keep the parent's length (the survivors fill a prefix: nothing is read back to size them)
std::tuple<Tensor, Tensor, Tensor> compact_layout(const Tensor& ptr, const Tensor& indices, const OptTensor& vals, const Tensor& eid,
                                                  const Tensor& keep) {
  check(ptr, at::kInt, 1, "ptr", ptr);
  check(indices, at::kInt, 1, "indices", ptr);
  const int64_t nnz = indices.numel();
  check_opt(vals, at::kFloat, nnz, "vals", ptr);
  const Keep k = keep_of(eid, keep, nnz, ptr, false);
  TORCH_CHECK(k.n > 0, "compact_layout needs at least one subset description");
  c10::hip::HIPGuardMasqueradingAsCUDA guard(ptr.device());
  Tensor ptr_out = at::empty_like(ptr), indices_out = at::empty_like(indices);
  const bool has_vals = vals.has_value() && vals->defined();
  Tensor vals_out = has_vals ? at::empty_like(*vals) : Tensor();
  const size_t wbytes = dgmi_compact_layout_workspace_bytes(nnz);
  Tensor ws = scratch(ptr, wbytes < 256 ? 256 : wbytes, kBuilder);
  check_status(dgmi_compact_layout_i32(ptr.data_ptr<int32_t>(), ptr.numel(), indices.data_ptr<int32_t>(), (const float*)optptr(vals),
                                       k.eid, nnz, k.table, k.n, ptr_out.data_ptr<int32_t>(), indices_out.data_ptr<int32_t>(),
                                       has_vals ? vals_out.data_ptr<float>() : nullptr, ws.data_ptr(), (size_t)ws.numel(),
                                       stream_of(ptr)), "dgmi_compact_layout_i32");
  return {ptr_out, indices_out, has_vals ? vals_out : at::empty({0}, ptr.options().dtype(at::kFloat))};
}

// (D2) row scale x multiplicity form of a weighted CSR: (row_scale[n_rows], mult[nnz] = m - 1, fail[1])
std::tuple<Tensor, Tensor, Tensor> row_multiplicity(const Tensor& indptr, const Tensor& vals, double rel_tol) {
  check(indptr, at::kInt, 1, "indptr", indptr);
  check(vals, at::kFloat, 1, "vals", indptr);
  c10::hip::HIPGuardMasqueradingAsCUDA guard(indptr.device());
  const int64_t n_rows = indptr.numel() - 1, nnz = vals.numel();
  Tensor scale = at::empty({n_rows}, vals.options()), mult = at::empty({nnz}, indptr.options()), fail = at::empty({1}, indptr.options());
  check_status(dgmi_row_multiplicity_f32(indptr.data_ptr<int32_t>(), vals.data_ptr<float>(), n_rows, nnz, (float)rel_tol,
                                         scale.data_ptr<float>(), mult.data_ptr<int32_t>(), fail.data_ptr<int32_t>(), stream_of(indptr)),
               "dgmi_row_multiplicity_f32");
  return {scale, mult, fail};
}

Tensor spmm_csr_new(const Tensor& indptr, const Tensor& indices, const OptTensor& vals, const OptTensor& eid, const OptTensor& keep,
                    const Tensor& X, const OptTensor& ss, const OptTensor& ds, const OptTensor& plan, int64_t chunk,
                    int64_t act, double slope, const OptTensor& out_mask, double mask_scale) {
  return spmm_csr_raw(indptr, indices, vals, eid, keep, X, ss, ds, plan, chunk, c10::nullopt, act, slope, out_mask, mask_scale);
}
void spmm_csr_out(const Tensor& indptr, const Tensor& indices, const OptTensor& vals, const OptTensor& eid, const OptTensor& keep,
                  const Tensor& X, const OptTensor& ss, const OptTensor& ds, const OptTensor& plan, int64_t chunk, Tensor out,
                  int64_t act, double slope, const OptTensor& out_mask, double mask_scale) {
  spmm_csr_raw(indptr, indices, vals, eid, keep, X, ss, ds, plan, chunk, out, act, slope, out_mask, mask_scale);
}
Tensor spmm_sliced_new(const Tensor& segptr, const Tensor& indices, const OptTensor& vals, const OptTensor& eid,
                       const OptTensor& keep, const Tensor& X, const OptTensor& ss, const OptTensor& ds, int64_t n_dst,
                       int64_t n_slices, int64_t act, double slope, const OptTensor& out_mask, double mask_scale,
                       int64_t column_passes, int64_t id_mult) {
  return spmm_sliced_raw(segptr, indices, vals, eid, keep, X, ss, ds, n_dst, n_slices, c10::nullopt, act, slope, out_mask,
                         mask_scale, column_passes, id_mult);
}
void spmm_sliced_out(const Tensor& segptr, const Tensor& indices, const OptTensor& vals, const OptTensor& eid,
                     const OptTensor& keep, const Tensor& X, const OptTensor& ss, const OptTensor& ds, int64_t n_dst,
                     int64_t n_slices, Tensor out, int64_t act, double slope, const OptTensor& out_mask, double mask_scale,
                     int64_t column_passes, int64_t id_mult) {
  spmm_sliced_raw(segptr, indices, vals, eid, keep, X, ss, ds, n_dst, n_slices, out, act, slope, out_mask, mask_scale,
                  column_passes, id_mult);
}

// bf16_rne(diag(scale) X) in one streaming pass: the gather table of spmm_sliced_bf16_raw (include/dgmi_bf16.h)
Tensor rows_to_bf16(const Tensor& X, const OptTensor& scale) {
  Dense x = dense16_of(X, "X");
  TORCH_CHECK(x.F % 8 == 0, "rows_to_bf16: X must have a multiple of 8 columns (16-B rows of bf16), got ", x.F);
  check_opt(scale, at::kFloat, x.rows, "scale", x.t);
  c10::hip::HIPGuardMasqueradingAsCUDA guard(x.t.device());
  Tensor out = at::empty({x.rows, x.F}, x.t.options().dtype(at::kBFloat16));
  if (x.F == 0) return out;  // no column: the leading dimension 1 of an (n, 0) tensor is not one the C ABI takes (ld % 4)
  check_status(dgmi_rows_to_bf16(x.t.data_ptr<float>(), x.ld, (const float*)optptr(scale), x.rows, x.F,
                                 reinterpret_cast<uint16_t*>(out.data_ptr()), x.F > 0 ? x.F : 8, stream_of(x.t)),
               "dgmi_rows_to_bf16");
  return out;
}

// the XCD-local product gathering from a bf16 table; accumulation, planes and output fp32 (dgmi_spmm_sliced_bf16)
Tensor spmm_sliced_bf16_impl(const Tensor& segptr, const Tensor& indices, const OptTensor& vals, const OptTensor& eid,
                             const OptTensor& keep, const Tensor& X, const OptTensor& dst_scale, int64_t n_dst, int64_t n_slices,
                             const OptTensor& out, int64_t act, double slope, const OptTensor& out_mask, double mask_scale,
                             int64_t column_passes, int64_t id_mult) {
  check(segptr, at::kInt, 1, "segptr", segptr);
  check(indices, at::kInt, 1, "indices", segptr);
  TORCH_CHECK(segptr.numel() == n_slices * n_dst + 1, "segptr has ", segptr.numel(), " entries, expected n_slices * n_dst + 1");
  check_dev(X, "X");
  TORCH_CHECK(X.scalar_type() == at::kBFloat16 && X.dim() == 2, "X must be a 2-D bfloat16 tensor");
  TORCH_CHECK(X.device() == segptr.device(), "X and the graph are on different devices");
  TORCH_CHECK(X.size(1) % 8 == 0, "the bf16 gather needs a multiple of 8 columns (16-B rows), got ", X.size(1));
  Tensor x = X;  // rows contiguous, 16-B aligned: a row-strided view is consumed in place, anything else is copied
  if (X.stride(1) != 1 || (X.size(0) > 1 && (X.stride(0) < X.size(1) || X.stride(0) % 8 != 0)) ||
      (reinterpret_cast<uintptr_t>(X.data_ptr()) & 15))
    x = X.clone(at::MemoryFormat::Contiguous);
  const int64_t rows = x.size(0), F = x.size(1), ldx = rows > 1 ? x.stride(0) : (F > 0 ? F : 8);
  const int64_t nnz = indices.numel();
  check_opt(vals, at::kFloat, nnz, "vals", segptr);
  check_opt(dst_scale, at::kFloat, n_dst, "dst_scale", segptr);
  const Keep k = keep_of(eid, keep, nnz, segptr);
  c10::hip::HIPGuardMasqueradingAsCUDA guard(segptr.device());
  Tensor y = out_of(out, n_dst, F, segptr);
  const Epi e = epi_of(act, slope, out_mask, mask_scale, n_dst, F, segptr);
  const size_t pbytes = dgmi_spmm_sliced_planes_bytes(n_dst, (int32_t)n_slices, F);
  Tensor planes = scratch(segptr, pbytes, kPlanes);
  check_status(dgmi_spmm_sliced_bf16(segptr.data_ptr<int32_t>(), indices.data_ptr<int32_t>(), (const float*)optptr(vals), k.eid,
                                     k.table, k.n, reinterpret_cast<const uint16_t*>(x.data_ptr()), ldx,
                                     (const float*)optptr(dst_scale), y.data_ptr<float>(), F, n_dst, rows, F, (int32_t)n_slices,
                                     (int32_t)column_passes, (int32_t)id_mult, planes.data_ptr(), pbytes, e.act, e.slope, e.mask,
                                     e.ldm, e.mscale, stream_of(segptr)), "dgmi_spmm_sliced_bf16");
  return y;
}

Tensor spmm_sliced_bf16_new(const Tensor& segptr, const Tensor& indices, const OptTensor& vals, const OptTensor& eid,
                            const OptTensor& keep, const Tensor& X, const OptTensor& ds, int64_t n_dst, int64_t n_slices,
                            int64_t act, double slope, const OptTensor& out_mask, double mask_scale, int64_t column_passes,
                            int64_t id_mult) {
  return spmm_sliced_bf16_impl(segptr, indices, vals, eid, keep, X, ds, n_dst, n_slices, c10::nullopt, act, slope, out_mask,
                               mask_scale, column_passes, id_mult);
}
void spmm_sliced_bf16_out(const Tensor& segptr, const Tensor& indices, const OptTensor& vals, const OptTensor& eid,
                          const OptTensor& keep, const Tensor& X, const OptTensor& ds, int64_t n_dst, int64_t n_slices, Tensor out,
                          int64_t act, double slope, const OptTensor& out_mask, double mask_scale, int64_t column_passes,
                          int64_t id_mult) {
  spmm_sliced_bf16_impl(segptr, indices, vals, eid, keep, X, ds, n_dst, n_slices, out, act, slope, out_mask, mask_scale,
                        column_passes, id_mult);
}

// ---------------------------------------------------------------------------------------------
// dreamgnn_mi::spmm_csr — the functional op of §8(b), with autograd w.r.t. X.
Tensor spmm_csr_forward(const Tensor& indptr, const Tensor& indices, const OptTensor& vals, const Tensor& X,
                        const OptTensor& src_scale, const OptTensor& dst_scale) {
  return spmm_csr_raw(indptr, indices, vals, c10::nullopt, c10::nullopt, X, src_scale, dst_scale, c10::nullopt, 0, c10::nullopt);
}

class SpmmCsrFunction : public torch::autograd::Function<SpmmCsrFunction> {
 public:
  static Tensor forward(torch::autograd::AutogradContext* ctx, const Tensor& indptr, const Tensor& indices,
                        const OptTensor& vals, const Tensor& X, const OptTensor& src_scale, const OptTensor& dst_scale) {
    TORCH_CHECK(!(src_scale.has_value() && src_scale->defined() && src_scale->requires_grad()) &&
                    !(dst_scale.has_value() && dst_scale->defined() && dst_scale->requires_grad()) &&
                    !(vals.has_value() && vals->defined() && vals->requires_grad()),
                "spmm_csr: gradients w.r.t. edge values and the diagonal scales are not part of the path "
                "(adjacency values are constants, ci / cj are non-learnable node data)");
    at::AutoDispatchBelowADInplaceOrView guard;
    ctx->save_for_backward({indptr, indices, vals.value_or(Tensor()), src_scale.value_or(Tensor()), dst_scale.value_or(Tensor())});
    ctx->saved_data["n_src"] = X.size(0);
    static auto op = c10::Dispatcher::singleton().findSchemaOrThrow("dreamgnn_mi::spmm_csr", "").typed<decltype(spmm_csr_forward)>();
    return op.call(indptr, indices, vals, X, src_scale, dst_scale);
  }

  static torch::autograd::variable_list backward(torch::autograd::AutogradContext* ctx, torch::autograd::variable_list grads) {
    const auto saved = ctx->get_saved_variables();
    const Tensor &indptr = saved[0], &indices = saved[1], &vals = saved[2], &ss = saved[3], &ds = saved[4];
    const int64_t n_src = ctx->saved_data["n_src"].toInt(), n_dst = indptr.numel() - 1;
    Tensor dX;
    if (grads[0].defined()) {  // X is the only differentiable input (forward refuses the others)
      // dX = diag(ss) A^T diag(ds) dY: the same kernel on the CSR of the reversed edges (built here;
      // callers with a graph object — dream_gnn_amd.ops.CSRGraph — keep it cached instead)
      const Tensor deg = indptr.slice(0, 1) - indptr.slice(0, 0, n_dst);
      const Tensor rows = at::repeat_interleave(at::arange(n_dst, indptr.options()), deg, c10::nullopt, indices.numel());
      auto t = csr_from_coo(indices, rows.to(at::kInt), n_src, n_dst);
      OptTensor vals_t = vals.defined() ? OptTensor(gather_f32(vals, std::get<2>(t))) : c10::nullopt;
      dX = spmm_csr_raw(std::get<0>(t), std::get<1>(t), vals_t, c10::nullopt, c10::nullopt, grads[0].contiguous(),
                        ds.defined() ? OptTensor(ds) : c10::nullopt, ss.defined() ? OptTensor(ss) : c10::nullopt,
                        c10::nullopt, 0, c10::nullopt);
    }
    return {Tensor(), Tensor(), Tensor(), dX, Tensor(), Tensor()};
  }
};

Tensor spmm_csr_autograd(const Tensor& indptr, const Tensor& indices, const OptTensor& vals, const Tensor& X,
                         const OptTensor& src_scale, const OptTensor& dst_scale) {
  return SpmmCsrFunction::apply(indptr, indices, vals, X, src_scale, dst_scale);
}

}  // namespace

TORCH_LIBRARY(dreamgnn_mi, m) {
  m.def("csr_from_coo(Tensor row, Tensor col, int n_rows, int n_cols=0) -> (Tensor, Tensor, Tensor, Tensor)");
  m.def("csr_sliced_from_coo(Tensor row, Tensor col, int n_rows, int n_cols, int n_slices) -> (Tensor, Tensor, Tensor, Tensor)");
  m.def("csr_sliced_from_csr(Tensor indptr, Tensor indices, Tensor eid, int n_cols, int n_slices) -> (Tensor, Tensor, Tensor, Tensor)");
  m.def("plan_build(Tensor indptr, int nnz, int chunk) -> Tensor");
  m.def("spmm_csr(Tensor indptr, Tensor indices, Tensor? vals, Tensor X, Tensor? src_scale=None, Tensor? dst_scale=None) -> Tensor");
  m.def("spmm_csr_raw(Tensor indptr, Tensor indices, Tensor? vals, Tensor? eid, Tensor? keep, Tensor X, Tensor? src_scale, "
        "Tensor? dst_scale, Tensor? plan, int chunk, int act=0, float slope=0., Tensor? out_mask=None, float mask_scale=1.) -> Tensor");
  m.def("spmm_csr_out(Tensor indptr, Tensor indices, Tensor? vals, Tensor? eid, Tensor? keep, Tensor X, Tensor? src_scale, "
        "Tensor? dst_scale, Tensor? plan, int chunk, Tensor(a!) out, int act=0, float slope=0., Tensor? out_mask=None, "
        "float mask_scale=1.) -> ()");
  m.def("spmm_sliced_raw(Tensor segptr, Tensor indices, Tensor? vals, Tensor? eid, Tensor? keep, Tensor X, Tensor? src_scale, "
        "Tensor? dst_scale, int n_dst, int n_slices, int act=0, float slope=0., Tensor? out_mask=None, float mask_scale=1., "
        "int column_passes=0, int id_mult=0) -> Tensor");
  m.def("spmm_sliced_out(Tensor segptr, Tensor indices, Tensor? vals, Tensor? eid, Tensor? keep, Tensor X, Tensor? src_scale, "
        "Tensor? dst_scale, int n_dst, int n_slices, Tensor(a!) out, int act=0, float slope=0., Tensor? out_mask=None, "
        "float mask_scale=1., int column_passes=0, int id_mult=0) -> ()");
  m.def("rows_to_bf16(Tensor X, Tensor? scale=None) -> Tensor");
  m.def("spmm_sliced_bf16_raw(Tensor segptr, Tensor indices, Tensor? vals, Tensor? eid, Tensor? keep, Tensor X, Tensor? dst_scale, "
        "int n_dst, int n_slices, int act=0, float slope=0., Tensor? out_mask=None, float mask_scale=1., int column_passes=0, "
        "int id_mult=0) -> Tensor");
  m.def("spmm_sliced_bf16_out(Tensor segptr, Tensor indices, Tensor? vals, Tensor? eid, Tensor? keep, Tensor X, Tensor? dst_scale, "
        "int n_dst, int n_slices, Tensor(a!) out, int act=0, float slope=0., Tensor? out_mask=None, float mask_scale=1., "
        "int column_passes=0, int id_mult=0) -> ()");
  m.def("epilogue_backward(Tensor dY, Tensor Y, Tensor? mask, int act, float slope, float mask_scale) -> Tensor");
  m.def("knn_cosine_topk(Tensor Xn, int k) -> Tensor");
  m.def("pair_mlp_topk(Tensor P, Tensor Q, Tensor W2, Tensor b2, Tensor w3, Tensor b3, Tensor? known_drug, Tensor? known_dis, "
        "int k) -> (Tensor, Tensor, Tensor, Tensor)");
  m.def("pair_mlp_row_topk(Tensor X, Tensor C, Tensor W2, Tensor b2, Tensor w3, Tensor b3, Tensor? known_query, "
        "Tensor? known_cand, int k) -> (Tensor cand, Tensor logit, Tensor count, Tensor info)");
  m.def("pair_mlp_score_list(Tensor X, Tensor C, Tensor W2, Tensor b2, Tensor w3, Tensor b3, Tensor pair_query, "
        "Tensor pair_cand) -> (Tensor logit, Tensor info)");
  m.def("pair_mlp_rank_list(Tensor X, Tensor C, Tensor W2, Tensor b2, Tensor w3, Tensor b3, Tensor pair_query, "
        "Tensor pair_cand, Tensor? known_query, Tensor? known_cand) -> (Tensor logit, Tensor above, Tensor total, Tensor info)");
  m.def("pair_mlp_emit(Tensor P, Tensor Q, Tensor W2, Tensor b2, Tensor w3, Tensor b3, Tensor? known_drug, Tensor? known_dis, "
        "float min_logit, Tensor(a!) out_drug, Tensor(b!) out_dis, Tensor(c!) out_logit) -> (Tensor count, Tensor info)");
  m.def("pair_records_sort(Tensor(a!) drug, Tensor(b!) dis, Tensor(c!) logit, int n) -> ()");
  m.def("scale_rows(Tensor X, Tensor scale) -> Tensor");
  m.def("colsum_rows_(Tensor(a!) feat_ext, Tensor coef, int n, int R, int i0) -> ()");
  m.def("colsum_rows_backward_(Tensor(a!) gf, Tensor coef, Tensor gs, int n, int R, int i0) -> ()");
  m.def("gather_f32(Tensor values, Tensor perm) -> Tensor");
  m.def("gather_concat_raw(Tensor src, Tensor dst, Tensor A, Tensor B) -> Tensor");
  m.def("gather_add_raw(Tensor src, Tensor dst, Tensor A, Tensor B, Tensor? bias, int act=0) -> Tensor");
  m.def("random_subset_select(Tensor like, int E, int keep, int seed, int e_offset=0) -> Tensor");
  m.def("random_subset_select_batch(Tensor like, int[] E, int[] keep, int[] seed, int[] e_offset) -> Tensor");
  m.def("random_subset_select_batch_dseed(Tensor seeds, int[] E, int[] keep, int[] e_offset) -> Tensor");
  m.def("keep_mask(Tensor keep, int E) -> Tensor");
  m.def("row_multiplicity(Tensor indptr, Tensor vals, float rel_tol) -> (Tensor, Tensor, Tensor)");
  m.def("compact_layout(Tensor ptr, Tensor indices, Tensor? vals, Tensor eid, Tensor keep) -> (Tensor, Tensor, Tensor)");
}

// ROCm builds of torch dispatch HIP tensors under the CUDA key
TORCH_LIBRARY_IMPL(dreamgnn_mi, CUDA, m) {
  m.impl("csr_from_coo", csr_from_coo);
  m.impl("csr_sliced_from_coo", csr_sliced_from_coo);
  m.impl("csr_sliced_from_csr", csr_sliced_from_csr);
  m.impl("plan_build", plan_build);
  m.impl("spmm_csr", spmm_csr_forward);
  m.impl("spmm_csr_raw", spmm_csr_new);
  m.impl("spmm_csr_out", spmm_csr_out);
  m.impl("spmm_sliced_raw", spmm_sliced_new);
  m.impl("spmm_sliced_out", spmm_sliced_out);
  m.impl("rows_to_bf16", rows_to_bf16);
  m.impl("spmm_sliced_bf16_raw", spmm_sliced_bf16_new);
  m.impl("spmm_sliced_bf16_out", spmm_sliced_bf16_out);
  m.impl("epilogue_backward", epilogue_backward);
  m.impl("knn_cosine_topk", knn_cosine_topk);
  m.impl("pair_mlp_topk", pair_mlp_topk);
  m.impl("pair_mlp_row_topk", pair_mlp_row_topk);
  m.impl("pair_mlp_score_list", pair_mlp_score_list);
  m.impl("pair_mlp_rank_list", pair_mlp_rank_list);
  m.impl("pair_mlp_emit", pair_mlp_emit);
  m.impl("pair_records_sort", pair_records_sort);
  m.impl("scale_rows", scale_rows);
  m.impl("colsum_rows_", colsum_rows_);
  m.impl("colsum_rows_backward_", colsum_rows_backward_);
  m.impl("gather_f32", gather_f32);
  m.impl("gather_concat_raw", gather_concat_raw);
  m.impl("gather_add_raw", gather_add_raw);
  m.impl("random_subset_select", random_subset_select);
  m.impl("random_subset_select_batch", random_subset_select_batch);
  m.impl("random_subset_select_batch_dseed", random_subset_select_batch_dseed);
  m.impl("keep_mask", keep_mask);
  m.impl("row_multiplicity", row_multiplicity);
  m.impl("compact_layout", compact_layout);
}

TORCH_LIBRARY_IMPL(dreamgnn_mi, Autograd, m) { m.impl("spmm_csr", spmm_csr_autograd); }

// The evaluation metrics, registered as a fragment of their own: curve_areas reads scores and writes statistics, it
// is no operand of a product, so its operand forms are tested with its arithmetic (tests/test_gpu_curve.py) and not in
// the binding case table, which holds one case per op of the block above (tests/_binding_cases.py).
TORCH_LIBRARY_FRAGMENT(dreamgnn_mi, train) {
  train.def("pair_mlp_train_forward(Tensor X, Tensor C, Tensor W2, Tensor b2, Tensor w3, Tensor b3, Tensor pair_query, "
            "Tensor pair_cand, float p, Tensor seed) -> (Tensor, Tensor)");
  train.def("pair_mlp_train_backward(Tensor X, Tensor C, Tensor W2, Tensor b2, Tensor w3, Tensor b3, Tensor pair_query, "
            "Tensor pair_cand, float p, Tensor seed, Tensor dlogit) -> (Tensor, Tensor, Tensor, Tensor, Tensor, Tensor)");
}

TORCH_LIBRARY_IMPL(dreamgnn_mi, CUDA, train) {
  train.impl("pair_mlp_train_forward", pair_mlp_train_forward);
  train.impl("pair_mlp_train_backward", pair_mlp_train_backward);
}

TORCH_LIBRARY_FRAGMENT(dreamgnn_mi, attn) {
  attn.def("attn_fuse_forward(Tensor A, Tensor B, Tensor? M, Tensor W1, Tensor b1, Tensor w2) -> (Tensor, Tensor)");
  attn.def("attn_fuse_backward(Tensor A, Tensor B, Tensor? M, Tensor W1, Tensor b1, Tensor w2, Tensor dout) -> (Tensor, Tensor, Tensor, Tensor, Tensor)");
}

TORCH_LIBRARY_IMPL(dreamgnn_mi, CUDA, attn) {
  attn.impl("attn_fuse_forward", attn_fuse_forward);
  attn.impl("attn_fuse_backward", attn_fuse_backward);
}

TORCH_LIBRARY_FRAGMENT(dreamgnn_mi, metrics) {
  metrics.def("curve_areas(Tensor score, Tensor label, Tensor? segment, int n_segments, float threshold) -> (Tensor count, Tensor area, Tensor info)");
}
TORCH_LIBRARY_IMPL(dreamgnn_mi, CUDA, metrics) { metrics.impl("curve_areas", curve_areas); }
