/*
 * dgmi_attn.h — C ABI of libdgmi.so, part 10: the two-channel attention fusion of the encoder (the harness's
 * model.Attention) in TRAINING: the weighted sum of two embedding tables in one kernel, every gradient from a recompute,
 * nothing of size n_rows x 2 x F kept between the two.
 *
 * Same conventions as dgmi.h / dgmi_train.h: device pointers, asynchronous on `stream`, never synchronises, allocates
 * nothing (capturable), returns DGMI_OK or a negative dgmi_status.
 */
#ifndef DGMI_ATTN_H_
#define DGMI_ATTN_H_

#include "dgmi.h"

#ifdef __cplusplus
extern "C" {
#endif

/* rows of one block (a workgroup takes blocks b, b + grid, ...) and the largest grid of the row launches */
#define DGMI_ATTN_BLOCK_ROWS 64
#define DGMI_ATTN_MAX_WORKGROUPS 1024

/* -------------------------------------------------------------------------
 * One call = one node type.  Operands, all fp32: A, B (n_rows, F) with leading dimensions lda / ldb, W1 (H, F) row-major,
 * b1 and w2 H floats, M an optional (n_rows, 2) contiguous multiplier (NULL: all ones; the caller's dropout factors).
 * Only H = 16 is taken; F % 4 == 0, 4 <= F <= 512; 0 <= n_rows <= 2^31 - 1.
 *
 * With z_0 = A[n], z_1 = B[n]:
 *   h_c = tanh(b1 + W1 z_c),  s_c = w2 . h_c,  beta = softmax(s_0, s_1),  beta'_c = beta_c * M[n, c]  (a product)
 *   out[n] = beta'_0 z_0 + beta'_1 z_1   (n_rows, F), leading dimension ldo
 *   out_beta[n] = (beta'_0, beta'_1)     (n_rows, 2) contiguous
 *
 * dgmi_attn_fuse_backward_f32: given the forward's operands and dout = dLoss / dout (leading dimension ldg), with
 *   dbeta'_c = dout[n] . z_c,  dbeta_c = M_c dbeta'_c,  ds_c = beta_c (dbeta_c - sum_k beta_k dbeta_k),
 *   dpre_c = ds_c w2 (1 - h_c^2):
 *   out_dA[n] = beta'_0 dout[n] + W1^T dpre_0,  out_dB[n] = beta'_1 dout[n] + W1^T dpre_1   (leading dimensions ld_da, ld_db)
 *   out_dW1 (H, F) = sum_{n, c} dpre_c z_c^T,  out_db1 (H) = sum_{n, c} dpre_c,  out_dw2 (H) = sum_{n, c} ds_c h_c.
 * M is a constant and out_beta gets no gradient.  The backward recomputes h and beta with the forward's instructions.
 * Non-finite operands follow IEEE: a NaN in row n reaches row n of the row outputs and the three sums, nothing else.
 *
 * Sums: block b of DGMI_ATTN_BLOCK_ROWS rows belongs to workgroup b mod grid, grid = min(blocks, DGMI_ATTN_MAX_WORKGROUPS);
 * a workgroup adds its blocks in order and writes one partial of (H F + 2 H) floats to the workspace, and one small
 * kernel adds the partials in workgroup order.  No float atomics: the same bits from run to run, the order a function of
 * n_rows and F alone.
 *
 * Errors, returned before any launch: DGMI_ERR_INVALID_ARG for a null pointer other than M, H != 16, F outside the range
 * above, a leading dimension below F or not a multiple of 4, a table pointer (A, B, W1, dout, out, out_dA, out_dB) not
 * 16-byte aligned, out overlapping A or B, n_rows negative or beyond int32; DGMI_ERR_WORKSPACE (backward only) for a
 * workspace below dgmi_attn_fuse_workspace_bytes(n_rows, F).  n_rows = 0 returns DGMI_OK: the forward writes nothing, the
 * backward writes zeros to out_dW1 / out_db1 / out_dw2 and needs no workspace; an empty call excuses no bad argument.
 * The workspace size is a multiple of 256, monotone in n_rows, and 0 for n_rows <= 0 or beyond int32 or a bad F.
 * ------------------------------------------------------------------------- */
DGMI_API size_t dgmi_attn_fuse_workspace_bytes(int64_t n_rows, int32_t F);
DGMI_API int dgmi_attn_fuse_forward_f32(const float* A, int64_t lda, const float* B, int64_t ldb, int64_t n_rows, int32_t F,
                                        int32_t H, const float* W1, const float* b1, const float* w2, const float* M,
                                        float* out, int64_t ldo, float* out_beta, dgmi_stream_t stream);
DGMI_API int dgmi_attn_fuse_backward_f32(const float* A, int64_t lda, const float* B, int64_t ldb, int64_t n_rows, int32_t F,
                                         int32_t H, const float* W1, const float* b1, const float* w2, const float* M,
                                         const float* dout, int64_t ldg, float* out_dA, int64_t ld_da, float* out_dB,
                                         int64_t ld_db, float* out_dW1, float* out_db1, float* out_dw2, void* workspace,
                                         size_t workspace_bytes, dgmi_stream_t stream);

#ifdef __cplusplus
}
#endif

#endif /* DGMI_ATTN_H_ */
