/* mumpy_hip_ext2.h — entry points of libmumpy_hip.so added after the surfaces of mumpy_hip.h (MUMPY_ABI_VERSION 2) and
 * mumpy_hip_ext.h (MUMPY_EXT_VERSION 1) were frozen.
 *
 * The conventions are those of mumpy_hip.h: plain C, raw DEVICE pointers + sizes + `void* stream` last, the CALLER allocates and
 * owns every buffer, nothing here allocates or synchronises (every launching call may be captured into a hipGraph), 0 on success, a
 * negative MUMPY_E* code for a rejected argument (nothing is launched), a positive hipError_t for a failed launch, the message in
 * mumpy_last_error().  This header has a version of its own; it grows by appending.
 */
#ifndef MUMPY_HIP_EXT2_H
#define MUMPY_HIP_EXT2_H

#include "mumpy_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define MUMPY_EXT2_VERSION 2
int mumpy_ext2_version(void);

/* ---- backward of the cross-view attention core on the bf16 MFMA: the pair of mumpy_deform_attention_mm16_fwd ----
 * Window form, fp32 in memory: q (B1w,49,C), kv (B1w*r,49,2C) = [k | v] per row, dout (B1w,49,C) -> dq (B1w,49,C), dkv (B1w*r,49,2C).
 * kv window b2 pairs with q window b2 % B1w and with dout of output window b2 / r.  With r(x) = round to nearest even to bf16 and
 * everything else fp32 (products on v_mfma_f32_32x32x16_bf16, fp32 accumulation):
 *   S = scale (r(q) r(k)^T),  P = softmax(S) over the 49 keys,  dP = r(dout) r(v)^T,  D = rowsum(P o dP),  dS = P o (dP - D)
 *   dv = r(P)^T r(dout),  dk = scale r(dS)^T r(q),
 *   dq[qw] = sum over m = 0 .. r-1, in that order, of scale r(dS_b2) r(k_b2),  b2 = qw + m B1w
 * dq is FINAL (unlike dq_part of mumpy_deform_attention_bwd: the r members are summed on the device in that fixed order, so the result
 * is deterministic); every element of dq and dkv is written; q, kv and dout are only read.
 * workspace: DEVICE, mumpy_deform_attention_mm16_bwd_workspace_bytes(B1w, r, C) bytes (0 for a shape the entry refuses), its contents
 * need not be initialised.  All six pointers required and 16-byte aligned (MUMPY_ENULL / MUMPY_EALIGN).  B1w > 0, r >= 1, C > 0 and
 * C % 32 == 0, workspace_bytes at least the query's value (MUMPY_EINVAL).  MUMPY_ERANGE: B1w * r >= 2^31, a grid of 2^31 blocks or
 * more, or 49 * 2C * 4 >= 2^32 (a row's byte offset inside a kv window is formed in 32 bits). */
int64_t mumpy_deform_attention_mm16_bwd_workspace_bytes(int64_t B1w, int r, int C);
int mumpy_deform_attention_mm16_bwd(const float* q, const float* kv, const float* dout, float* dq, float* dkv, void* workspace,
                                    int64_t workspace_bytes, int64_t B1w, int r, int C, float scale, void* stream);

/* ---- (version 2) the MLP of a transformer block on the training tape: fc1 with two outputs, fc2's backward with the GELU derivative ----
 * mumpy_linear_gelu_dual_fwd: z (M,N) = x (M,K) W (N,K)^T + bias and a (M,N) = gelu_erf(z) from ONE launch (+ the split-K combine where
 * the plan splits): the plan, the kernels and the epilogue arithmetic of mumpy_linear_wsz_fwd with act = MUMPY_ACT_GELU | math, whose
 * epilogue stores its value a second time, before the activation.  a is bit for bit what that call writes, z what the call without the
 * activation writes on the same route.  Both fp32; every element of both is written; x, W and bias are only read; bias may be null.
 * math: 0 or MUMPY_MATH_BF16 (operands rounded to bf16 while staged); anything else -- the split-precision modes included -- is
 * MUMPY_EINVAL.  workspace: null, or the KEPT workspace of mumpy_linear_wsz_fwd (first 4096 bytes zero on entry, left zero), at least
 * mumpy_linear_workspace_bytes(M, N, K) bytes (smaller: MUMPY_EINVAL).  x, W, z, a required (MUMPY_ENULL), all pointers 16-byte aligned
 * (MUMPY_EALIGN), K % 32 == 0, N % 32 == 0 (MUMPY_EINVAL), z != a (MUMPY_EINVAL); the ranges of mumpy_linear_fwd (MUMPY_ERANGE).
 *
 * mumpy_linear_gelu_bwd: the backward of y (M,N) = a W^T + b for a (M,K) = gelu_erf(z): mumpy_linear_bwd with x = a, except that the
 * input gradient is taken through the activation in the same launches,  dz (M,K) = (dy W) o gelu'(z)  -- where the dX product is
 * stored when it ran unsplit, in the one reduce launch, after the fixed-order sum, when it ran split (bitwise reproducible either way).
 * dW (N,K) (+)= dy^T a and db (N) (+)= column sums of dy are those of mumpy_linear_bwd.  accumulate, workspace
 * (mumpy_linear_gelu_bwd_workspace_bytes = mumpy_linear_bwd_workspace_bytes) and the M / N % 32 / K % 32 limits: as there.
 * dy and one of dz / dW / db required; dz needs z and W, dW needs a (MUMPY_ENULL).  MUMPY_EINVAL as well for z == a and for a dz that
 * overlaps z, a or dy.  Every element of dz is written; a, z, W and dy are only read. */
int mumpy_linear_gelu_dual_fwd(const float* x, const float* W, const float* bias, float* z, float* a, int64_t M, int N, int K, int math,
                               void* workspace, int64_t workspace_bytes, void* stream);
int64_t mumpy_linear_gelu_bwd_workspace_bytes(int64_t M, int N, int K);
int mumpy_linear_gelu_bwd(const float* a, const float* z, const float* W, const float* dy, float* dz, float* dW, float* db, int64_t M,
                          int N, int K, int accumulate, void* workspace, int64_t workspace_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* MUMPY_HIP_EXT2_H */
