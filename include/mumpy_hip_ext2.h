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

#define MUMPY_EXT2_VERSION 1
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

#ifdef __cplusplus
}
#endif
#endif /* MUMPY_HIP_EXT2_H */
