/* mumpy_hip_ext8.h — entry points of libmumpy_hip.so added after the surfaces of mumpy_hip.h (MUMPY_ABI_VERSION 2), mumpy_hip_ext.h
 * (MUMPY_EXT_VERSION 1), mumpy_hip_ext2.h (MUMPY_EXT2_VERSION 2), mumpy_hip_ext3.h (MUMPY_EXT3_VERSION 1), mumpy_hip_ext4.h
 * (MUMPY_EXT4_VERSION 1), mumpy_hip_ext5.h (MUMPY_EXT5_VERSION 1), mumpy_hip_ext6.h (MUMPY_EXT6_VERSION 1) and mumpy_hip_ext7.h
 * (MUMPY_EXT7_VERSION 1) were frozen.  No name lives in two headers.
 *
 * The conventions are those of mumpy_hip.h: plain C, raw DEVICE pointers + sizes + `void* stream` last, the CALLER allocates and
 * owns every buffer, nothing here allocates or synchronises (every launching call may be captured into a hipGraph), 0 on success, a
 * negative MUMPY_E* code for a rejected argument (nothing is launched), a positive hipError_t for a failed launch, the message in
 * mumpy_last_error().  This header has a version of its own.
 *
 * GROUPED PAIRING of the cross-view attention (SwinDAttention).  The reference pairs kv window i with q window i mod nq
 * (`x1.repeat`, deform:330) and sums adjacent r-tuples of kv windows into output window i / r (deform:394-395), where nq counts the
 * q windows of EVERY sample of the batch: what a sample's windows attend with depends on the batch it travels in.  The frozen
 * entries (mumpy_deform_sample_fwd, mumpy_deform_sample_kv[_mm16]_fwd, mumpy_deform_attention[_mm16]_fwd) reproduce that.  The five
 * entries here take one more argument, `int groups` (G), and apply the reference's rule inside each of G equal, contiguous groups:
 * with nq q windows and nkv = r nq kv windows in the launch and nqg = nq / G,
 *
 *     g = i / (r nqg)        q(i) = g nqg + ((i - g r nqg) mod nqg)        out(i) = i / r
 *
 * G = 1 is the frozen entry (the same kernel instantiation is launched: the same bits).  G = B is PER-SAMPLE pairing: every sample of
 * the batch pairs as the reference pairs a batch of one, so a grouped launch on a batch equals the frozen entry on each sample's slice,
 * concatenated -- bit for bit, every kernel computes a window from the same values in the same order whatever the launch holds.
 * For r = 1 the grouped and the frozen rule coincide (q(i) = i).
 *
 * Everything else -- layouts, alignment, ranges, what is read and written -- is the frozen sibling's, documented in mumpy_hip.h.
 * Every entry refuses, before anything is launched:
 *   MUMPY_EINVAL: groups < 1; groups does not divide nq; groups does not divide B; (groups > 1) nq does not divide nkv;
 *   and whatever its sibling refuses, with the sibling's code.
 *
 * The plan of the fp32 attention core does not depend on the grouping: mumpy_deform_attention_plan(B, H, W, C, r) holds for
 * mumpy_deform_attention_grouped_fwd at every G (the form is a function of the unit count B (H/7) (W/7) (C/32) alone).
 */
#ifndef MUMPY_HIP_EXT8_H
#define MUMPY_HIP_EXT8_H

#include "mumpy_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define MUMPY_EXT8_VERSION 1
int mumpy_ext8_version(void);

/* mumpy_deform_sample_fwd with grouped pairing: out[i] = x2 window i sampled at pos[q(i)].  nq q windows (pos is (nq, 3, 49, 2)),
 * nkv = B (Hs2/7) (W/7) kv windows. */
int mumpy_deform_sample_grouped_fwd(const float* x2, const float* pos, float* out, int B, int Hs2, int W, int C, int nq, int groups,
                                    void* stream);

/* mumpy_deform_sample_kv_fwd / mumpy_deform_sample_kv_mm16_fwd with grouped pairing: kv[i] = [proj_k | proj_v] of x2 window i
 * sampled at pos[q(i)]. */
int mumpy_deform_sample_kv_grouped_fwd(const float* x2, const float* pos, const float* Wkv, const float* bkv, float* kv, int B,
                                       int Hs2, int W, int C, int nq, int groups, void* stream);
int mumpy_deform_sample_kv_mm16_grouped_fwd(const float* x2, const float* pos, const float* Wkv, const float* bkv, float* kv, int B,
                                            int Hs2, int W, int C, int nq, int groups, void* stream);

/* mumpy_deform_attention_fwd / mumpy_deform_attention_mm16_fwd with grouped pairing: output window b1 sums, in the order
 * t = 0 .. r-1, the attention of q window q(b1 r + t) over kv window b1 r + t.  nq = B (H/7) (W/7), nkv = r nq. */
int mumpy_deform_attention_grouped_fwd(const float* q, const float* kv, const float* padmask, float* out, int B, int H, int W, int C,
                                       int r, float scale, int groups, void* stream);
int mumpy_deform_attention_mm16_grouped_fwd(const float* q, const float* kv, const float* padmask, float* out, int B, int H, int W,
                                            int C, int r, float scale, int groups, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* MUMPY_HIP_EXT8_H */
