/* mumpy_hip_ext9.h — entry points of libmumpy_hip.so added after the surfaces of mumpy_hip.h (MUMPY_ABI_VERSION 2), mumpy_hip_ext.h
 * (MUMPY_EXT_VERSION 1), mumpy_hip_ext2.h (MUMPY_EXT2_VERSION 2), mumpy_hip_ext3.h (MUMPY_EXT3_VERSION 1), mumpy_hip_ext4.h
 * (MUMPY_EXT4_VERSION 1), mumpy_hip_ext5.h (MUMPY_EXT5_VERSION 1), mumpy_hip_ext6.h (MUMPY_EXT6_VERSION 1), mumpy_hip_ext7.h
 * (MUMPY_EXT7_VERSION 1) and mumpy_hip_ext8.h (MUMPY_EXT8_VERSION 1) were frozen.  No name lives in two headers.
 *
 * The conventions are those of mumpy_hip.h: plain C, raw DEVICE pointers + sizes + `void* stream` last, the CALLER allocates and
 * owns every buffer, nothing here allocates or synchronises (every launching call may be captured into a hipGraph), 0 on success, a
 * negative MUMPY_E* code for a rejected argument (nothing is launched), a positive hipError_t for a failed launch, the message in
 * mumpy_last_error().  This header has a version of its own.
 *
 * GROUPED PAIRING IN THE BACKWARD of the cross-view attention (SwinDAttention): the training half of mumpy_hip_ext8.h, whose
 * comment states the rule.  With nq q windows and nkv = r nq kv windows in the launch, G = groups and nqg = nq / G,
 *
 *     g = i / (r nqg)        q(i) = g nqg + ((i - g r nqg) mod nqg)        out(i) = i / r
 *     kv windows of q window qw, in the order their contributions are summed:  (qw / nqg) r nqg + (qw mod nqg) + m nqg,  m = 0 .. r-1
 *
 * G = 1 is the frozen entry (the same kernel instantiations are launched: the same bits).  With G equal to the number of clips every
 * clip is differentiated as the reference differentiates a batch of one: a grouped launch on a batch equals the frozen entry on each
 * clip's slice, concatenated -- bit for bit, every kernel computes a window from the same values in the same order whatever the
 * launch holds.  For r = 1 the grouped and the frozen rule coincide.  These entries take window counts and no batch size: a group is
 * nq / G q windows with their r nq / G kv windows.
 *
 * Everything else -- layouts, alignment, ranges, workspaces, what is read and written -- is the frozen sibling's, documented in
 * mumpy_hip.h and mumpy_hip_ext2.h.  Every entry refuses, before anything is launched:
 *   MUMPY_EINVAL: groups < 1; groups does not divide nq; (groups > 1) nq does not divide nkv;
 *   and whatever its sibling refuses, with the sibling's code.
 */
#ifndef MUMPY_HIP_EXT9_H
#define MUMPY_HIP_EXT9_H

#include "mumpy_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define MUMPY_EXT9_VERSION 1
int mumpy_ext9_version(void);

/* mumpy_deform_sample_bwd with grouped pairing: kv window i reads pos[q(i)].  dpos_part stays one slot per kv window, (B2, 3, 49, 2):
 * the caller sums the r slots of a q window (slots (qw / nqg) r nqg + (qw mod nqg) + m nqg). */
int mumpy_deform_sample_grouped_bwd(const float* x2, const float* pos, const float* dsampled, float* dx2, float* dpos_part,
                                    int64_t B2, int C, int nq, int groups, void* stream);

/* mumpy_deform_attention_bwd with grouped pairing: kv window i meets q window q(i) and the dout of output window i / r.  dq_part stays
 * one slot per kv window, (B1w r, 49, C), summed by the caller as above.  Workspace: mumpy_deform_attention_bwd_workspace_bytes. */
int mumpy_deform_attention_grouped_bwd(const float* q, const float* kv, const float* dout, float* dq_part, float* dkv,
                                       void* workspace, int64_t workspace_bytes, int64_t B1w, int r, int C, float scale, int groups,
                                       void* stream);

/* mumpy_deform_attention_mm16_bwd with grouped pairing: dq comes out final, each q window's r contributions summed on the device in
 * the order m = 0 .. r-1 above.  Workspace: mumpy_deform_attention_mm16_bwd_workspace_bytes. */
int mumpy_deform_attention_mm16_grouped_bwd(const float* q, const float* kv, const float* dout, float* dq, float* dkv,
                                            void* workspace, int64_t workspace_bytes, int64_t B1w, int r, int C, float scale,
                                            int groups, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* MUMPY_HIP_EXT9_H */
