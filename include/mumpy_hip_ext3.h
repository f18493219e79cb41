/* mumpy_hip_ext3.h — entry points of libmumpy_hip.so added after the surfaces of mumpy_hip.h (MUMPY_ABI_VERSION 2), mumpy_hip_ext.h
 * (MUMPY_EXT_VERSION 1) and mumpy_hip_ext2.h (MUMPY_EXT2_VERSION 2) were frozen.  No name lives in two headers.
 *
 * The conventions are those of mumpy_hip.h: plain C, raw DEVICE pointers + sizes + `void* stream` last, the CALLER allocates and
 * owns every buffer, nothing here allocates or synchronises (every launching call may be captured into a hipGraph), 0 on success, a
 * negative MUMPY_E* code for a rejected argument (nothing is launched), a positive hipError_t for a failed launch, the message in
 * mumpy_last_error().  This header has a version of its own; it is the one that grows from here on, by appending.
 */
#ifndef MUMPY_HIP_EXT3_H
#define MUMPY_HIP_EXT3_H

#include "mumpy_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define MUMPY_EXT3_VERSION 1
int mumpy_ext3_version(void);

/* ---- the training input stage: uint8 clips -> augmented, normalized fp32 clips and 0/1 targets, one call ----
 * The loader's resize (PIL NEAREST), the reference's enabled augmentations (the dihedral group of the square canvas: flips, 90-degree
 * rotations; crop boxes followed by a NEAREST resize back), ToTensor + Normalize + HWC -> CHW, and the target construction
 * (sequence_from_masks: mask > 0) are all index permutations followed by the arithmetic of mumpy_normalize_u8_fwd.  They fold into two
 * per-clip index tables of L entries and one swap word (built on the host: mumpy_hip/augment.py, clip_tables).
 *
 *   frames (nclips*T, Hs, Ws, 3) uint8          -> out    (nclips*T, 3, L, L) fp32
 *   masks  (nmasks, Hs, Ws) uint8  (optional)   -> target (nclips, L*L) fp32     (optional; given together or both null)
 *   tab_a, tab_b (nclips, L) int32 and swap (nclips) int32: DEVICE memory, read by the kernel when it RUNS -- a captured launch replays
 *   with whatever parameters were uploaded last.  mean3 / std3: HOST arrays of 3, read at the call (as in mumpy_normalize_u8_fwd).
 *
 * For clip c, frame t, output pixel (y, x):
 *   i  = swap[c] & 1 ? x : y              j  = swap[c] & 1 ? y : x
 *   sy = clamp(tab_a[c][i], 0, Hs - 1)    sx = clamp(tab_b[c][j], 0, Ws - 1)
 *   out[c*T + t, ch, y, x] = ((float)frames[c*T + t, sy, sx, ch] / 255.0f - mean[ch]) / std[ch]
 *       (the expression of mumpy_normalize_u8_fwd / mumpy_resize_normalize_u8_fwd in the same order: results compare bitwise)
 *   target[c, y*L + x]     = masks[c % nmasks, sy, sx] > 0 ? 1.0f : 0.0f
 *       (clip c reads mask c % nmasks: the reference's cat([masks] * 3) over the sequences of a sample)
 * The tables cannot be validated on the host, so the clamp and the `& 1` are part of the contract: NO table or swap content makes the
 * kernel read outside frames / masks.  Every element of out (and of target, when given) is written; frames, masks, the tables and
 * swap are only read.  One launch.
 *
 * MUMPY_ENULL: frames, out, tab_a, tab_b, swap, mean3 or std3 null; exactly one of masks / target given.
 * MUMPY_EINVAL: T < 1, Hs < 1, Ws < 1, L < 4 or L % 4 != 0; nclips < 0 (nclips == 0 is an accepted no-op: returns 0, launches nothing);
 *   with masks, nmasks < 1 or nclips % nmasks != 0 (without masks nmasks is ignored); a zero std.
 * MUMPY_EALIGN: out, target, tab_a or tab_b not 16-byte aligned (16-byte stores, 16-byte table loads; L % 4 == 0 keeps every row so).
 * MUMPY_ERANGE: nclips * T >= 2^31 (the frame index); 3 * Hs * Ws >= 2^31 (a byte offset inside one frame is formed in 32 bits);
 *   3 * L * L >= 2^31 (with the frame bound this keeps every element count below 2^62; all other offsets are 64-bit).  The grid is
 *   capped (grid-stride loop), so it sets no limit. */
int mumpy_augment_stage_u8_fwd(const uint8_t* frames, const uint8_t* masks, float* out, float* target,
                               const int32_t* tab_a, const int32_t* tab_b, const int32_t* swap,
                               int64_t nclips, int T, int64_t nmasks, int Hs, int Ws, int L,
                               const float* mean3, const float* std3, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* MUMPY_HIP_EXT3_H */
