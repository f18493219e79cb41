/* mumpy_hip_ext5.h — entry points of libmumpy_hip.so added after the surfaces of mumpy_hip.h (MUMPY_ABI_VERSION 2), mumpy_hip_ext.h
 * (MUMPY_EXT_VERSION 1), mumpy_hip_ext2.h (MUMPY_EXT2_VERSION 2), mumpy_hip_ext3.h (MUMPY_EXT3_VERSION 1) and mumpy_hip_ext4.h
 * (MUMPY_EXT4_VERSION 1) were frozen.  No name lives in two headers.
 *
 * The conventions are those of mumpy_hip.h: plain C, raw DEVICE pointers + sizes + `void* stream` last, the CALLER allocates and
 * owns every buffer, nothing here allocates or synchronises (every launching call may be captured into a hipGraph), 0 on success, a
 * negative MUMPY_E* code for a rejected argument (nothing is launched), a positive hipError_t for a failed launch, the message in
 * mumpy_last_error().  This header has a version of its own.
 *
 * These three are the device side of whole-video inference (mumpy_hip/video.py): the reference builds one clip per frame -- the frame
 * and its T // 2 neighbours on each side, clamped at the ends (dataloaders/universaldataloader.py:41-48) --, keeps the centre frame's
 * mask, writes mask * 255 (test.py:86-111) and scores every frame with the per-image F1 / IoU of measure.py:57-62, 86-89.
 */
#ifndef MUMPY_HIP_EXT5_H
#define MUMPY_HIP_EXT5_H

#include "mumpy_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define MUMPY_EXT5_VERSION 1
int mumpy_ext5_version(void);

/* ---- sliding clips out of a video that is resident on the device: gather + resize + ToTensor + Normalize in one launch ----
 *   frames (nframes, Hs, Ws, 3) uint8: the video.   frame_idx (nclips, T) int32: the source frame of every clip frame.
 *   out (nclips, T, 3, H, W) float32.   ytab (H) / xtab (W) int32, mean3 / std3 (HOST arrays of 3, read at the call): exactly as in
 *   mumpy_resize_normalize_u8_fwd (mumpy_resize_nearest_table builds the tables; identity tables give the plain staging).
 *   frames, frame_idx, ytab and xtab are DEVICE memory, read by the kernel when it RUNS: a captured launch replays with what was
 *   uploaded last.
 *
 *   out[c, t] = what mumpy_resize_normalize_u8_fwd writes for source frame clamp(frame_idx[c][t], 0, nframes - 1), bit for bit (the
 *   two kernels share the pixel expression: csrc/u8_pixel.h).
 * The clamp is part of the contract: NO content of frame_idx makes the kernel read outside frames (ytab / xtab entries are clamped to
 * the source frame as well).  Every element of out is written; all inputs are only read.
 *
 * MUMPY_ENULL: frames, out, frame_idx, ytab, xtab, mean3 or std3 null.
 * MUMPY_EINVAL: nframes < 1, T < 1, Hs < 1, Ws < 1, H < 1, W < 1 or W % 4 != 0; nclips < 0 (nclips == 0 is an accepted no-op: returns
 *   0, launches nothing); a zero std.
 * MUMPY_EALIGN: out or xtab not 16-byte aligned (16-byte stores and loads; W % 4 == 0 keeps every row so).
 * MUMPY_ERANGE: nframes >= 2^31 (frame_idx is 32-bit); nclips * T >= 2^31; 3 * Hs * Ws >= 2^31; 3 * H * W >= 2^31 (offsets inside a
 *   frame are 32-bit). */
int mumpy_clip_window_u8_fwd(const uint8_t* frames, float* out, const int32_t* frame_idx, const int32_t* ytab, const int32_t* xtab,
                             int64_t nclips, int T, int64_t nframes, int Hs, int Ws, int H, int W, const float* mean3,
                             const float* std3, void* stream);

/* ---- the masks of a batch of clips into the per-frame mask bank, and the four counts the metrics need ----
 *   mask (nclips, npix) uint8: the 0 / non-0 mask mumpy_final_conv_fwd emits (Decoder.predict_mask).
 *   dest (nclips) int32, DEVICE memory read when the kernel runs: the frame each clip's mask belongs to.
 *   bank (nbank, npix) uint8: the per-frame masks.   gt (nbank, npix) uint8, or NULL: the per-frame annotations.
 *   counts (nbank, 4) int32, NULL exactly when gt is.
 * For clip c with 0 <= dest[c] < nbank:
 *   bank[dest[c]][i] = mask[c][i] ? 255 : 0                                  (the bytes test.py:109-111 saves)
 *   counts[dest[c]]  = {sum(p & g), sum(p), sum(g), sum(p | g)}              with p = mask[c][i] != 0, g = gt[dest[c]][i] > 0
 * A clip whose dest is outside [0, nbank) writes NOTHING: the padding clips of a batch tail carry -1.  Two clips with the same valid
 * dest in one call are the CALLER's error (both write the same rows; which one wins is not defined).  Rows of bank / counts that no
 * dest names are left as they are.  The counts are exact integers, written (not accumulated: counts need no zeroing), one workgroup
 * per clip with a fixed reduce and no atomics: the same input gives the same bits.  mask, dest and gt are only read.
 *
 * MUMPY_ENULL: mask, dest or bank null; exactly one of gt / counts given.
 * MUMPY_EINVAL: npix < 1 or npix % 16 != 0; nbank < 1; nclips < 0 (nclips == 0 is an accepted no-op).
 * MUMPY_EALIGN: mask, bank or gt not 16-byte aligned (16-byte loads and stores; npix % 16 == 0 keeps every row so).
 * MUMPY_ERANGE: nclips, nbank or npix >= 2^31 (dest and the counts are 32-bit). */
int mumpy_mask_score_u8_fwd(const uint8_t* mask, const uint8_t* gt, const int32_t* dest, uint8_t* bank, int32_t* counts,
                            int64_t nclips, int64_t npix, int64_t nbank, void* stream);

/* ---- per-frame F1 / IoU of the counts, summed over a video ----
 *   counts (>= nscored, 4) int32 as mumpy_mask_score_u8_fwd writes them: {inter, sum p, sum g, union} of frames 0 .. nscored - 1.
 *   acc3: double[3] in DEVICE memory = [sum F1, sum IoU, n], the layout mumpy_hip.evaluate.finalize_metrics all-reduces.
 * Per frame, in fp64 (measure.py:57-62, 86-89 as mumpy_hip.distributed.eval_metric_vector states them):
 *   recall = inter / (sum g + 1e-6 * npix),  precision = inter / (sum p + 1e-6),  F1 = 2 P R / (P + R + 1e-6),
 *   IoU = (inter + 1e-5) / (union + 1e-5)
 * acc3 = [sum F1, sum IoU, nscored] when accumulate == 0, else acc3 += that (one accumulator over the videos of a dataset).
 * nscored == 0 is accepted: it writes zeros, or adds nothing.  One workgroup, a fixed-order reduce: the same input gives the same bits.
 *
 * MUMPY_ENULL: counts or acc3 null.   MUMPY_EINVAL: nscored < 0, npix < 1.   MUMPY_EALIGN: acc3 not 8-byte aligned.
 * MUMPY_ERANGE: nscored or npix >= 2^31. */
int mumpy_frame_metrics_fwd(const int32_t* counts, int64_t nscored, int64_t npix, double* acc3, int accumulate, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* MUMPY_HIP_EXT5_H */
