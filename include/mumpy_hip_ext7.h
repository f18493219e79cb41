/* mumpy_hip_ext7.h — entry points of libmumpy_hip.so added after the surfaces of mumpy_hip.h (MUMPY_ABI_VERSION 2), mumpy_hip_ext.h
 * (MUMPY_EXT_VERSION 1), mumpy_hip_ext2.h (MUMPY_EXT2_VERSION 2), mumpy_hip_ext3.h (MUMPY_EXT3_VERSION 1), mumpy_hip_ext4.h
 * (MUMPY_EXT4_VERSION 1), mumpy_hip_ext5.h (MUMPY_EXT5_VERSION 1) and mumpy_hip_ext6.h (MUMPY_EXT6_VERSION 1) were frozen.  No name
 * lives in two headers.
 *
 * The conventions are those of mumpy_hip.h: plain C, raw DEVICE pointers + sizes + `void* stream` last, the CALLER allocates and
 * owns every buffer, nothing here allocates or synchronises (every launching call may be captured into a hipGraph), 0 on success, a
 * negative MUMPY_E* code for a rejected argument (nothing is launched), a positive hipError_t for a failed launch, the message in
 * mumpy_last_error().  This header has a version of its own.
 *
 * These two score a whole video at EVERY threshold of a table in one pass (mumpy_hip/video.py: VideoPredictor(sweep=...)): the
 * reference fixes the mask threshold at 0.5 (test.py:108, measure.py:85); choosing the operating point on a validation split, or
 * a pixel-level ROC, otherwise costs one forward per candidate.  The logits, the annotation bank and the clip-to-frame table are on
 * the device while the forward's graph runs; the first call counts, per frame and class, the pixels whose probability exceeds each
 * threshold, the second turns the counts into per-threshold metric sums.
 */
#ifndef MUMPY_HIP_EXT7_H
#define MUMPY_HIP_EXT7_H

#include "mumpy_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define MUMPY_EXT7_VERSION 1
int mumpy_ext7_version(void);

/* the longest threshold table: K + 1 = 1024 bins per class */
#define MUMPY_SWEEP_MAX_THRESHOLDS 1023

/* ---- per frame and class, the number of pixels whose probability exceeds each threshold of a table ----
 *   logits (nclips, npix) float32, as mumpy_final_conv_fwd writes them.
 *   gt (nbank, npix) uint8: the per-frame annotations, > 0 is forged (the gt bank of mumpy_mask_score_u8_fwd).
 *   dest (nclips) int32: the frame each clip belongs to.   thr_tab (K) float32, ascending.
 *   exceed (nbank, 2, K + 1) int32.
 * dest and thr_tab are DEVICE memory read when the kernel RUNS: a captured launch replays with what was uploaded last.
 * For clip c with 0 <= dest[c] < nbank, d = dest[c], p_i = 1.0f / (1.0f + __expf(-logits[c][i])), class g_i = gt[d][i] > 0:
 *   exceed[d][g][k] = #{ i : g_i == g and p_i > thr_tab[k] }        k = 0 .. K - 1
 *   exceed[d][g][K] = #{ i : g_i == g }
 * Row k is exactly what mumpy_mask_score_u8_fwd counts from the mask mumpy_final_conv_fwd emits at thr = thr_tab[k]:
 *   inter = exceed[d][1][k],  sum p = exceed[d][0][k] + exceed[d][1][k],  sum g = exceed[d][1][K],  union = sum p + sum g - inter
 * BIT FOR BIT, by contract: the two kernels share the sigmoid-and-compare expression (csrc/sigmoid_thr.h), the comparison is the
 * same strict `>` (a probability equal to a threshold does not exceed it) and a NaN logit exceeds nothing, as in the mask.
 * The rows are WRITTEN, not accumulated: exceed needs no zeroing.  A clip whose dest is outside [0, nbank) writes NOTHING (the padding
 * clips of a batch tail carry -1); rows no dest names are left as they are.  Two clips with the same valid dest in one call are the
 * CALLER's error.  One workgroup per clip, integer counting only, no arrival order in the result: the same input gives the same bits.
 * logits, gt, dest and thr_tab are only read.
 * The table's CONTENT cannot be validated on the host.  Whatever it holds (unsorted, NaN), the kernel writes only the exceed rows of
 * valid dests and every value written lies in [0, npix]; only an ascending table gives the meaning above.
 *
 * MUMPY_ENULL: logits, gt, dest, thr_tab or exceed null.
 * MUMPY_EINVAL: npix < 1 or npix % 16 != 0; nbank < 1; nclips < 0 (nclips == 0 is an accepted no-op: returns 0, launches nothing);
 *   K < 1 or K > MUMPY_SWEEP_MAX_THRESHOLDS.
 * MUMPY_EALIGN: logits, gt, thr_tab or exceed not 16-byte aligned (16-byte loads; npix % 16 == 0 keeps every row of logits and gt so).
 * MUMPY_ERANGE: nclips, npix, nbank or nbank * 2 * (K + 1) >= 2^31 (dest, the counts and the offsets into exceed are 32-bit). */
int mumpy_score_exceed_fwd(const float* logits, const uint8_t* gt, const int32_t* dest, const float* thr_tab, int32_t* exceed,
                           int64_t nclips, int64_t npix, int64_t nbank, int K, void* stream);

/* ---- per-threshold F1 / IoU sums over a video, and the counts pooled over its frames ----
 *   exceed (>= nscored, 2, K + 1) int32 as mumpy_score_exceed_fwd writes them: frames 0 .. nscored - 1 are read.
 *   acc (K, 3) double in DEVICE memory: acc[k] = [sum F1, sum IoU, n] over the frames at threshold k -- row k has the layout
 *   mumpy_frame_metrics_fwd gives its acc3.   pooled (2, K + 1) int64, or NULL: pooled[g][j] = sum over the frames of exceed[f][g][j]
 *   (the ROC points of the table: FPR_k = pooled[0][k] / pooled[0][K], TPR_k = pooled[1][k] / pooled[1][K]).
 * Per frame and threshold, in fp64, the expressions of mumpy_frame_metrics_fwd (csrc/frame_metric.h is shared by the two kernels)
 * applied to the four counts derived above:
 *   recall = inter / (sum g + 1e-6 * npix),  precision = inter / (sum p + 1e-6),  F1 = 2 P R / (P + R + 1e-6),
 *   IoU = (inter + 1e-5) / (union + 1e-5)
 * accumulate == 0: both outputs are overwritten; else the sums are added into both (one accumulator over the videos of a dataset).
 * nscored == 0 is accepted: it writes zeros, or adds nothing.  One workgroup per threshold with a fixed-order reduce over the frames,
 * pooled summed in frame order in integers: the same input gives the same bits.  exceed is only read.
 *
 * MUMPY_ENULL: exceed or acc null.   MUMPY_EINVAL: nscored < 0, npix < 1, K < 1 or K > MUMPY_SWEEP_MAX_THRESHOLDS.
 * MUMPY_EALIGN: acc or pooled not 8-byte aligned.
 * MUMPY_ERANGE: nscored, npix or nscored * 2 * (K + 1) >= 2^31. */
int mumpy_sweep_metrics_fwd(const int32_t* exceed, int64_t nscored, int64_t npix, int K, double* acc, int64_t* pooled,
                            int accumulate, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* MUMPY_HIP_EXT7_H */
