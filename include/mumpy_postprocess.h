/* mumpy_postprocess.h — entry points of libmumpy_hip.so for cleaning predicted masks on the device: connected components smaller
 * than a threshold removed, holes up to a threshold filled (the numpy statement: mumpy_hip/postprocess.py, held to scipy.ndimage by
 * tests/test_postprocess_host.py).  A surface of its own beside mumpy_perturb.h, mumpy_photometric.h and mumpy_geometric.h, with a
 * version of its own; no name lives in two headers.
 *
 * The conventions are those of mumpy_hip.h: plain C, raw DEVICE pointers + sizes + `void* stream` last, the CALLER allocates and
 * owns every buffer, nothing here allocates or synchronises (the launching call may be captured into a hipGraph), 0 on success, a
 * negative MUMPY_E* code for a rejected argument (nothing is launched), a positive hipError_t for a failed launch, the message in
 * mumpy_last_error().
 */
#ifndef MUMPY_POSTPROCESS_H
#define MUMPY_POSTPROCESS_H

#include "mumpy_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define MUMPY_POSTPROCESS_VERSION 1
int mumpy_postprocess_version(void);

/* The largest image: 224 * 224 pixels, whose 16-bit labels (100,352 B) fit one workgroup's LDS on gfx950. */
#define MUMPY_MASK_CLEAN_MAX_PIXELS 50176

/* The bytes of caller-owned workspace mumpy_mask_clean_u8_fwd needs for nimg images of H x W (the component areas of the images in
 * flight: 4 * H * W bytes per workgroup of the launch); 0 for nimg = 0.  A negative MUMPY_E* code for a shape the entry refuses. */
int64_t mumpy_mask_clean_workspace_bytes(int64_t nimg, int H, int W);

/* out[i] = mask[i] cleaned under row i of params; a pixel is foreground where its byte is not 0, the output bytes are 0 or 255:
 *   1. the foreground is labelled with connectivity 8 (4 when the row says 4) and every component of area < min_area becomes
 *      background (min_area <= 1 removes nothing);
 *   2. the background of that result is labelled with the complementary connectivity (4 for 8, 8 for 4); a hole is a background
 *      component with no pixel on the image border; every hole of area <= max_hole becomes foreground (max_hole < 0: every hole;
 *      max_hole = 0: none).
 * mask / out (nimg, H * W) uint8; out == mask (in place) is allowed, any other overlap is refused.
 * gt (nimg, H * W) uint8 or NULL, counts (nimg, 4) int32, NULL exactly when gt is: counts[i] = {sum p & g, sum p, sum g, sum p | g}
 *   of the cleaned mask p against g = gt > 0, written (not accumulated), in the layout of mumpy_mask_score_u8_fwd, so
 *   mumpy_frame_metrics_fwd takes it unchanged.
 * stats (nimg, 8) int32 or NULL: {components found, components kept, pixels removed, holes filled, pixels filled, largest kept
 *   component's area, 0, status}.
 * params (nimg, 4) int32 on the DEVICE, read when the kernel runs (a captured launch follows later uploads):
 *   {min_area, max_hole, connectivity, 0}; a connectivity word other than 4 means 8.  Every int32 row is safe: no content makes the
 *   kernel read or write outside its buffers.  mumpy_hip/postprocess.py: params_row is the one place that encodes a row.
 * workspace: mumpy_mask_clean_workspace_bytes(nimg, H, W) bytes, 16-byte aligned; the kernel zeroes what it uses of it.
 * One launch; image i is handled by one workgroup that keeps the frame's labels in LDS.  Every loop whose trip count depends on the
 * image is bounded by a multiple of H * W; a workgroup that reaches a bound copies its raw mask to out as 0 / 255, writes the counts
 * of that, and sets stats[i] = {0, 0, 0, 0, 0, 0, 0, 1}: status 0 is the only value a correct library ever writes.
 * Every byte of out is written exactly once and no other byte; mask (when not in place), gt and params are only read; the result
 * is bitwise the same from run to run.
 * Refuses: MUMPY_ENULL a null mask, out or params, a null workspace when the needed size is above 0, exactly one of gt and counts;
 * MUMPY_EINVAL nimg < 0, H or W < 1, H * W not a multiple of 16, out overlapping mask without being mask, workspace_bytes too small;
 * MUMPY_ERANGE H * W above MUMPY_MASK_CLEAN_MAX_PIXELS, nimg of 2^31 or more; MUMPY_EALIGN mask, out, gt, params or workspace not
 * 16-byte aligned.  nimg = 0 is a valid call that launches nothing. */
int mumpy_mask_clean_u8_fwd(const uint8_t* mask, uint8_t* out, const uint8_t* gt, int32_t* counts, int32_t* stats,
                            const int32_t* params, void* workspace, int64_t workspace_bytes, int64_t nimg, int H, int W, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* MUMPY_POSTPROCESS_H */
