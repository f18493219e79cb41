/* mumpy_geometric.h — entry points of libmumpy_hip.so for the geometric group of the reference's augmentation file
 * (utils/randaugment.py:20-86 the affine operations, :209-260 Cutout) on uint8 frames and masks that stay on the device.  A surface of
 * its own beside mumpy_perturb.h and mumpy_photometric.h, with a version of its own; no name lives in two headers.
 *
 * The conventions are those of mumpy_hip.h: plain C, raw DEVICE pointers + sizes + `void* stream` last, the CALLER allocates and
 * owns every buffer, nothing here allocates or synchronises (the launching call may be captured into a hipGraph), 0 on success, a
 * negative MUMPY_E* code for a rejected argument (nothing is launched), a positive hipError_t for a failed launch, the message in
 * mumpy_last_error().
 */
#ifndef MUMPY_GEOMETRIC_H
#define MUMPY_GEOMETRIC_H

#include "mumpy_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define MUMPY_GEOMETRIC_VERSION 1
int mumpy_geometric_version(void);

/* The modes (params[i][0]); mumpy_hip/geometric.py: MODES holds the same codes.  0 and every value outside the table copy the image
 * through. */
#define MUMPY_GEO_NONE 0
#define MUMPY_GEO_FIXED16 1
#define MUMPY_GEO_SHIFT 2
#define MUMPY_GEO_RECT 3

/* Image i of dst is image i of src under row i of params, bit for bit what Pillow's Image.transform(size, AFFINE, m, NEAREST,
 * fillcolor=0), Image.rotate(angle, fillcolor=0) and ImageDraw.rectangle(xy, 0) return (the arithmetic: DESIGN.md "Geometric
 * operations", its numpy statement: mumpy_hip/geometric.py).  src / dst (nimg, H, W, C) uint8, C = 1 (masks) or 3 (frames).
 * params (nimg, 8) int32 on the DEVICE, read when the kernel runs (a captured launch follows later uploads):
 * {mode, a0, a1, a2, a3, a4, a5, 0}; mumpy_hip/geometric.py: params_row is the one place that encodes a row.
 *   MUMPY_GEO_FIXED16  the six 16.16 words of Pillow's affine_fixed: output (x, y) is source ((a2 + a0 x + a1 y) >> 16,
 *                      (a5 + a3 x + a4 y) >> 16), or 0 when either index is outside the image
 *   MUMPY_GEO_SHIFT    output (x, y) is source (x + a0, y + a1), or 0 outside (Pillow's scale path for a translation)
 *   MUMPY_GEO_RECT     a copy with the pixels of a0 <= x <= a2, a1 <= y <= a3 set to 0 (Cutout; an empty rectangle is a copy)
 * The walk is done in 64-bit integers, so every int32 row is safe: no row makes the kernel read outside src.
 * One launch, no workspace; every byte of dst is written exactly once and no other byte; src is never written; the result is bitwise
 * the same from run to run.  A gather cannot run in place: dst == src is refused like any other overlap.
 * Refuses: MUMPY_ENULL a null pointer; MUMPY_EALIGN params not 16-byte aligned; MUMPY_EINVAL nimg < 0, H or W < 1, C not 1 or 3, dst
 * overlapping src; MUMPY_ERANGE nimg of 2^31 or more, H or W above 8192, H * W above 2^24. */
int mumpy_geometric_u8_fwd(const uint8_t* src, uint8_t* dst, const int32_t* params, int64_t nimg, int H, int W, int C, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* MUMPY_GEOMETRIC_H */
