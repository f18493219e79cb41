/* mumpy_photometric.h — entry points of libmumpy_hip.so for the photometric half of the reference's augmentation file
 * (utils/randaugment.py:89-110, 129-191) on uint8 frames that stay on the device.  A surface of its own beside mumpy_perturb.h, with a
 * version of its own; no name lives in two headers.
 *
 * The conventions are those of mumpy_hip.h: plain C, raw DEVICE pointers + sizes + `void* stream` last, the CALLER allocates and
 * owns every buffer, nothing here allocates or synchronises (the launching call may be captured into a hipGraph), 0 on success, a
 * negative MUMPY_E* code for a rejected argument (nothing is launched), a positive hipError_t for a failed launch, the message in
 * mumpy_last_error().
 */
#ifndef MUMPY_PHOTOMETRIC_H
#define MUMPY_PHOTOMETRIC_H

#include "mumpy_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define MUMPY_PHOTOMETRIC_VERSION 1
int mumpy_photometric_version(void);

/* The kinds (params[i][0]); mumpy_hip/photometric.py: KINDS holds the same codes.  0 and every value outside the table copy the image
 * through. */
#define MUMPY_PHOTO_NONE 0
#define MUMPY_PHOTO_AUTOCONTRAST 1
#define MUMPY_PHOTO_INVERT 2
#define MUMPY_PHOTO_EQUALIZE 3
#define MUMPY_PHOTO_SOLARIZE 4
#define MUMPY_PHOTO_POSTERIZE 5
#define MUMPY_PHOTO_CONTRAST 6
#define MUMPY_PHOTO_COLOR 7
#define MUMPY_PHOTO_BRIGHTNESS 8
#define MUMPY_PHOTO_SHARPNESS 9

/* Image i of dst is what Pillow returns for one of ImageOps.autocontrast / invert / equalize / solarize / posterize and
 * ImageEnhance.Contrast / Color / Brightness / Sharpness on image i of src, bit for bit (the arithmetic: DESIGN.md "Photometric
 * operations", its numpy statement: mumpy_hip/photometric.py).  src / dst (nimg, H, W, 3) uint8, any H, W >= 1 with H * W <= 2^24
 * (counts and sums of one image stay 32-bit); dst == src is allowed for every kind, any other overlap is refused.
 * params (nimg, 4) int32 on the DEVICE, read when the kernels run (a captured launch follows later uploads): {kind, value, 0, 0}.
 * value: the bits of the float32 factor for contrast, color, brightness and sharpness; the integer ceil(threshold) in 0 .. 256 for
 * solarize (i < threshold in float is i < ceil(threshold)); the integer bit count 0 .. 8 for posterize (read clamped to that range);
 * ignored by the other kinds.  mumpy_hip/photometric.py: params_row is the one place that encodes a row.
 * Three launches: (1) per image and slab of pixels, the three 256-bin histograms (autocontrast, equalize) or the sum of the
 * luminance (contrast) into the workspace, and for sharpness a copy of the image there (the stencil of an in-place call must not read
 * what it wrote); images of the other kinds cost one read of their kind.  (2) one workgroup per image: the 3 x 256 byte lookup table
 * of the seven kinds that are pointwise given the statistics.  (3) streaming: gather through the table / blend with the luminance /
 * blend with the 3x3 SMOOTH filter of the copy.
 * The result does not depend on what the workspace held, and is bitwise the same from run to run.
 * workspace: mumpy_photometric_workspace_bytes(nimg, H, W) bytes (that query: MUMPY_EINVAL / MUMPY_ERANGE as below); no byte beyond
 * them is written.
 * Refuses: MUMPY_ENULL a null pointer; MUMPY_EALIGN params or workspace not 16-byte aligned; MUMPY_EINVAL nimg < 0, H or W < 1,
 * workspace_bytes below the query, dst overlapping src without being src; MUMPY_ERANGE nimg of 2^31 or more, H * W above 2^24. */
int64_t mumpy_photometric_workspace_bytes(int64_t nimg, int H, int W);
int mumpy_photometric_u8_fwd(const uint8_t* src, uint8_t* dst, const int32_t* params, void* workspace, int64_t workspace_bytes,
                             int64_t nimg, int H, int W, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* MUMPY_PHOTOMETRIC_H */
