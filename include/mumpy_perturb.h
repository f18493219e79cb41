/* mumpy_perturb.h — entry points of libmumpy_hip.so for ordinary post-processing of uint8 frames on the device.  A surface of its own,
 * beside mumpy_hip.h and mumpy_hip_ext.h .. mumpy_hip_ext10.h, with a version of its own; no name lives in two headers.
 *
 * The conventions are those of mumpy_hip.h: plain C, raw DEVICE pointers + sizes + `void* stream` last, the CALLER allocates and
 * owns every buffer, nothing here allocates or synchronises (every launching call may be captured into a hipGraph), 0 on success, a
 * negative MUMPY_E* code for a rejected argument (nothing is launched), a positive hipError_t for a failed launch, the message in
 * mumpy_last_error().
 *
 * ROBUSTNESS OF THE INPUT CLIP: the gradient and the PGD step of mumpy_hip_ext10.h are its worst-case half, the two ordinary
 * perturbations here its average-case half -- the JPEG round trip and the Gaussian blur of the reference's augmentation code
 * (utils/randaugment.py:492-512), bit for bit what Pillow computes, on uint8 frames (nimg, H, W, 3) that stay on the device.
 * Every per-image setting (quantisation tables, table choice, box parameters) is DEVICE memory read when the kernel runs: a captured
 * launch follows later uploads.  mumpy_resize_nearest_u8_fwd puts source frames on the canvas that is perturbed.
 */
#ifndef MUMPY_PERTURB_H
#define MUMPY_PERTURB_H

#include "mumpy_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define MUMPY_PERTURB_VERSION 1
int mumpy_perturb_version(void);

/* The JPEG round trip: image i of dst is what Pillow returns for save(format="JPEG", quality=q) followed by Image.open -- baseline
 * JPEG, YCbCr 4:2:0, libjpeg's slow-integer DCT both ways (the inverse with a saturating clamp), fancy (triangle) chroma upsampling.
 * Entropy coding is lossless and not done.  src / dst (nimg, H, W, 3) uint8, any H, W >= 1, dst == src allowed (partial overlap is
 * not).  qtab (ntab, 2, 64) uint16: luminance then chrominance, natural row-major order, entries >= 1 (an entry 0 is read as 1);
 * sel (nimg) int32: the table of image i.  sel[i] < 0 copies the image through unchanged; sel[i] >= ntab cannot be refused on the host
 * (sel is device memory) and the kernels treat it as "copy through" as well.
 * Two launches: (1) one wave per 16x16 MCU: colour conversion, 2x2 chroma downsampling, per 8x8 block forward DCT -> quantise ->
 * dequantise -> inverse DCT; the decoded Y (H, W) and Cb, Cr (ceil(H/2), ceil(W/2)) planes go to the workspace; (2) per pixel:
 * triangle upsampling of the chroma (it reads the neighbouring MCUs' chroma: hence two launches) and YCbCr -> RGB into dst.
 * Edges: input columns are replicated to a multiple of 16 and input rows to an even count; after the downsampling every plane is
 * padded to a multiple of 8 rows by its own last row.
 * workspace: mumpy_jpeg_roundtrip_workspace_bytes(nimg, H, W) bytes (that query: MUMPY_EINVAL / MUMPY_ERANGE as below); no byte
 * beyond them is written.
 * Refuses: MUMPY_ENULL a null pointer; MUMPY_EALIGN qtab or workspace not 16-byte aligned, sel not 4-byte aligned; MUMPY_EINVAL
 * nimg < 0, H or W < 1, ntab < 1, workspace_bytes below the query; MUMPY_ERANGE nimg or 3*H*W of 2^31 or more. */
int64_t mumpy_jpeg_roundtrip_workspace_bytes(int64_t nimg, int H, int W);
int mumpy_jpeg_roundtrip_u8_fwd(const uint8_t* src, uint8_t* dst, const uint16_t* qtab, const int32_t* sel, void* workspace,
                                int64_t workspace_bytes, int64_t nimg, int ntab, int H, int W, void* stream);

/* ImageFilter.GaussianBlur(radius) of Pillow on RGB images: three extended-box passes along rows, then three along columns, uint8
 * between passes.  One pass along a line of n samples, in unsigned 32-bit arithmetic, indices clamped to [0, n - 1] (a window may be
 * wider than the image):
 *     out[x] = (ww * sum_{d=-r..r} in[x + d] + fw * (in[x - r - 1] + in[x + r + 1]) + 2^23) >> 24
 * params (nimg, 4) int32 on the device: {r, ww, fw, on} of image i, computed by the host in Pillow's float arithmetic
 * (mumpy_hip/perturb.py: box_params); on == 0 copies the image through; a negative r is read as 0.  src / dst (nimg, H, W, 3) uint8,
 * dst == src allowed.  Two launches: the row passes on a row held in LDS (into the workspace), the column passes on a tile of 16, 8,
 * 4, 2 or 1 columns held in LDS -- the widest whose two buffers of H rows fit 64 KiB.
 * workspace: mumpy_gaussian_blur_workspace_bytes(nimg, H, W) bytes.
 * Refuses: MUMPY_ENULL a null pointer; MUMPY_EALIGN params or workspace not 16-byte aligned; MUMPY_EINVAL nimg < 0, H or W < 1,
 * workspace_bytes below the query; MUMPY_ERANGE nimg or 3*H*W of 2^31 or more, H or W above 10922 (a line does not fit LDS). */
int64_t mumpy_gaussian_blur_workspace_bytes(int64_t nimg, int H, int W);
int mumpy_gaussian_blur_u8_fwd(const uint8_t* src, uint8_t* dst, const int32_t* params, void* workspace, int64_t workspace_bytes,
                               int64_t nimg, int H, int W, void* stream);

/* Image.resize((W, H), NEAREST) of nimg images of C interleaved channels (3: RGB frames, 1: their masks, which have to reach the same
 * canvas): dst[i, y, x] = src[i, ytab[y], xtab[x]], src (nimg, Hs, Ws, C) and dst (nimg, H, W, C) uint8, ytab (H) / xtab (W) int32 on
 * the device as mumpy_resize_nearest_table fills them (entries are clamped to the source: the tables are device memory that nobody
 * validated).  src and dst must not overlap.
 * Refuses: MUMPY_ENULL a null pointer; MUMPY_EALIGN a table not 4-byte aligned; MUMPY_EINVAL nimg < 0, a side < 1 or C outside
 * 1 .. 4; MUMPY_ERANGE nimg, C*Hs*Ws or C*H*W of 2^31 or more. */
int mumpy_resize_nearest_u8_fwd(const uint8_t* src, uint8_t* dst, const int32_t* ytab, const int32_t* xtab, int64_t nimg, int Hs,
                                int Ws, int H, int W, int C, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* MUMPY_PERTURB_H */
