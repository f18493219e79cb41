/* mumpy_hip_ext6.h — entry points of libmumpy_hip.so added after the surfaces of mumpy_hip.h (MUMPY_ABI_VERSION 2), mumpy_hip_ext.h
 * (MUMPY_EXT_VERSION 1), mumpy_hip_ext2.h (MUMPY_EXT2_VERSION 2), mumpy_hip_ext3.h (MUMPY_EXT3_VERSION 1), mumpy_hip_ext4.h
 * (MUMPY_EXT4_VERSION 1) and mumpy_hip_ext5.h (MUMPY_EXT5_VERSION 1) were frozen.  No name lives in two headers.
 *
 * The conventions are those of mumpy_hip.h: plain C, raw DEVICE pointers + sizes + `void* stream` last, the CALLER allocates and
 * owns every buffer, nothing here allocates or synchronises (every launching call may be captured into a hipGraph), 0 on success, a
 * negative MUMPY_E* code for a rejected argument (nothing is launched), a positive hipError_t for a failed launch, the message in
 * mumpy_last_error().  This header has a version of its own.
 *
 * The one entry is the annotation side of whole-video scoring (mumpy_hip/video.py): the reference's measure.py:21-40, 77 loads every
 * annotation at its own size, resizes it to 224 x 224 with Image.resize(BILINEAR) and thresholds with > 0.  Pillow's 8-bit resize is
 * two integer passes (horizontal, then vertical) of a triangle filter stretched by the scale; it is reproduced here bit for bit.
 */
#ifndef MUMPY_HIP_EXT6_H
#define MUMPY_HIP_EXT6_H

#include "mumpy_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define MUMPY_EXT6_VERSION 1
int mumpy_ext6_version(void);

/* the largest ykmax / xkmax the kernel is built for: Pillow's BILINEAR tap count is 2 * ceil(max(n_in / n_out, 1)) + 1, so 65 covers
 * every ratio up to 32 (a 7168-pixel side to 224; 4320 -> 224 needs 41) */
#define MUMPY_RESIZE_KMAX_CAP 65
/* bytes of workgroup memory a band of intermediate rows may take (see the W rule below) */
#define MUMPY_RESIZE_BAND_BYTES 49152

/* ---- Image.resize((W, H), Image.BILINEAR) of n single-channel 8-bit images, both passes in one launch ----
 *   src (n, Hs, Ws) uint8.   out (n, H, W) uint8.
 *   ystart / ycount (H) int32 and ycoef (H, ykmax) int32: the vertical taps -- output row y reads source rows ystart[y] ..
 *   ystart[y] + ycount[y] - 1 with the 22-bit fixed-point weights ycoef[y][0 .. ycount[y] - 1].  xstart / xcount (W), xcoef (W, xkmax):
 *   the horizontal taps, likewise.  mumpy_hip.video.bilinear_taps(Hs, H) / (Ws, W) builds Pillow's.
 *   All six tables are DEVICE memory, read by the kernel when it RUNS: a captured launch replays with what was uploaded last.
 *
 *   tmp[r][x] = clip8((2^21 + sum_k xcoef[x][k] * src[f][r][xstart[x] + k]) >> 22)         the horizontal pass, rounded to uint8
 *   out[f][y][x] = clip8((2^21 + sum_k ycoef[y][k] * tmp[ystart[y] + k][x]) >> 22)          the vertical pass
 * with clip8(v) = min(max(v, 0), 255): for the tables of bilinear_taps, mumpy_hip.video.bilinear_resize(src[f], (H, W)) and Pillow's
 * result bit for bit (the sums are 32-bit integers: exact in any order).  tmp never reaches memory: one workgroup takes a band of
 * output rows of one image and keeps the intermediate rows that band reads in workgroup memory.
 *
 * Every element of out is written; src and the six tables are only read.  NO content of the tables makes the kernel read outside
 * src or the tables, or write outside out: a start is clamped to [0, size - 1], a count to [0, kmax], start + k to the last row /
 * column, and the rows one band reads to the capacity of its workgroup memory.  For tables that are not Pillow's the bytes of out
 * are unspecified (sums wrap modulo 2^32); the accesses are in bounds all the same.
 *
 * Any Hs, Ws >= 1, any H >= 1 and no alignment beyond the element's own: rows of 854 or 107 bytes are read as they are, and out
 * is written byte by byte.  W is bounded by the band: min(ykmax + 1, Hs) * W <= MUMPY_RESIZE_BAND_BYTES (W <= 1170 at ykmax 41).
 *
 * MUMPY_ENULL: src, out or one of the six tables null.
 * MUMPY_EINVAL: Hs < 1, Ws < 1, H < 1, W < 1; ykmax or xkmax < 1 or > MUMPY_RESIZE_KMAX_CAP; n < 0 (n == 0 is an accepted no-op: returns
 *   0, launches nothing); min(ykmax + 1, Hs) * W > MUMPY_RESIZE_BAND_BYTES.
 * MUMPY_EALIGN: a table not 4-byte aligned.
 * MUMPY_ERANGE: n >= 2^31; Hs * Ws >= 2^31; H * W >= 2^31; H * ykmax or W * xkmax >= 2^31 (offsets inside an image and inside a table
 *   are 32-bit); n * H >= 2^31 (the bands of all images are numbered in 32 bits). */
int mumpy_resize_bilinear_u8_fwd(const uint8_t* src, uint8_t* out, const int32_t* ystart, const int32_t* ycount, const int32_t* ycoef,
                                 const int32_t* xstart, const int32_t* xcount, const int32_t* xcoef, int64_t n, int Hs, int Ws, int H,
                                 int W, int ykmax, int xkmax, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* MUMPY_HIP_EXT6_H */
