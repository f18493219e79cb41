/* mumpy_hip_ext4.h — entry points of libmumpy_hip.so added after the surfaces of mumpy_hip.h (MUMPY_ABI_VERSION 2), mumpy_hip_ext.h
 * (MUMPY_EXT_VERSION 1), mumpy_hip_ext2.h (MUMPY_EXT2_VERSION 2) and mumpy_hip_ext3.h (MUMPY_EXT3_VERSION 1) were frozen.  No name
 * lives in two headers.
 *
 * The conventions are those of mumpy_hip.h: plain C, raw DEVICE pointers + sizes + `void* stream` last, the CALLER allocates and
 * owns every buffer, nothing here allocates or synchronises (every launching call may be captured into a hipGraph), 0 on success, a
 * negative MUMPY_E* code for a rejected argument (nothing is launched), a positive hipError_t for a failed launch, the message in
 * mumpy_last_error().  This header has a version of its own; it is the one that grows from here on, by appending.
 */
#ifndef MUMPY_HIP_EXT4_H
#define MUMPY_HIP_EXT4_H

#include "mumpy_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define MUMPY_EXT4_VERSION 1
int mumpy_ext4_version(void);

/* ---- the training input stage with the interpolating augmentations: one call for a batch whose clips mix all modes ----
 * mumpy_augment_stage_u8_fwd (mumpy_hip_ext3.h) runs the augmentations that permute pixels.  The reference's other two shape operations
 * interpolate on the L x L canvas: RandomScaleCrop (a CUBIC upscale, a crop box, NEAREST back) and RandomRotate (a bilinear rotation
 * and a centre crop).  Here every clip carries a mode word, and the 8-bit value v of an output pixel is formed from the canvas
 *
 *   canvas_c(Y, X) = src[clamp(tab_a[c][i], 0, Hs - 1), clamp(tab_b[c][j], 0, Ws - 1)],   (i, j) = swap[c] & 1 ? (X, Y) : (Y, X)
 *
 * (src: a frame channel of clip c, or mask c % nmasks; tab_a / tab_b / swap: what mumpy_hip/augment.py's clip_tables returns).
 *
 *   frames, masks, out, target, nclips, T, nmasks, Hs, Ws, L, mean3, std3, stream: exactly as in mumpy_augment_stage_u8_fwd.
 *   tab_a, tab_b (nclips, L) int32, swap (nclips) int32: the canvas accessor.
 *   mode (nclips) int32, read as mode & 3; 3 behaves as 0.
 *   pos_y, pos_x (nclips, L) int32;  coef_y, coef_x (nclips, L, 4) int32;  affine (nclips, 8) float32: m00 m01 m02 m10 m11 m12 0 0.
 *   All of these are DEVICE memory, read by the kernel when it RUNS: a captured launch replays with what was uploaded last.
 *
 * With clampL(k) = clamp(k, 0, L - 1) and clip8(a) = clamp(a, 0, 255), output pixel (y, x) of clip c:
 *   mode 0 (gather):  v = canvas(y, x) -- the output equals mumpy_augment_stage_u8_fwd bitwise.
 *   mode 1 (separable 4-tap fixed point: Pillow's 8-bit resample, horizontal pass then vertical pass):
 *       h_j = clip8((2^21 + sum_{i<4} coef_x[x][i] * canvas(clampL(pos_y[y] + j), clampL(pos_x[x] + i))) >> 22)      for j < 4
 *       v   = clip8((2^21 + sum_{j<4} coef_y[y][j] * h_j) >> 22)
 *     in 32-bit two's complement: the sums wrap (they do not for normalised cubic taps: sum |k| * 255 < 2^31), >> is arithmetic;
 *     pos + i is formed without overflow.  A tap that Pillow drops at an edge arrives as a zero coefficient.
 *   mode 2 (bilinear under an affine map, constant-0 border), in fp32:
 *       u = (float)pos_x[x], w = (float)pos_y[y];  sx = m00 * u + m01 * w + m02,  sy = m10 * u + m11 * w + m12
 *       x0 = floor(sx), y0 = floor(sy), fx = sx - x0, fy = sy - y0
 *       p(dy, dx) = canvas(y0 + dy, x0 + dx) when 0 <= y0 + dy <= L - 1 and 0 <= x0 + dx <= L - 1, else 0
 *       blend = (1 - fy) * ((1 - fx) * p(0,0) + fx * p(0,1)) + fy * ((1 - fx) * p(1,0) + fx * p(1,1))
 *       v = clip8((int)(blend + 0.5f));   a NaN or out-of-range sx / sy is "outside": v = 0.  (The compiler may contract a * b + c.)
 *   out[c*T + t, ch, y, x] = ((float)v / 255.0f - mean[ch]) / std[ch]        (the expression of mumpy_normalize_u8_fwd, same order)
 *   target[c, y*L + x]     = v_mask > 0 ? 1.0f : 0.0f                         (v_mask: the same arithmetic on mask c % nmasks)
 * Nothing here can be validated on the host, so the clamps, the `& 1` and the `& 3` are part of the contract: NO content of any table,
 * mode word or affine row makes the kernel read outside frames / masks.  Every element of out (and of target, when given) is
 * written; all inputs are only read.  One launch; the mode is uniform over a block.
 *
 * MUMPY_ENULL: frames, out, tab_a, tab_b, swap, mode, pos_y, pos_x, coef_y, coef_x, affine, mean3 or std3 null; exactly one of masks /
 *   target given.
 * MUMPY_EINVAL: T < 1, Hs < 1, Ws < 1, L < 4 or L % 4 != 0; nclips < 0 (nclips == 0 is an accepted no-op: returns 0, launches nothing);
 *   with masks, nmasks < 1 or nclips % nmasks != 0 (without masks nmasks is ignored); a zero std.
 * MUMPY_EALIGN: out, target, tab_a, tab_b, pos_y, pos_x, coef_y or coef_x not 16-byte aligned (16-byte stores and loads; L % 4 == 0
 *   keeps every row so).  swap, mode and affine are read a word at a time.
 * MUMPY_ERANGE: nclips * T >= 2^31; 3 * Hs * Ws >= 2^31; 3 * L * L >= 2^31 (as in mumpy_augment_stage_u8_fwd). */
int mumpy_augment_warp_u8_fwd(const uint8_t* frames, const uint8_t* masks, float* out, float* target,
                              const int32_t* tab_a, const int32_t* tab_b, const int32_t* swap, const int32_t* mode,
                              const int32_t* pos_y, const int32_t* pos_x, const int32_t* coef_y, const int32_t* coef_x,
                              const float* affine, int64_t nclips, int T, int64_t nmasks, int Hs, int Ws, int L,
                              const float* mean3, const float* std3, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* MUMPY_HIP_EXT4_H */
