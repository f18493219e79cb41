/* mumpy_hip_ext10.h — entry points of libmumpy_hip.so added after the surfaces of mumpy_hip.h (MUMPY_ABI_VERSION 2) and
 * mumpy_hip_ext.h .. mumpy_hip_ext9.h were frozen.  No name lives in two headers.
 *
 * The conventions are those of mumpy_hip.h: plain C, raw DEVICE pointers + sizes + `void* stream` last, the CALLER allocates and
 * owns every buffer, nothing here allocates or synchronises (every launching call may be captured into a hipGraph), 0 on success, a
 * negative MUMPY_E* code for a rejected argument (nothing is launched), a positive hipError_t for a failed launch, the message in
 * mumpy_last_error().  Per-channel constants are HOST arrays of three floats, read before the launch.  This header has a version
 * of its own.
 *
 * THE GRADIENT WITH RESPECT TO THE INPUT CLIP.  A clip x (B,T,3,H,W) enters the three-view model in two places: the tokenizer
 * gathers it into one column matrix per view (Conv3d with kernel = stride = (t_v,4,4) as a Linear over columns ordered
 * (ch, t, py, px)), and the FAF branch transforms ONE frame of it (mumpy_faf_fwd).  mumpy_faf_bwd is the adjoint of the second,
 * mumpy_tokenize_dx the adjoint of the first with the FAF part folded in, mumpy_pgd_step the projected signed-gradient update that
 * consumes the result.  All three are deterministic: no atomics, a fixed summation order.
 */
#ifndef MUMPY_HIP_EXT10_H
#define MUMPY_HIP_EXT10_H

#include "mumpy_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define MUMPY_EXT10_VERSION 1
int mumpy_ext10_version(void);

/* The gradient of mumpy_faf_fwd with respect to the frame it read.  dout (B,9,224,224), channel = band*3 + rgb; D / Dt the DCT
 * matrix and its transpose (224,224), as the forward takes them; scratch B*3*224*224 floats (the summed spectrum);
 *     dxf (B,3,224,224) = D^T ( sum_band M_band o (D dout[band,rgb] D^T) ) D,    M_band = [lo <= i + j <= hi]
 * with the forward's bands: low [0, lo_hi], mid [mid_lo, mid_hi], high [224, 448].  A coefficient in two bands counts twice, one in
 * none contributes nothing.  Two launches, exact fp32 MFMA, the bands summed in the order low, mid, high.
 * Refuses: MUMPY_ENULL a null pointer; MUMPY_EALIGN a pointer not 16-byte aligned; MUMPY_EINVAL B < 1 or band limits the forward
 * refuses. */
int mumpy_faf_bwd(const float* dout, const float* D, const float* Dt, float* scratch, float* dxf, int B, int lo_hi, int mid_lo,
                  int mid_hi, void* stream);

/* One launch: the three views' column gradients and (optionally) the FAF gradient folded into dx (B,T,3,H,W).
 * dcols_v (B*tt_v*(H/4)*(W/4), ld_v), tt_v = (T - t_v)/t_v + 1 tubelets of t_v frames, columns (ch, t, py, px); ld_v >= 48 t_v is
 * the row stride in floats (the 32-padded K: a multiple of 4), the columns past 48 t_v are never read.  dxf (B,3,H,W) or null goes to
 * frame `frame`.  Every element of dx is written exactly once, nothing needs zeroing:
 *     dx[b,f,ch,y,x] = sum_v [f < tt_v t_v] dcols_v[(b, f / t_v, y/4, x/4), (ch, f % t_v, y%4, x%4)] + [f == frame] dxf[b,ch,y,x]
 * summed in the order v = 0, 1, 2, dxf (a view whose tubelets do not reach frame f adds nothing to it).
 * Refuses: MUMPY_ENULL a null dcols_v or dx; MUMPY_EALIGN a pointer not 16-byte aligned; MUMPY_EINVAL B < 1, T < 1, H or W not a
 * positive multiple of 4, t_v outside [1, T], ld_v < 48 t_v or not a multiple of 4, (dxf given) frame outside [0, T);
 * MUMPY_ERANGE 3*H*W or a row count of 2^31 or more. */
int mumpy_tokenize_dx(const float* dcols0, const float* dcols1, const float* dcols2, const float* dxf, float* dx, int B, int T, int H,
                      int W, int t0, int t1, int t2, int ld0, int ld1, int ld2, int frame, void* stream);

/* One projected signed-gradient step, in place, on a normalised clip of n = (clips*frames) * 3 * hw elements (channel of element i:
 * (i / hw) % 3):
 *     x_adv <- clamp( clamp(x_adv + alpha * sgn(g), x0 - eps_c, x0 + eps_c), lo_c, hi_c ),     clamp(v, a, b) = min(max(v, a), b)
 * in fp32 in exactly this order (the same torch expression gives the same bits).  sgn(0) = sgn(-0) = 0, a NaN gradient counts as 0
 * (the element is only re-projected), +-inf as +-1.  alpha may be negative (descent).  eps3 / lo3 / hi3: HOST arrays.
 * Refuses: MUMPY_ENULL a null pointer; MUMPY_EALIGN a device pointer not 16-byte aligned; MUMPY_EINVAL n < 0, hw < 1, n not a
 * multiple of 3*hw, a negative or NaN eps_c, lo_c > hi_c, a non-finite alpha. */
int mumpy_pgd_step(float* x_adv, const float* g, const float* x0, int64_t n, int64_t hw, float alpha, const float* eps3,
                   const float* lo3, const float* hi3, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* MUMPY_HIP_EXT10_H */
