// input_grad.hip — the gradient with respect to the input clip (include/mumpy_hip_ext10.h): the fold of the three views' column
// gradients (+ the FAF gradient of one frame) into dx, and the projected signed-gradient step that consumes it.  Both are streaming
// kernels over a few MB: 16-byte accesses, no LDS, no atomics, every output element written exactly once.
//
// tokenize_dx: the tokenizer's forward gathers x (B,T,3,H,W) into rows (b, tubelet, py, px) x columns (ch, t, y%4, x%4) per view
// (Conv3d with kernel = stride = (t_v,4,4)); every pixel of a frame that view v reaches lies in exactly one row of its matrix, so the
// adjoint is a gather too.  A thread owns the 4 pixels (y, 4 px .. 4 px + 3) of one plane: in each view they are 16 contiguous bytes of
// one row of dcols_v.  Lanes 4k .. 4k+3 of a wave take the four image rows of one patch, i.e. 64 contiguous bytes of that row; the 16
// patches of a wave are neighbours along x, so the stores are runs of 256 bytes in each of the four image rows.
#include "common.h"
#include "../../include/mumpy_hip_ext10.h"
using namespace mumpy;

namespace {

struct DxView {
    const float* dcols;      // (B * tt * (H/4) * (W/4), ld)
    int t, tt, ld;           // frames per tubelet, tubelets per clip, row stride in floats
};

__global__ __launch_bounds__(256) void tokenize_dx_kernel(DxView v0, DxView v1, DxView v2, const float* __restrict__ dxf,
                                                          float* __restrict__ dx, int64_t items, int T, int H, int W, int frame) {
    const int hp = H >> 2, wp = W >> 2;
    for (int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x; idx < items; idx += (int64_t)gridDim.x * 256) {
        const int r4 = (int)(idx & 3);
        int64_t p = idx >> 2;
        const int px = (int)(p % wp);
        p /= wp;
        const int py = (int)(p % hp);
        p /= hp;                                             // plane (b, f, ch)
        const int ch = (int)(p % 3);
        const int64_t bf = p / 3;
        const int f = (int)(bf % T);
        const int64_t b = bf / T;
        f32x4 s = {0.f, 0.f, 0.f, 0.f};
        const DxView* vs[3] = {&v0, &v1, &v2};
#pragma unroll
        for (int v = 0; v < 3; ++v) {
            const DxView& w = *vs[v];
            if (f < w.tt * w.t) {                            // (view 2, tubelet T-1, never reaches frame T-1)
                const int tb = f / w.t, ft = f - tb * w.t;
                const int64_t row = ((b * w.tt + tb) * hp + py) * wp + px;
                s += *reinterpret_cast<const f32x4*>(w.dcols + row * w.ld + ((ch * w.t + ft) * 4 + r4) * 4);
            }
        }
        const int y = 4 * py + r4, x = 4 * px;
        if (dxf != nullptr && f == frame) s += *reinterpret_cast<const f32x4*>(dxf + ((b * 3 + ch) * H + y) * (int64_t)W + x);
        *reinterpret_cast<f32x4*>(dx + (p * H + y) * (int64_t)W + x) = s;
    }
}

__device__ __forceinline__ float pgd_one(float x, float g, float x0, float alpha, float eps, float lo, float hi) {
    const float sg = g > 0.f ? 1.f : (g < 0.f ? -1.f : 0.f);          // NaN compares false twice: 0
    float v = x + alpha * sg;                                          // (alpha * sg is exact: contracted or not, one rounding)
    v = fminf(fmaxf(v, x0 - eps), x0 + eps);
    return fminf(fmaxf(v, lo), hi);
}

// VEC: hw % 4 == 0, so four consecutive elements share a channel and the buffers are walked 16 bytes at a time
template <bool VEC>
__global__ __launch_bounds__(256) void pgd_step_kernel(float* __restrict__ xa, const float* __restrict__ g, const float* __restrict__ x0,
                                                       int64_t n, int64_t hw, float alpha, float e0, float e1, float e2, float l0, float l1,
                                                       float l2, float h0, float h1, float h2) {
    const int64_t step = (int64_t)gridDim.x * 256;
    if (VEC) {
        for (int64_t q = (int64_t)blockIdx.x * 256 + threadIdx.x; 4 * q < n; q += step) {
            const int ch = (int)(((4 * q) / hw) % 3);
            const float eps = ch == 0 ? e0 : (ch == 1 ? e1 : e2), lo = ch == 0 ? l0 : (ch == 1 ? l1 : l2), hi = ch == 0 ? h0 : (ch == 1 ? h1 : h2);
            f32x4 x = *reinterpret_cast<const f32x4*>(xa + 4 * q);
            const f32x4 gg = *reinterpret_cast<const f32x4*>(g + 4 * q), xx = *reinterpret_cast<const f32x4*>(x0 + 4 * q);
#pragma unroll
            for (int k = 0; k < 4; ++k) x[k] = pgd_one(x[k], gg[k], xx[k], alpha, eps, lo, hi);
            *reinterpret_cast<f32x4*>(xa + 4 * q) = x;
        }
    } else {
        for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += step) {
            const int ch = (int)((i / hw) % 3);
            const float eps = ch == 0 ? e0 : (ch == 1 ? e1 : e2), lo = ch == 0 ? l0 : (ch == 1 ? l1 : l2), hi = ch == 0 ? h0 : (ch == 1 ? h1 : h2);
            xa[i] = pgd_one(xa[i], g[i], x0[i], alpha, eps, lo, hi);
        }
    }
}

inline unsigned grid_for(int64_t threads) {
    const int64_t blocks = (threads + 255) / 256;
    return (unsigned)(blocks < 1 ? 1 : (blocks < 8192 ? blocks : 8192));
}

}  // namespace

extern "C" int mumpy_tokenize_dx(const float* dcols0, const float* dcols1, const float* dcols2, const float* dxf, float* dx, int B, int T,
                                 int H, int W, int t0, int t1, int t2, int ld0, int ld1, int ld2, int frame, void* stream) {
    MUMPY_REQUIRE(dcols0 && dcols1 && dcols2 && dx, MUMPY_ENULL, "tokenize_dx: null pointer");
    MUMPY_REQUIRE(aligned16(dcols0) && aligned16(dcols1) && aligned16(dcols2) && aligned16(dxf) && aligned16(dx), MUMPY_EALIGN,
                  "tokenize_dx: pointers must be 16-byte aligned");
    MUMPY_REQUIRE(B > 0 && T > 0 && H >= 4 && W >= 4 && H % 4 == 0 && W % 4 == 0, MUMPY_EINVAL,
                  "tokenize_dx: bad sizes B=%d T=%d, %dx%d (H and W must be positive multiples of 4)", B, T, H, W);
    const float* ptr[3] = {dcols0, dcols1, dcols2};
    const int t[3] = {t0, t1, t2}, ld[3] = {ld0, ld1, ld2};
    for (int v = 0; v < 3; ++v) {
        MUMPY_REQUIRE(t[v] >= 1 && t[v] <= T, MUMPY_EINVAL, "tokenize_dx: tubelet %d of view %d outside [1, T=%d]", t[v], v, T);
        MUMPY_REQUIRE(ld[v] >= 48 * t[v] && ld[v] % 4 == 0, MUMPY_EINVAL,
                      "tokenize_dx: row stride %d of view %d must be a multiple of 4 and at least 48 * %d", ld[v], v, t[v]);
    }
    MUMPY_REQUIRE(!dxf || (frame >= 0 && frame < T), MUMPY_EINVAL, "tokenize_dx: frame %d outside clip of %d", frame, T);
    constexpr int64_t LIM = (int64_t)1 << 31;
    MUMPY_REQUIRE(3 * (int64_t)H * W < LIM && (int64_t)B * T * (H / 4) * (W / 4) < LIM, MUMPY_ERANGE,
                  "tokenize_dx: 3*%d*%d or the row count B*T*(H/4)*(W/4) is 2^31 or more", H, W);
    DxView vw[3];
    for (int v = 0; v < 3; ++v) vw[v] = DxView{ptr[v], t[v], (T - t[v]) / t[v] + 1, ld[v]};
    const int64_t items = (int64_t)B * T * 3 * H * (W / 4);
    hipLaunchKernelGGL(tokenize_dx_kernel, dim3(grid_for(items)), dim3(256), 0, as_stream(stream), vw[0], vw[1], vw[2], dxf, dx, items, T,
                       H, W, frame);
    MUMPY_CHECK_LAUNCH("tokenize_dx");
    return 0;
}

extern "C" int mumpy_pgd_step(float* x_adv, const float* g, const float* x0, int64_t n, int64_t hw, float alpha, const float* eps3,
                              const float* lo3, const float* hi3, void* stream) {
    MUMPY_REQUIRE(x_adv && g && x0 && eps3 && lo3 && hi3, MUMPY_ENULL, "pgd_step: null pointer");
    MUMPY_REQUIRE(aligned16(x_adv) && aligned16(g) && aligned16(x0), MUMPY_EALIGN, "pgd_step: x_adv, g and x0 must be 16-byte aligned");
    MUMPY_REQUIRE(n >= 0 && hw >= 1 && n % (3 * hw) == 0, MUMPY_EINVAL,
                  "pgd_step: n=%lld must be a multiple of 3*hw, hw=%lld >= 1", (long long)n, (long long)hw);
    MUMPY_REQUIRE(alpha - alpha == 0.f, MUMPY_EINVAL, "pgd_step: alpha must be finite");
    for (int c = 0; c < 3; ++c)
        MUMPY_REQUIRE(eps3[c] >= 0.f && lo3[c] <= hi3[c], MUMPY_EINVAL, "pgd_step: channel %d needs eps >= 0 and lo <= hi", c);
    if (n == 0) return 0;
    if (hw % 4 == 0)
        hipLaunchKernelGGL(pgd_step_kernel<true>, dim3(grid_for(n / 4)), dim3(256), 0, as_stream(stream), x_adv, g, x0, n, hw, alpha,
                           eps3[0], eps3[1], eps3[2], lo3[0], lo3[1], lo3[2], hi3[0], hi3[1], hi3[2]);
    else
        hipLaunchKernelGGL(pgd_step_kernel<false>, dim3(grid_for(n)), dim3(256), 0, as_stream(stream), x_adv, g, x0, n, hw, alpha,
                           eps3[0], eps3[1], eps3[2], lo3[0], lo3[1], lo3[2], hi3[0], hi3[1], hi3[2]);
    MUMPY_CHECK_LAUNCH("pgd_step");
    return 0;
}
