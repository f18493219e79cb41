// input_warp.hip — the training input stage with the interpolating augmentations (include/mumpy_hip_ext4.h): uint8 clips -> augmented,
// normalized fp32 clips + 0/1 targets, one launch for a batch whose clips mix three modes.
// input_stage.hip runs the reference's augmentations that permute pixels.  Its other two shape operations interpolate on the L x L canvas
// that those permutations produce: RandomScaleCrop (utils/randaugment.py:398-428: Pillow's CUBIC upscale of 8-bit images, a crop box,
// NEAREST back) and RandomRotate (randaugment.py:434-474: cv2.warpAffine's bilinear rotation, a centre crop).  The host
// (mumpy_hip/augment.py) folds each into per-clip rows: mode 1 reads 4 x 4 canvas pixels through fixed-point taps, horizontal pass then
// vertical pass with Pillow's rounding; mode 2 reads 2 x 2 under an affine map in fp32; mode 0 is the gather of input_stage.hip.
//
// The work split is that of input_stage.hip: a block owns a TS x TS tile of output pixels of one frame (all three channels) or of one
// clip's target, thread (y, x4) of it makes one 16-byte store per channel, and the swap bit and the mode are uniform over a block (one
// clip), so no path diverges inside a wave.  A canvas pixel (Y, X) sits at source offset rowpart(Y) + colpart(X): the two tables are
// read once per canvas row / column a thread touches (4 + 16 entries in mode 1), not once per tap.  Every canvas coordinate is clamped
// to [0, L - 1] before it indexes a table and every table entry to the source before it indexes a frame: nothing a table, a mode word
// or an affine row holds moves a read outside frames / masks.
// Mode 0 keeps both forms of input_stage.hip (direct reads; swap clips through the LDS transpose).  Mode 1 is separable, and a tile of
// the rows the host builds touches at most 35 x 35 canvas pixels: the block stages that patch in LDS (lanes along the source row,
// swap clips too), runs the horizontal pass once per patch row and output column into LDS, and a thread's vertical pass reads 4 dwords
// per channel.  Read directly (cubic4, kept for tables whose taps span more than the patch: their content is not validated) a thread
// made 192 single-byte global loads and an all-mode-1 launch took 3.1x as long.  Mode 2 reads the source directly, also for swap
// clips, where a wave's loads then walk source rows.  Measurements: profiles/augment_warp.md.
#include "common.h"
#include "../../include/mumpy_hip_ext4.h"
using namespace mumpy;

namespace {

constexpr int TS = 32, TROW = TS + 4;
constexpr int PR = 40, PROW = PR + 4;    // the staged canvas patch of mode 1: PR x PR pixels, rows of 11 dwords
constexpr int PREC = 22;                 // Pillow's PRECISION_BITS

__device__ __forceinline__ int clampr(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }
__device__ __forceinline__ int clip8(int v) { return clampr(v, 0, 255); }

// The canvas of one clip read from one source plane (a frame: nch = 3 interleaved channels; a mask: nch = 1).
struct Canvas {
    const uint8_t* src;
    const int32_t *ta, *tb;
    int Hs, Ws, L, nch, sw;
    // pixel offsets (before * nch) of canvas row Y / column X; any int is accepted
    __device__ __forceinline__ int rowpart(int Y) const {
        Y = clampr(Y, 0, L - 1);
        return sw ? clampr(tb[Y], 0, Ws - 1) : clampr(ta[Y], 0, Hs - 1) * Ws;
    }
    __device__ __forceinline__ int colpart(int X) const {
        X = clampr(X, 0, L - 1);
        return sw ? clampr(ta[X], 0, Hs - 1) * Ws : clampr(tb[X], 0, Ws - 1);
    }
};

// Mode 1: pixels (y, x .. x + 3) -> w[ch], pixel k in byte k.  The sums are formed in uint32 (they wrap, as the header says, instead of
// overflowing a signed int on tables nobody validated) and shifted as int32.
__device__ __forceinline__ void cubic4(const Canvas& cv, const int32_t* __restrict__ py, const int32_t* __restrict__ px,
                                       const int32_t* __restrict__ cy, const int32_t* __restrict__ cx, int y, int x, uint32_t w[3]) {
    const int L = cv.L;
    const int4 cyv = *reinterpret_cast<const int4*>(cy + 4 * (int64_t)y);
    const int4 px4 = *reinterpret_cast<const int4*>(px + x);
    const int y0 = clampr(py[y], -4, L);                     // clampL(pos + i) is unchanged by this, and pos + i cannot overflow
    int P[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) P[j] = cv.rowpart(y0 + j);
    const int pxs[4] = {px4.x, px4.y, px4.z, px4.w};
    const uint32_t cys[4] = {(uint32_t)cyv.x, (uint32_t)cyv.y, (uint32_t)cyv.z, (uint32_t)cyv.w};
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int4 cxv = *reinterpret_cast<const int4*>(cx + 4 * (int64_t)(x + k));
        const uint32_t cxs[4] = {(uint32_t)cxv.x, (uint32_t)cxv.y, (uint32_t)cxv.z, (uint32_t)cxv.w};
        const int x0 = clampr(pxs[k], -4, L);
        int Q[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) Q[i] = cv.colpart(x0 + i);
#pragma unroll
        for (int ch = 0; ch < 3; ++ch) {
            if (ch < cv.nch) {
                uint32_t acc = 1u << (PREC - 1);
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    uint32_t a = 1u << (PREC - 1);
#pragma unroll
                    for (int i = 0; i < 4; ++i) a += cxs[i] * (uint32_t)cv.src[(P[j] + Q[i]) * cv.nch + ch];
                    acc += cys[j] * (uint32_t)clip8((int32_t)a >> PREC);
                }
                w[ch] |= (uint32_t)clip8((int32_t)acc >> PREC) << (8 * k);
            }
        }
    }
}

// Mode 2: pixels (y, x .. x + 3) -> w[ch].  `in` is false for a NaN and for anything floorf could not turn into an index.
__device__ __forceinline__ void affine4(const Canvas& cv, const int32_t* __restrict__ py, const int32_t* __restrict__ px,
                                        const float* __restrict__ m, int y, int x, uint32_t w[3]) {
    const int L = cv.L;
    const float Lf = (float)L, wv = (float)py[y];
    const int4 px4 = *reinterpret_cast<const int4*>(px + x);
    const int pxs[4] = {px4.x, px4.y, px4.z, px4.w};
    const float m00 = m[0], m01 = m[1], m02 = m[2], m10 = m[3], m11 = m[4], m12 = m[5];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const float u = (float)pxs[k];
        const float sx = m00 * u + m01 * wv + m02, sy = m10 * u + m11 * wv + m12;
        const bool in = sx > -1.0f && sx < Lf && sy > -1.0f && sy < Lf;
        const float fx0 = in ? floorf(sx) : 0.0f, fy0 = in ? floorf(sy) : 0.0f;
        const int x0 = (int)fx0, y0 = (int)fy0;              // in [-1, L - 1]
        const float fx = in ? sx - fx0 : 0.0f, fy = in ? sy - fy0 : 0.0f;
        const bool vx0 = in && x0 >= 0, vx1 = in && x0 + 1 <= L - 1, vy0 = in && y0 >= 0, vy1 = in && y0 + 1 <= L - 1;
        const int P0 = cv.rowpart(y0), P1 = cv.rowpart(y0 + 1), Q0 = cv.colpart(x0), Q1 = cv.colpart(x0 + 1);
#pragma unroll
        for (int ch = 0; ch < 3; ++ch) {
            if (ch < cv.nch) {
                const float p00 = vy0 && vx0 ? (float)cv.src[(P0 + Q0) * cv.nch + ch] : 0.0f;
                const float p01 = vy0 && vx1 ? (float)cv.src[(P0 + Q1) * cv.nch + ch] : 0.0f;
                const float p10 = vy1 && vx0 ? (float)cv.src[(P1 + Q0) * cv.nch + ch] : 0.0f;
                const float p11 = vy1 && vx1 ? (float)cv.src[(P1 + Q1) * cv.nch + ch] : 0.0f;
                const float blend = (1.0f - fy) * ((1.0f - fx) * p00 + fx * p01) + fy * ((1.0f - fx) * p10 + fx * p11);
                w[ch] |= (uint32_t)clip8((int)(blend + 0.5f)) << (8 * k);
            }
        }
    }
}

// Work units [0, nframes * nt^2): tile (ty, tx) of frame pl; the rest: tile (ty, tx) of the target of clip pl - nframes.
__global__ __launch_bounds__(256) void augment_warp_u8_kernel(const uint8_t* __restrict__ frames, const uint8_t* __restrict__ masks,
                                                              float* __restrict__ out, float* __restrict__ target,
                                                              const int32_t* __restrict__ tab_a, const int32_t* __restrict__ tab_b,
                                                              const int32_t* __restrict__ swap, const int32_t* __restrict__ mode,
                                                              const int32_t* __restrict__ pos_y, const int32_t* __restrict__ pos_x,
                                                              const int32_t* __restrict__ coef_y, const int32_t* __restrict__ coef_x,
                                                              const float* __restrict__ affine, int64_t nframes, int64_t units, int T,
                                                              int64_t nmasks, int Hs, int Ws, int L, int nt, float m0, float m1, float m2,
                                                              float s0, float s1, float s2) {
    __shared__ __attribute__((aligned(16))) uint8_t tile[3][PR][TROW];          // mode 0: the transposed tile; mode 1: the horizontal pass
    __shared__ uint8_t patch[3][PR][PROW];                                       // mode 1: the canvas patch under the tile's taps
    __shared__ int span[4];                                                      // mode 1: min / max of the tile's pos_y, pos_x
    const int tid = threadIdx.x;
    const int64_t hw = (int64_t)Hs * Ws;                     // 3 * hw < 2^31 (the entry's range check): offsets inside a frame are ints
    for (int64_t u = blockIdx.x; u < units; u += gridDim.x) {
        const int64_t pl = u / (nt * nt);
        const int tu = (int)(u - pl * (nt * nt));
        const int Y0 = (tu / nt) * TS, X0 = (tu % nt) * TS;
        const bool is_frame = pl < nframes;
        const int64_t c = is_frame ? pl / T : pl - nframes;
        const int nch = is_frame ? 3 : 1;
        float* dst = is_frame ? out + pl * 3 * (int64_t)L * L : target + c * (int64_t)L * L;
        const Canvas cv = {is_frame ? frames + pl * hw * 3 : masks + (c % nmasks) * hw, tab_a + c * L, tab_b + c * L, Hs, Ws, L, nch,
                           swap[c] & 1};
        const int md = mode[c] & 3;
        const bool staged = cv.sw && md != 1 && md != 2;     // mode 0 (and 3) of a swap clip: the LDS transpose of input_stage.hip
        if (staged) {
            for (int idx = tid; idx < TS * TS; idx += 256) {
                const int yl = idx % TS, xl = idx / TS;
                const int y = Y0 + yl, x = X0 + xl;
                if (y < L && x < L) {
                    const uint8_t* p = cv.src + (cv.rowpart(y) + cv.colpart(x)) * nch;
                    tile[0][yl][xl] = p[0];
                    if (is_frame) { tile[1][yl][xl] = p[1]; tile[2][yl][xl] = p[2]; }
                }
            }
            __syncthreads();
        }
        // Mode 1 through LDS when the tile's taps fit a PR x PR patch of the canvas -- always, for the rows scale_crop_params builds
        // (32 output pixels span at most 32 canvas pixels + 3 taps); tables that span more take the direct form, cubic4.
        const int32_t *py = pos_y + c * L, *px = pos_x + c * L;
        const int32_t *cy = coef_y + c * 4 * (int64_t)L, *cx = coef_x + c * 4 * (int64_t)L;
        bool patched = false;
        int r0 = 0;
        if (md == 1) {
            if (tid < 64) {                                  // wave 0: lanes 0..31 the tile's pos_y, lanes 32..63 its pos_x
                const int t = tid & 31, base = tid < 32 ? Y0 : X0;
                const int v = clampr((tid < 32 ? py : px)[base + t < L ? base + t : base], -4, L);
                int lo = v, hi = v;
                for (int o = 16; o; o >>= 1) {
                    lo = min(lo, __shfl_xor(lo, o));
                    hi = max(hi, __shfl_xor(hi, o));
                }
                if (t == 0) { span[tid < 32 ? 0 : 2] = lo; span[tid < 32 ? 1 : 3] = hi; }
            }
            __syncthreads();
            r0 = clampr(span[0], 0, L - 1);
            const int c0 = clampr(span[2], 0, L - 1);
            const int nr = clampr(span[1] + 3, 0, L - 1) - r0 + 1, nc = clampr(span[3] + 3, 0, L - 1) - c0 + 1;
            patched = nr <= PR && nc <= PR;
            if (patched) {
                const int na = cv.sw ? nr : nc;              // lanes walk the source row: canvas columns, or canvas rows of a swap clip
                for (int idx = tid; idx < nr * nc; idx += 256) {
                    const int a = idx % na, b = idx / na;
                    const int r = cv.sw ? a : b, q = cv.sw ? b : a;
                    const uint8_t* p = cv.src + (cv.rowpart(r0 + r) + cv.colpart(c0 + q)) * nch;
                    patch[0][r][q] = p[0];
                    if (is_frame) { patch[1][r][q] = p[1]; patch[2][r][q] = p[2]; }
                }
                __syncthreads();
                const int xl = tid & 31, xo = X0 + xl;       // the horizontal pass: thread -> output column xl, patch rows tid / 32 + 8n
                if (xo < L) {
                    const int4 cxv = *reinterpret_cast<const int4*>(cx + 4 * (int64_t)xo);
                    const uint32_t cxs[4] = {(uint32_t)cxv.x, (uint32_t)cxv.y, (uint32_t)cxv.z, (uint32_t)cxv.w};
                    const int x0 = clampr(px[xo], -4, L);
                    int q[4];                                // in [0, nc): c0 <= clampL(x0 + i) <= clampL(max + 3), clampL being monotone
#pragma unroll
                    for (int i = 0; i < 4; ++i) q[i] = clampr(x0 + i, 0, L - 1) - c0;
                    for (int r = tid >> 5; r < nr; r += 8) {
                        for (int ch = 0; ch < nch; ++ch) {
                            uint32_t a = 1u << (PREC - 1);
#pragma unroll
                            for (int i = 0; i < 4; ++i) a += cxs[i] * (uint32_t)patch[ch][r][q[i]];
                            tile[ch][r][xl] = (uint8_t)clip8((int32_t)a >> PREC);
                        }
                    }
                }
                __syncthreads();
            }
        }
        const int yl = tid >> 3, x4l = tid & 7;
        const int y = Y0 + yl, x = X0 + 4 * x4l;
        if (y < L && x < L) {                                // L % 4 == 0: a group of 4 pixels is inside or outside as a whole
            uint32_t w[3] = {0u, 0u, 0u};                    // per channel the 4 values, pixel k in byte k
            if (patched) {                                   // the vertical pass: 4 rows of the horizontal one, 4 pixels per dword
                const int4 cyv = *reinterpret_cast<const int4*>(cy + 4 * (int64_t)y);
                const uint32_t cys[4] = {(uint32_t)cyv.x, (uint32_t)cyv.y, (uint32_t)cyv.z, (uint32_t)cyv.w};
                const int y0 = clampr(py[y], -4, L);
                for (int ch = 0; ch < nch; ++ch) {
                    uint32_t h[4];
#pragma unroll
                    for (int j = 0; j < 4; ++j)
                        h[j] = *reinterpret_cast<const uint32_t*>(&tile[ch][clampr(y0 + j, 0, L - 1) - r0][4 * x4l]);
#pragma unroll
                    for (int k = 0; k < 4; ++k) {
                        uint32_t acc = 1u << (PREC - 1);
#pragma unroll
                        for (int j = 0; j < 4; ++j) acc += cys[j] * ((h[j] >> (8 * k)) & 255u);
                        w[ch] |= (uint32_t)clip8((int32_t)acc >> PREC) << (8 * k);
                    }
                }
            } else if (md == 1) {
                cubic4(cv, py, px, cy, cx, y, x, w);
            } else if (md == 2) {
                affine4(cv, py, px, affine + c * 8, y, x, w);
            } else if (staged) {
                for (int ch = 0; ch < nch; ++ch) w[ch] = *reinterpret_cast<const uint32_t*>(&tile[ch][yl][4 * x4l]);
            } else {         // one source row
                const int row = cv.rowpart(y);
                const int4 b = *reinterpret_cast<const int4*>(cv.tb + x);
                const int p0 = (row + clampr(b.x, 0, Ws - 1)) * nch, p1 = (row + clampr(b.y, 0, Ws - 1)) * nch;
                const int p2 = (row + clampr(b.z, 0, Ws - 1)) * nch, p3 = (row + clampr(b.w, 0, Ws - 1)) * nch;
                for (int ch = 0; ch < nch; ++ch)
                    w[ch] = cv.src[p0 + ch] | (cv.src[p1 + ch] << 8) | (cv.src[p2 + ch] << 16) | ((uint32_t)cv.src[p3 + ch] << 24);
            }
            for (int ch = 0; ch < nch; ++ch) {
                f32x4 v;
                if (is_frame) {
                    const float mean = ch == 0 ? m0 : (ch == 1 ? m1 : m2);
                    const float stdv = ch == 0 ? s0 : (ch == 1 ? s1 : s2);
#pragma unroll
                    for (int k = 0; k < 4; ++k) v[k] = ((float)((w[ch] >> (8 * k)) & 255u) / 255.0f - mean) / stdv;
                } else {
#pragma unroll
                    for (int k = 0; k < 4; ++k) v[k] = ((w[ch] >> (8 * k)) & 255u) > 0 ? 1.0f : 0.0f;
                }
                *reinterpret_cast<f32x4*>(dst + ((int64_t)ch * L + y) * L + x) = v;
            }
        }
        if (staged || md == 1) __syncthreads();              // the next unit of this block reuses the tile, the patch and span
    }
}

}  // namespace

extern "C" int mumpy_augment_warp_u8_fwd(const uint8_t* frames, const uint8_t* masks, float* out, float* target,
                                         const int32_t* tab_a, const int32_t* tab_b, const int32_t* swap, const int32_t* mode,
                                         const int32_t* pos_y, const int32_t* pos_x, const int32_t* coef_y, const int32_t* coef_x,
                                         const float* affine, int64_t nclips, int T, int64_t nmasks, int Hs, int Ws, int L,
                                         const float* mean3, const float* std3, void* stream) {
    MUMPY_REQUIRE(frames && out && tab_a && tab_b && swap && mode && pos_y && pos_x && coef_y && coef_x && affine && mean3 && std3,
                  MUMPY_ENULL, "augment_warp_u8: null pointer");
    MUMPY_REQUIRE((masks == nullptr) == (target == nullptr), MUMPY_ENULL,
                  "augment_warp_u8: masks and target go together (both given or both null)");
    MUMPY_REQUIRE(nclips >= 0 && T >= 1 && Hs >= 1 && Ws >= 1 && L >= 4 && L % 4 == 0, MUMPY_EINVAL,
                  "augment_warp_u8: bad sizes nclips=%lld T=%d, %dx%d -> %dx%d (the output side must be a multiple of 4)",
                  (long long)nclips, T, Hs, Ws, L, L);
    MUMPY_REQUIRE(!masks || (nmasks >= 1 && nclips % nmasks == 0), MUMPY_EINVAL,
                  "augment_warp_u8: nclips=%lld must be a multiple of nmasks=%lld >= 1", (long long)nclips, (long long)nmasks);
    MUMPY_REQUIRE(std3[0] != 0.f && std3[1] != 0.f && std3[2] != 0.f, MUMPY_EINVAL, "augment_warp_u8: zero std");
    MUMPY_REQUIRE(aligned16(out) && aligned16(target) && aligned16(tab_a) && aligned16(tab_b) && aligned16(pos_y) && aligned16(pos_x) &&
                      aligned16(coef_y) && aligned16(coef_x),
                  MUMPY_EALIGN, "augment_warp_u8: out, target, tab_a, tab_b, pos_y, pos_x, coef_y and coef_x must be 16-byte aligned");
    constexpr int64_t LIM = (int64_t)1 << 31;
    MUMPY_REQUIRE(nclips < LIM && nclips * (int64_t)T < LIM, MUMPY_ERANGE, "augment_warp_u8: nclips*T=%lld*%d frames is 2^31 or more",
                  (long long)nclips, T);
    MUMPY_REQUIRE(3 * (int64_t)Hs * Ws < LIM && 3 * (int64_t)L * L < LIM, MUMPY_ERANGE,
                  "augment_warp_u8: 3*%d*%d or 3*%d*%d is 2^31 or more (offsets inside a frame are 32-bit)", Hs, Ws, L, L);
    if (nclips == 0) return 0;
    const int nt = (L + TS - 1) / TS;
    const int64_t nframes = nclips * T, units = (nframes + (masks ? nclips : 0)) * nt * nt;          // < 2^32 * 2^20
    const unsigned grid = (unsigned)(units < 16384 ? units : 16384);
    hipLaunchKernelGGL(augment_warp_u8_kernel, dim3(grid), dim3(256), 0, as_stream(stream), frames, masks, out, target, tab_a, tab_b, swap,
                       mode, pos_y, pos_x, coef_y, coef_x, affine, nframes, units, T, nmasks, Hs, Ws, L, nt, mean3[0], mean3[1],
                       mean3[2], std3[0], std3[1], std3[2]);
    MUMPY_CHECK_LAUNCH("augment_warp_u8");
    return 0;
}
