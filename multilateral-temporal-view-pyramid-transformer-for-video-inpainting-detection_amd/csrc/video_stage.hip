// video_stage.hip — the device side of whole-video inference (include/mumpy_hip_ext5.h; host: mumpy_hip/video.py).
// The reference runs a video as one clip per frame: the frame and its T // 2 neighbours on each side, clamped at the ends
// (dataloaders/universaldataloader.py:41-48), every frame resized and normalised once per clip it appears in, by CPU workers; it keeps
// the centre frame's mask, writes mask * 255 (test.py:86-111) and scores each frame (measure.py:57-62, 86-89).  Here the video is
// uploaded once and three launches bracket the forward:
//   clip_window_u8_kernel   the clips of a batch, gathered through a (nclips, T) frame table out of the resident video: the body of
//                           resize_normalize_u8_kernel (norm.hip) with one more indirection; the pixel expression is shared (u8_pixel.h);
//   mask_score_u8_kernel    the batch's masks into the per-frame bank as 0 / 255 and, per frame, the four counts of the metrics;
//   frame_metrics_kernel    F1 / IoU of the counts in fp64, summed in a fixed order.
// The last two move ~50 KB per clip and a few KB per video: one workgroup per clip / one workgroup, bounded by launch latency.
#include "common.h"
#include "u8_pixel.h"
#include "frame_metric.h"
#include "../../include/mumpy_hip_ext5.h"
using namespace mumpy;

namespace {

// The clamps are unconditional: the tables are device memory that nobody validated.
__device__ __forceinline__ int clampi(int v, int hi) { return v < 0 ? 0 : (v > hi ? hi : v); }

// A thread converts 4 consecutive pixels of one channel of one clip frame: one 16-byte store, as in resize_normalize_u8_kernel.
__global__ __launch_bounds__(256) void clip_window_u8_kernel(const uint8_t* __restrict__ src, float* __restrict__ dst,
                                                             const int32_t* __restrict__ frame_idx, const int32_t* __restrict__ ytab,
                                                             const int32_t* __restrict__ xtab, int64_t nout, int nframes, int Hs, int Ws,
                                                             int H, int W, float m0, float m1, float m2, float s0, float s1, float s2) {
    const int q4 = W >> 2;
    const int64_t total = nout * 3 * H * q4;                 // nout = nclips * T < 2^31, 3 * H * W < 2^31: below 2^62
    const int64_t fsz = (int64_t)Hs * Ws * 3;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
        const int x4 = (int)(i % q4);
        int64_t t = i / q4;
        const int y = (int)(t % H); t /= H;
        const int ch = (int)(t % 3);
        const int64_t f = t / 3;                             // output frame c * T + t
        const float mean = ch == 0 ? m0 : (ch == 1 ? m1 : m2);
        const float stdv = ch == 0 ? s0 : (ch == 1 ? s1 : s2);
        const int sf = clampi(frame_idx[f], nframes - 1);
        const uint8_t* row = src + sf * fsz + (clampi(ytab[y], Hs - 1) * Ws) * 3 + ch;          // 3 * Hs * Ws < 2^31
        int4 xi = *reinterpret_cast<const int4*>(xtab + 4 * x4);
        xi.x = clampi(xi.x, Ws - 1); xi.y = clampi(xi.y, Ws - 1); xi.z = clampi(xi.z, Ws - 1); xi.w = clampi(xi.w, Ws - 1);
        *reinterpret_cast<f32x4*>(dst + ((f * 3 + ch) * H + y) * (int64_t)W + 4 * x4) = normalize_u8_gather4(row, xi, mean, stdv);
    }
}

// 0x80 in every byte of w that is not zero
__device__ __forceinline__ uint32_t nonzero_bytes(uint32_t w) { return (((w & 0x7f7f7f7fu) + 0x7f7f7f7fu) | w) & 0x80808080u; }

__device__ __forceinline__ int wave_sum_i(int v) {
#pragma unroll
    for (int s = 1; s < WAVE; s <<= 1) v += __shfl_xor(v, s);
    return v;
}

// One workgroup per clip (a grid-stride walk only past 65536 clips); dest[c] is uniform over the workgroup, so a dropped clip is
// skipped as a whole, before any barrier.
__device__ __forceinline__ void mask_score_clip(const uint8_t* __restrict__ mask, const uint8_t* __restrict__ gt,
                                                const int32_t* __restrict__ dest, uint8_t* __restrict__ bank,
                                                int32_t* __restrict__ counts, int c, int tid, int npix, int nbank, int (*red)[4]) {
    const int d = dest[c];
    if (d < 0 || d >= nbank) return;
    const uint4* m4 = reinterpret_cast<const uint4*>(mask + (int64_t)c * npix);
    uint4* b4 = reinterpret_cast<uint4*>(bank + (int64_t)d * npix);
    const uint4* g4 = gt ? reinterpret_cast<const uint4*>(gt + (int64_t)d * npix) : nullptr;
    int inter = 0, sp = 0, sg = 0, uni = 0;
    for (int i = tid; i < (npix >> 4); i += 256) {
        const uint4 m = m4[i];
        const uint32_t p[4] = {nonzero_bytes(m.x), nonzero_bytes(m.y), nonzero_bytes(m.z), nonzero_bytes(m.w)};
        uint4 o;
        o.x = (p[0] >> 7) * 255u; o.y = (p[1] >> 7) * 255u; o.z = (p[2] >> 7) * 255u; o.w = (p[3] >> 7) * 255u;      // 0x01 -> 0xff per byte
        b4[i] = o;
        if (g4) {
            const uint4 gv = g4[i];
            const uint32_t g[4] = {nonzero_bytes(gv.x), nonzero_bytes(gv.y), nonzero_bytes(gv.z), nonzero_bytes(gv.w)};
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                inter += __popc(p[k] & g[k]); sp += __popc(p[k]); sg += __popc(g[k]); uni += __popc(p[k] | g[k]);
            }
        }
    }
    if (!g4) return;                                         // (uniform: a kernel argument)
    inter = wave_sum_i(inter); sp = wave_sum_i(sp); sg = wave_sum_i(sg); uni = wave_sum_i(uni);
    if ((tid & (WAVE - 1)) == 0) {
        int* r = red[tid / WAVE];
        r[0] = inter; r[1] = sp; r[2] = sg; r[3] = uni;
    }
    __syncthreads();
    if (tid < 4) counts[(int64_t)d * 4 + tid] = red[0][tid] + red[1][tid] + red[2][tid] + red[3][tid];
    __syncthreads();                                         // the next clip of this workgroup reuses red
}

__global__ __launch_bounds__(256) void mask_score_u8_kernel(const uint8_t* __restrict__ mask, const uint8_t* __restrict__ gt,
                                                            const int32_t* __restrict__ dest, uint8_t* __restrict__ bank,
                                                            int32_t* __restrict__ counts, int nclips, int npix, int nbank) {
    __shared__ int red[4][4];
    const int tid = threadIdx.x;
    for (int c = blockIdx.x; c < nclips; c += gridDim.x) mask_score_clip(mask, gt, dest, bank, counts, c, tid, npix, nbank, red);
}

// One workgroup: thread k adds frames k, k + 256, ... in order, then a fixed tree over the 256 partial sums.
__global__ __launch_bounds__(256) void frame_metrics_kernel(const int32_t* __restrict__ counts, int nscored, double eps_g,
                                                            double* __restrict__ acc3, int accumulate) {
    __shared__ double red[256][2];
    const int tid = threadIdx.x;
    double f1 = 0.0, iou = 0.0;
    for (int f = tid; f < nscored; f += 256) {
        const int32_t* c = counts + (int64_t)f * 4;
        const double inter = (double)c[0], sp = (double)c[1], sg = (double)c[2], uni = (double)c[3];
        double ff, fi;
        frame_f1_iou(inter, sp, sg, uni, eps_g, ff, fi);     // eps_g = 1e-6 * npix (frame_metric.h)
        f1 += ff;
        iou += fi;
    }
    red[tid][0] = f1; red[tid][1] = iou;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if (tid < s) { red[tid][0] += red[tid + s][0]; red[tid][1] += red[tid + s][1]; }
        __syncthreads();
    }
    if (tid == 0) {
        const double n = (double)nscored;
        if (accumulate) { acc3[0] += red[0][0]; acc3[1] += red[0][1]; acc3[2] += n; }
        else { acc3[0] = red[0][0]; acc3[1] = red[0][1]; acc3[2] = n; }
    }
}

constexpr int64_t LIM = (int64_t)1 << 31;

}  // namespace

extern "C" int mumpy_clip_window_u8_fwd(const uint8_t* frames, float* out, const int32_t* frame_idx, const int32_t* ytab,
                                        const int32_t* xtab, int64_t nclips, int T, int64_t nframes, int Hs, int Ws, int H, int W,
                                        const float* mean3, const float* std3, void* stream) {
    MUMPY_REQUIRE(frames && out && frame_idx && ytab && xtab && mean3 && std3, MUMPY_ENULL, "clip_window_u8: null pointer");
    MUMPY_REQUIRE(nclips >= 0 && T >= 1 && nframes >= 1 && Hs >= 1 && Ws >= 1 && H >= 1 && W >= 1 && W % 4 == 0, MUMPY_EINVAL,
                  "clip_window_u8: bad sizes nclips=%lld T=%d nframes=%lld, %dx%d -> %dx%d (the output width must be a multiple of 4)",
                  (long long)nclips, T, (long long)nframes, Hs, Ws, H, W);
    MUMPY_REQUIRE(std3[0] != 0.f && std3[1] != 0.f && std3[2] != 0.f, MUMPY_EINVAL, "clip_window_u8: zero std");
    MUMPY_REQUIRE(aligned16(out) && aligned16(xtab), MUMPY_EALIGN, "clip_window_u8: out and xtab must be 16-byte aligned");
    MUMPY_REQUIRE(nframes < LIM, MUMPY_ERANGE, "clip_window_u8: nframes=%lld is 2^31 or more (frame_idx is 32-bit)", (long long)nframes);
    MUMPY_REQUIRE(nclips < LIM && nclips * (int64_t)T < LIM, MUMPY_ERANGE, "clip_window_u8: nclips*T=%lld*%d frames is 2^31 or more",
                  (long long)nclips, T);
    MUMPY_REQUIRE(3 * (int64_t)Hs * Ws < LIM && 3 * (int64_t)H * W < LIM, MUMPY_ERANGE,
                  "clip_window_u8: 3*%d*%d or 3*%d*%d is 2^31 or more (offsets inside a frame are 32-bit)", Hs, Ws, H, W);
    if (nclips == 0) return 0;
    const int64_t nout = nclips * T, total = nout * 3 * (int64_t)H * (W / 4);
    int64_t grid = (total + 255) / 256;
    if (grid > 4096) grid = 4096;
    hipLaunchKernelGGL(clip_window_u8_kernel, dim3((unsigned)grid), dim3(256), 0, as_stream(stream), frames, out, frame_idx, ytab, xtab,
                       nout, (int)nframes, Hs, Ws, H, W, mean3[0], mean3[1], mean3[2], std3[0], std3[1], std3[2]);
    MUMPY_CHECK_LAUNCH("clip_window_u8");
    return 0;
}

extern "C" int mumpy_mask_score_u8_fwd(const uint8_t* mask, const uint8_t* gt, const int32_t* dest, uint8_t* bank, int32_t* counts,
                                       int64_t nclips, int64_t npix, int64_t nbank, void* stream) {
    MUMPY_REQUIRE(mask && dest && bank, MUMPY_ENULL, "mask_score_u8: null pointer");
    MUMPY_REQUIRE((gt == nullptr) == (counts == nullptr), MUMPY_ENULL,
                  "mask_score_u8: gt and counts go together (both given or both null)");
    MUMPY_REQUIRE(nclips >= 0 && npix >= 1 && npix % 16 == 0 && nbank >= 1, MUMPY_EINVAL,
                  "mask_score_u8: bad sizes nclips=%lld npix=%lld nbank=%lld (npix must be a multiple of 16)", (long long)nclips,
                  (long long)npix, (long long)nbank);
    MUMPY_REQUIRE(aligned16(mask) && aligned16(bank) && aligned16(gt), MUMPY_EALIGN,
                  "mask_score_u8: mask, bank and gt must be 16-byte aligned");
    MUMPY_REQUIRE(nclips < LIM && npix < LIM && nbank < LIM, MUMPY_ERANGE,
                  "mask_score_u8: nclips=%lld, npix=%lld or nbank=%lld is 2^31 or more (dest and the counts are 32-bit)",
                  (long long)nclips, (long long)npix, (long long)nbank);
    if (nclips == 0) return 0;
    hipLaunchKernelGGL(mask_score_u8_kernel, dim3((unsigned)(nclips < 65536 ? nclips : 65536)), dim3(256), 0, as_stream(stream), mask, gt, dest, bank, counts,
                       (int)nclips, (int)npix, (int)nbank);
    MUMPY_CHECK_LAUNCH("mask_score_u8");
    return 0;
}

extern "C" int mumpy_frame_metrics_fwd(const int32_t* counts, int64_t nscored, int64_t npix, double* acc3, int accumulate,
                                       void* stream) {
    MUMPY_REQUIRE(counts && acc3, MUMPY_ENULL, "frame_metrics: null pointer");
    MUMPY_REQUIRE(nscored >= 0 && npix >= 1, MUMPY_EINVAL, "frame_metrics: bad sizes nscored=%lld npix=%lld", (long long)nscored,
                  (long long)npix);
    MUMPY_REQUIRE((reinterpret_cast<uintptr_t>(acc3) & 7u) == 0, MUMPY_EALIGN, "frame_metrics: acc3 must be 8-byte aligned");
    MUMPY_REQUIRE(nscored < LIM && npix < LIM, MUMPY_ERANGE, "frame_metrics: nscored=%lld or npix=%lld is 2^31 or more",
                  (long long)nscored, (long long)npix);
    hipLaunchKernelGGL(frame_metrics_kernel, dim3(1), dim3(256), 0, as_stream(stream), counts, (int)nscored, 1e-6 * (double)npix, acc3,
                       accumulate != 0 ? 1 : 0);
    MUMPY_CHECK_LAUNCH("frame_metrics");
    return 0;
}
