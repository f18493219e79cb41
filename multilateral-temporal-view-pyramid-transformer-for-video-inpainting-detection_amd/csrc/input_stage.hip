// input_stage.hip — the training input stage (include/mumpy_hip_ext3.h): uint8 clips -> augmented, normalized fp32 clips + 0/1 targets.
// The reference's loader resizes every frame with PIL NEAREST, applies one of its enabled augmentations (flips, 90-degree rotations,
// crop boxes resized back: utils/randaugment.py:113-127, 263-309, 515-539; universaldataset.py:101-120), then ToTensor + Normalize, and
// builds the target as mask > 0 (universaldataset.py:141-144).  All of these are index permutations of the source pixels; the host
// (mumpy_hip/augment.py) folds them into two per-clip tables of L entries and a swap bit, and this kernel is the gather of
// resize_normalize_u8_kernel (norm.hip) through them, with the same arithmetic in the same order.
//
// A block owns a TS x TS tile of output pixels of one frame (all three channels) or of one clip's target; thread (y, x4) of it makes
// one 16-byte store per channel.  The swap bit is uniform over a block (one clip), so the two paths never diverge inside a wave:
//   * without it the thread's 4 pixels lie in one source row and are read directly (the form of resize_normalize_u8_kernel);
//   * with it they lie in one source COLUMN -- read directly, every load instruction of a wave touches 64 different source rows, which
//     ran 1.6x - 1.9x longer than the other path -- so the tile goes through LDS: a thread loads whole pixels (3 channels from one
//     place) with lanes walking the output y, i.e. the source column, fastest, so a wave reads runs of one source row; the bytes are
//     stored as tile[ch][y][x] (row stride TS + 4 bytes = 9 dwords: a wave writing a column hits 32 different banks), and after the
//     barrier thread (y, x4) reads one dword per channel = its 4 pixels.
// Measurements of both forms: profiles/augment_input.md.
#include "common.h"
#include "../../include/mumpy_hip_ext3.h"
using namespace mumpy;

namespace {

constexpr int TS = 32, TROW = TS + 4;

// The clamp is unconditional: the tables are device memory that nobody validated.
__device__ __forceinline__ int clampi(int v, int hi) { return v < 0 ? 0 : (v > hi ? hi : v); }

// Work units [0, nframes * nt^2): tile (ty, tx) of frame pl; the rest: tile (ty, tx) of the target of clip pl - nframes.
__global__ __launch_bounds__(256) void augment_stage_u8_kernel(const uint8_t* __restrict__ frames, const uint8_t* __restrict__ masks,
                                                               float* __restrict__ out, float* __restrict__ target,
                                                               const int32_t* __restrict__ tab_a, const int32_t* __restrict__ tab_b,
                                                               const int32_t* __restrict__ swap, int64_t nframes, int64_t units, int T,
                                                               int64_t nmasks, int Hs, int Ws, int L, int nt, float m0, float m1, float m2,
                                                               float s0, float s1, float s2) {
    __shared__ __attribute__((aligned(16))) uint8_t tile[3][TS][TROW];
    const int tid = threadIdx.x;
    const int64_t hw = (int64_t)Hs * Ws;                     // 3 * hw < 2^31 (the entry's range check): offsets inside a frame are ints
    for (int64_t u = blockIdx.x; u < units; u += gridDim.x) {
        const int64_t pl = u / (nt * nt);
        const int tu = (int)(u - pl * (nt * nt));
        const int Y0 = (tu / nt) * TS, X0 = (tu % nt) * TS;
        const bool is_frame = pl < nframes;
        const int64_t c = is_frame ? pl / T : pl - nframes;
        const int nch = is_frame ? 3 : 1;
        const uint8_t* src = is_frame ? frames + pl * hw * 3 : masks + (c % nmasks) * hw;
        float* dst = is_frame ? out + pl * 3 * (int64_t)L * L : target + c * (int64_t)L * L;
        const int sw = swap[c] & 1;
        const int32_t* ta = tab_a + c * L;
        const int32_t* tb = tab_b + c * L;
        if (sw) {            // i = x, j = y: stage the tile, lanes along y
            for (int idx = tid; idx < TS * TS; idx += 256) {
                const int yl = idx % TS, xl = idx / TS;
                const int y = Y0 + yl, x = X0 + xl;
                if (y < L && x < L) {
                    const uint8_t* p = src + (clampi(ta[x], Hs - 1) * Ws + clampi(tb[y], Ws - 1)) * nch;
                    tile[0][yl][xl] = p[0];
                    if (is_frame) { tile[1][yl][xl] = p[1]; tile[2][yl][xl] = p[2]; }
                }
            }
            __syncthreads();
        }
        const int yl = tid >> 3, x4l = tid & 7;
        const int y = Y0 + yl, x = X0 + 4 * x4l;
        if (y < L && x < L) {                                // L % 4 == 0: a group of 4 pixels is inside or outside as a whole
            int4 p = {0, 0, 0, 0};
            if (!sw) {       // i = y, j = x: one source row
                const int4 b = *reinterpret_cast<const int4*>(tb + x);
                const int row = clampi(ta[y], Hs - 1) * Ws;
                p.x = (row + clampi(b.x, Ws - 1)) * nch;
                p.y = (row + clampi(b.y, Ws - 1)) * nch;
                p.z = (row + clampi(b.z, Ws - 1)) * nch;
                p.w = (row + clampi(b.w, Ws - 1)) * nch;
            }
            for (int ch = 0; ch < nch; ++ch) {
                uint32_t w;                                  // the 4 source bytes, pixel k in byte k
                if (sw) w = *reinterpret_cast<const uint32_t*>(&tile[ch][yl][4 * x4l]);
                else w = src[p.x + ch] | (src[p.y + ch] << 8) | (src[p.z + ch] << 16) | ((uint32_t)src[p.w + ch] << 24);
                f32x4 v;
                if (is_frame) {
                    const float mean = ch == 0 ? m0 : (ch == 1 ? m1 : m2);
                    const float stdv = ch == 0 ? s0 : (ch == 1 ? s1 : s2);
#pragma unroll
                    for (int k = 0; k < 4; ++k) v[k] = ((float)((w >> (8 * k)) & 255u) / 255.0f - mean) / stdv;
                } else {
#pragma unroll
                    for (int k = 0; k < 4; ++k) v[k] = ((w >> (8 * k)) & 255u) > 0 ? 1.0f : 0.0f;
                }
                *reinterpret_cast<f32x4*>(dst + ((int64_t)ch * L + y) * L + x) = v;
            }
        }
        if (sw) __syncthreads();                             // the next unit of this block reuses the tile
    }
}

}  // namespace

extern "C" int mumpy_augment_stage_u8_fwd(const uint8_t* frames, const uint8_t* masks, float* out, float* target,
                                          const int32_t* tab_a, const int32_t* tab_b, const int32_t* swap,
                                          int64_t nclips, int T, int64_t nmasks, int Hs, int Ws, int L,
                                          const float* mean3, const float* std3, void* stream) {
    MUMPY_REQUIRE(frames && out && tab_a && tab_b && swap && mean3 && std3, MUMPY_ENULL, "augment_stage_u8: null pointer");
    MUMPY_REQUIRE((masks == nullptr) == (target == nullptr), MUMPY_ENULL,
                  "augment_stage_u8: masks and target go together (both given or both null)");
    MUMPY_REQUIRE(nclips >= 0 && T >= 1 && Hs >= 1 && Ws >= 1 && L >= 4 && L % 4 == 0, MUMPY_EINVAL,
                  "augment_stage_u8: bad sizes nclips=%lld T=%d, %dx%d -> %dx%d (the output side must be a multiple of 4)",
                  (long long)nclips, T, Hs, Ws, L, L);
    MUMPY_REQUIRE(!masks || (nmasks >= 1 && nclips % nmasks == 0), MUMPY_EINVAL,
                  "augment_stage_u8: nclips=%lld must be a multiple of nmasks=%lld >= 1", (long long)nclips, (long long)nmasks);
    MUMPY_REQUIRE(std3[0] != 0.f && std3[1] != 0.f && std3[2] != 0.f, MUMPY_EINVAL, "augment_stage_u8: zero std");
    MUMPY_REQUIRE(aligned16(out) && aligned16(target) && aligned16(tab_a) && aligned16(tab_b), MUMPY_EALIGN,
                  "augment_stage_u8: out, target, tab_a and tab_b must be 16-byte aligned");
    constexpr int64_t LIM = (int64_t)1 << 31;
    MUMPY_REQUIRE(nclips < LIM && nclips * (int64_t)T < LIM, MUMPY_ERANGE, "augment_stage_u8: nclips*T=%lld*%d frames is 2^31 or more",
                  (long long)nclips, T);
    MUMPY_REQUIRE(3 * (int64_t)Hs * Ws < LIM && 3 * (int64_t)L * L < LIM, MUMPY_ERANGE,
                  "augment_stage_u8: 3*%d*%d or 3*%d*%d is 2^31 or more (offsets inside a frame are 32-bit)", Hs, Ws, L, L);
    if (nclips == 0) return 0;
    const int nt = (L + TS - 1) / TS;
    const int64_t nframes = nclips * T, units = (nframes + (masks ? nclips : 0)) * nt * nt;          // < 2^32 * 2^20
    const unsigned grid = (unsigned)(units < 16384 ? units : 16384);
    hipLaunchKernelGGL(augment_stage_u8_kernel, dim3(grid), dim3(256), 0, as_stream(stream), frames, masks, out, target, tab_a, tab_b, swap,
                       nframes, units, T, nmasks, Hs, Ws, L, nt, mean3[0], mean3[1], mean3[2], std3[0], std3[1], std3[2]);
    MUMPY_CHECK_LAUNCH("augment_stage_u8");
    return 0;
}
