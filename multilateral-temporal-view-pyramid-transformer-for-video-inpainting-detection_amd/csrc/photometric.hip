// photometric.hip — the photometric half of the reference's augmentation file (utils/randaugment.py:89-110, 129-191) on uint8 frames
// that stay on the device (include/mumpy_photometric.h), bit for bit what Pillow computes.  mumpy_hip/photometric.py is the numpy
// statement and DESIGN.md ("Photometric operations") gives the arithmetic.
//
// Seven of the nine kinds are a 256-entry table per channel once the image's statistics are known, so the work is three launches:
//   photo_stats_kernel   per (image, slab of pixels): the three histograms in LDS (autocontrast, equalize) or the sum of the
//                        luminance (contrast), written as that slab's partial to the workspace; for sharpness a copy of the slab
//                        (the stencil of an in-place call reads the copy); any other kind returns after reading its kind
//   photo_table_kernel   per image, thread i owns table entry i: sums the slabs in their order (integers: any order gives the same)
//   photo_apply_kernel   per (image, chunk of 8192 pixels): gather through the LDS-staged table / color / sharpness / copy
// Pixels move as groups of 16 (48 bytes, three 16-byte accesses) when the image's base address allows it and as bytes when it does not
// (an odd-sized image inside a batch); a group starts on a pixel, so byte k of a group is channel k % 3 at compile time.
//
// FLOATS: Pillow's blend and its 3x3 filter round every product and every sum to float32 on their own, and ImageOps.autocontrast
// does the same in double.  The file is compiled with contraction off (Makefile) and says so again here; no expression below may
// become a fused multiply-add.
#include "common.h"
#include "../../include/mumpy_photometric.h"
using namespace mumpy;

#pragma clang fp contract(off)

namespace {

constexpr int64_t LIM31 = (int64_t)1 << 31;
constexpr int HW_MAX = 1 << 24;                          // 255 * 2^24 < 2^32: the luminance sum of one image fits a uint32
constexpr int TABLE_BYTES = 3 * 256;
constexpr int SLAB_WORDS = 3 * 256 + 4;                  // three histograms, the luminance sum, padding to 16 bytes
constexpr int SLAB_BYTES = SLAB_WORDS * 4;
constexpr int SLAB_MAX = 64;                             // slabs per image at most
constexpr int SLAB_GROUPS = 512;                         // ... of at least this many 16-pixel groups
constexpr int CHUNK_GROUPS = 512;                        // groups per workgroup iteration of the apply launch
constexpr int CHUNK_PIXELS = CHUNK_GROUPS * 16;

// 255.0 / d in IEEE double, as Python computes it: divided by the compiler, not on the device
struct InvTab { double v[256]; };
constexpr InvTab make_inv() {
    InvTab t{};
    for (int d = 1; d < 256; ++d) t.v[d] = 255.0 / d;
    return t;
}
__constant__ const InvTab INV255 = make_inv();

// ImageFilter.SMOOTH: (1 1 1 / 1 5 1 / 1 1 1) / 13, divided in float32
constexpr float K1 = 1.0f / 13.0f, K5 = 5.0f / 13.0f;

__device__ __forceinline__ int mini(int a, int b) { return a < b ? a : b; }
__device__ __forceinline__ int maxi(int a, int b) { return a > b ? a : b; }
__device__ __forceinline__ int luma(int r, int g, int b) { return (19595 * r + 38470 * g + 7471 * b + 32768) >> 16; }

// float -> byte as Pillow clips it: 0 if <= 0 (and for a NaN), 255 if >= 255, else truncated
__device__ __forceinline__ int clip8(float t) { return !(t > 0.0f) ? 0 : (t >= 255.0f ? 255 : (int)t); }

// Image.blend(degenerate, image, alpha): two float32 roundings.  For 0 <= alpha <= 1 Pillow truncates without clipping; t then lies
// between d and i, where clipping and truncating agree.
__device__ __forceinline__ int blend(int d, int i, float alpha) {
    const float prod = alpha * (float)(i - d);
    const float t = (float)d + prod;
    return clip8(t);
}

struct Row { int kind, value; };
__device__ __forceinline__ Row row_of(const int32_t* __restrict__ params, int64_t img) {
    const int4 p = *reinterpret_cast<const int4*>(params + img * 4);
    return {p.x, p.y};
}
__device__ __forceinline__ bool table_kind(int k) {
    return k == MUMPY_PHOTO_AUTOCONTRAST || k == MUMPY_PHOTO_INVERT || k == MUMPY_PHOTO_EQUALIZE || k == MUMPY_PHOTO_SOLARIZE ||
           k == MUMPY_PHOTO_POSTERIZE || k == MUMPY_PHOTO_CONTRAST || k == MUMPY_PHOTO_BRIGHTNESS;
}

// n <= 16 pixels (3 n bytes) at p <-> twelve dwords; `vec`: p is 16-byte aligned
__device__ __forceinline__ void load48(const uint8_t* p, int n, bool vec, uint32_t (&w)[12]) {
    if (vec && n == 16) {
        const uint4* q = reinterpret_cast<const uint4*>(p);
        const uint4 a = q[0], b = q[1], c = q[2];
        w[0] = a.x; w[1] = a.y; w[2] = a.z; w[3] = a.w; w[4] = b.x; w[5] = b.y; w[6] = b.z; w[7] = b.w;
        w[8] = c.x; w[9] = c.y; w[10] = c.z; w[11] = c.w;
        return;
    }
#pragma unroll
    for (int j = 0; j < 12; ++j) w[j] = 0;
#pragma unroll
    for (int k = 0; k < 48; ++k)
        if (k < 3 * n) w[k >> 2] |= (uint32_t)p[k] << (8 * (k & 3));
}
__device__ __forceinline__ void store48(uint8_t* p, int n, bool vec, const uint32_t (&w)[12]) {
    if (vec && n == 16) {
        uint4* q = reinterpret_cast<uint4*>(p);
        q[0] = make_uint4(w[0], w[1], w[2], w[3]);
        q[1] = make_uint4(w[4], w[5], w[6], w[7]);
        q[2] = make_uint4(w[8], w[9], w[10], w[11]);
        return;
    }
#pragma unroll
    for (int k = 0; k < 48; ++k)
        if (k < 3 * n) p[k] = (uint8_t)(w[k >> 2] >> (8 * (k & 3)));
}
#define BYTE_OF(w, k) (((w)[(k) >> 2] >> (8 * ((k) & 3))) & 255u)

__global__ __launch_bounds__(256) void photo_stats_kernel(const uint8_t* __restrict__ src, const int32_t* __restrict__ params,
                                                          uint32_t* __restrict__ slabs, uint8_t* __restrict__ copies,
                                                          int64_t copy_stride, int64_t units, int S, int gps, int HW) {
    __shared__ uint32_t h[SLAB_WORDS];
    const int G = (HW + 15) >> 4;
    for (int64_t u = blockIdx.x; u < units; u += gridDim.x) {
        const int64_t img = u / S;
        const int slab = (int)(u - img * S);
        const int kind = row_of(params, img).kind;                               // uniform over the block
        const bool hist = kind == MUMPY_PHOTO_AUTOCONTRAST || kind == MUMPY_PHOTO_EQUALIZE;
        const bool lsum = kind == MUMPY_PHOTO_CONTRAST, sharp = kind == MUMPY_PHOTO_SHARPNESS;
        if (!(hist || lsum || sharp)) continue;
        const uint8_t* s = src + img * ((int64_t)HW * 3);
        uint8_t* cp = copies + img * copy_stride;
        const bool vec = (reinterpret_cast<uintptr_t>(s) & 15u) == 0;
        const int g0 = slab * gps, g1 = mini(g0 + gps, G);
        if (!sharp) {
            for (int e = threadIdx.x; e < SLAB_WORDS; e += 256) h[e] = 0;
            __syncthreads();
        }
        uint32_t acc = 0;
        for (int g = g0 + threadIdx.x; g < g1; g += 256) {
            const int n = mini(16, HW - 16 * g);
            uint32_t w[12];
            load48(s + (int64_t)g * 48, n, vec, w);
            if (sharp) {
                store48(cp + (int64_t)g * 48, n, true, w);                           // the copies are 16-byte aligned
            } else if (hist) {
#pragma unroll
                for (int k = 0; k < 48; ++k)
                    if (k < 3 * n) atomicAdd(&h[(k % 3) * 256 + BYTE_OF(w, k)], 1u);
            } else {
#pragma unroll
                for (int k = 0; k < 16; ++k)
                    if (k < n) acc += (uint32_t)luma(BYTE_OF(w, 3 * k), BYTE_OF(w, 3 * k + 1), BYTE_OF(w, 3 * k + 2));
            }
        }
        if (sharp) continue;
        if (lsum) atomicAdd(&h[3 * 256], acc);
        __syncthreads();
        uint32_t* out = slabs + (img * S + slab) * SLAB_WORDS;
        if (hist)
            for (int e = threadIdx.x; e < 3 * 256; e += 256) out[e] = h[e];
        else if (threadIdx.x == 0)
            out[3 * 256] = h[3 * 256];
        __syncthreads();                                                         // the next unit of this block zeroes h
    }
}

__global__ __launch_bounds__(256) void photo_table_kernel(const int32_t* __restrict__ params, const uint32_t* __restrict__ slabs,
                                                          uint8_t* __restrict__ tables, int64_t nimg, int S, int HW) {
    __shared__ uint32_t h[256];
    __shared__ int lohi[2];
    const int i = threadIdx.x;
    for (int64_t img = blockIdx.x; img < nimg; img += gridDim.x) {
        const Row row = row_of(params, img);                                     // uniform over the block
        if (!table_kind(row.kind)) continue;
        uint8_t* t = tables + img * TABLE_BYTES;
        const uint32_t* sl = slabs + img * S * SLAB_WORDS;
        const float alpha = __int_as_float(row.value);
        if (row.kind == MUMPY_PHOTO_AUTOCONTRAST || row.kind == MUMPY_PHOTO_EQUALIZE) {
            for (int c = 0; c < 3; ++c) {
                uint32_t cnt = 0;
                for (int s = 0; s < S; ++s) cnt += sl[s * SLAB_WORDS + c * 256 + i];
                __syncthreads();                                                 // the previous channel's readers are done
                h[i] = cnt;
                if (i == 0) { lohi[0] = 255; lohi[1] = 0; }
                __syncthreads();
                if (cnt) { atomicMin(&lohi[0], i); atomicMax(&lohi[1], i); }
                __syncthreads();
                const int lo = lohi[0], hi = lohi[1];
                int e = i;                                                       // a flat channel: the identity
                if (hi > lo && row.kind == MUMPY_PHOTO_AUTOCONTRAST) {
                    const double scale = INV255.v[hi - lo];
                    const double offset = -(double)lo * scale;
                    const double prod = (double)i * scale;
                    const double v = prod + offset;
                    e = mini(maxi((int)v, 0), 255);
                } else if (hi > lo) {
                    const uint32_t step = ((uint32_t)HW - h[hi]) / 255u;
                    if (step) {
                        uint32_t n = step >> 1;
                        for (int j = 0; j < i; ++j) n += h[j];
                        const uint32_t q = n / step;
                        e = q > 255u ? 255 : (int)q;                             // Pillow's table saturates
                    }
                }
                t[c * 256 + i] = (uint8_t)e;
            }
            continue;
        }
        int e = i;
        if (row.kind == MUMPY_PHOTO_INVERT) {
            e = 255 - i;
        } else if (row.kind == MUMPY_PHOTO_SOLARIZE) {
            e = i < row.value ? i : 255 - i;
        } else if (row.kind == MUMPY_PHOTO_POSTERIZE) {
            const int bits = mini(maxi(row.value, 0), 8);
            e = i & ~((1 << (8 - bits)) - 1) & 255;
        } else if (row.kind == MUMPY_PHOTO_BRIGHTNESS) {
            e = blend(0, i, alpha);
        } else {                                                                 // contrast: the rounded mean of the luminance
            unsigned long long sum = 0;
            for (int s = 0; s < S; ++s) sum += sl[s * SLAB_WORDS + 3 * 256];
            const int m = (int)((2ull * sum + (unsigned long long)HW) / (2ull * (unsigned long long)HW));
            e = blend(m, i, alpha);
        }
        t[i] = t[256 + i] = t[512 + i] = (uint8_t)e;
    }
}

// one row term of the 3x3 filter on channel c of the pixels left, mid, right (offsets from a row's start, in bytes)
__device__ __forceinline__ float smooth_row(const uint8_t* __restrict__ r, float kmid) {
    const float a = (float)r[-3] * K1;
    const float b = (float)r[0] * kmid;
    const float c = (float)r[3] * K1;
    const float ab = a + b;
    return ab + c;
}

__global__ __launch_bounds__(256) void photo_apply_kernel(const uint8_t* src, uint8_t* dst, const int32_t* __restrict__ params,
                                                          const uint8_t* __restrict__ tables, const uint8_t* __restrict__ copies,
                                                          int64_t copy_stride, int64_t units, int chunks, int H, int W) {
    __shared__ __align__(16) uint8_t tab[TABLE_BYTES];
    const int HW = H * W, G = (HW + 15) >> 4;
    for (int64_t u = blockIdx.x; u < units; u += gridDim.x) {
        const int64_t img = u / chunks;
        const int chunk = (int)(u - img * chunks);
        const Row row = row_of(params, img);                                     // uniform over the block
        const uint8_t* s = src + img * ((int64_t)HW * 3);
        uint8_t* d = dst + img * ((int64_t)HW * 3);
        const bool svec = (reinterpret_cast<uintptr_t>(s) & 15u) == 0, dvec = (reinterpret_cast<uintptr_t>(d) & 15u) == 0;
        const float alpha = __int_as_float(row.value);
        if (row.kind == MUMPY_PHOTO_SHARPNESS) {
            const uint8_t* cp = copies + img * copy_stride;
            const int p1 = mini((chunk + 1) * CHUNK_PIXELS, HW);
            for (int p = chunk * CHUNK_PIXELS + threadIdx.x; p < p1; p += 256) {
                const int y = p / W, x = p - y * W;
                const uint8_t* c0 = cp + (int64_t)p * 3;
                int o[3] = {c0[0], c0[1], c0[2]};
                if (H >= 3 && W >= 3 && y > 0 && y < H - 1 && x > 0 && x < W - 1) {      // the border keeps the image
#pragma unroll
                    for (int c = 0; c < 3; ++c) {
                        float ss = 0.5f;
                        ss = ss + smooth_row(c0 + c + 3 * W, K1);
                        ss = ss + smooth_row(c0 + c, K5);
                        ss = ss + smooth_row(c0 + c - 3 * W, K1);
                        o[c] = blend(clip8(ss), o[c], alpha);
                    }
                }
                uint8_t* q = d + (int64_t)p * 3;
                q[0] = (uint8_t)o[0]; q[1] = (uint8_t)o[1]; q[2] = (uint8_t)o[2];
            }
            continue;
        }
        const bool tk = table_kind(row.kind), color = row.kind == MUMPY_PHOTO_COLOR;
        if (!tk && !color && src == dst) continue;                               // copy through, in place: nothing to move
        if (tk) {
            __syncthreads();                                                     // the previous unit's gathers are done
            if (threadIdx.x < TABLE_BYTES / 16)
                reinterpret_cast<uint4*>(tab)[threadIdx.x] = reinterpret_cast<const uint4*>(tables + img * TABLE_BYTES)[threadIdx.x];
            __syncthreads();
        }
        const int g1 = mini((chunk + 1) * CHUNK_GROUPS, G);
        for (int g = chunk * CHUNK_GROUPS + threadIdx.x; g < g1; g += 256) {
            const int n = mini(16, HW - 16 * g);
            uint32_t w[12];
            load48(s + (int64_t)g * 48, n, svec, w);
            if (tk) {
                uint32_t r[12];
#pragma unroll
                for (int j = 0; j < 12; ++j) r[j] = 0;
#pragma unroll
                for (int k = 0; k < 48; ++k) r[k >> 2] |= (uint32_t)tab[(k % 3) * 256 + BYTE_OF(w, k)] << (8 * (k & 3));
                store48(d + (int64_t)g * 48, n, dvec, r);
            } else if (color) {
                uint32_t r[12];
#pragma unroll
                for (int j = 0; j < 12; ++j) r[j] = 0;
#pragma unroll
                for (int k = 0; k < 16; ++k) {
                    const int cr = BYTE_OF(w, 3 * k), cg = BYTE_OF(w, 3 * k + 1), cb = BYTE_OF(w, 3 * k + 2);
                    const int L = luma(cr, cg, cb);
                    r[(3 * k) >> 2] |= (uint32_t)blend(L, cr, alpha) << (8 * ((3 * k) & 3));
                    r[(3 * k + 1) >> 2] |= (uint32_t)blend(L, cg, alpha) << (8 * ((3 * k + 1) & 3));
                    r[(3 * k + 2) >> 2] |= (uint32_t)blend(L, cb, alpha) << (8 * ((3 * k + 2) & 3));
                }
                store48(d + (int64_t)g * 48, n, dvec, r);
            } else {
                store48(d + (int64_t)g * 48, n, dvec, w);
            }
        }
    }
}

inline int64_t up16(int64_t v) { return (v + 15) & ~(int64_t)15; }
inline unsigned grid_for(int64_t units, int64_t cap) { return (unsigned)(units < cap ? units : cap); }

struct Plan { int G, S, gps, chunks; int64_t copy_stride, per_image; };
Plan plan_for(int H, int W) {
    Plan p;
    const int HW = H * W;
    p.G = (HW + 15) / 16;
    p.S = (p.G + SLAB_GROUPS - 1) / SLAB_GROUPS;
    if (p.S > SLAB_MAX) p.S = SLAB_MAX;
    p.gps = (p.G + p.S - 1) / p.S;
    p.chunks = (p.G + CHUNK_GROUPS - 1) / CHUNK_GROUPS;
    p.copy_stride = up16((int64_t)HW * 3);
    p.per_image = TABLE_BYTES + (int64_t)p.S * SLAB_BYTES + p.copy_stride;
    return p;
}

int check_sizes(const char* who, int64_t nimg, int H, int W) {
    MUMPY_REQUIRE(nimg >= 0 && H >= 1 && W >= 1, MUMPY_EINVAL, "%s: bad sizes nimg=%lld, %dx%d", who, (long long)nimg, H, W);
    MUMPY_REQUIRE(nimg < LIM31 && (int64_t)H * W <= HW_MAX, MUMPY_ERANGE,
                  "%s: nimg=%lld is 2^31 or more, or %d*%d is above 2^24 (an image's counts and sums are 32-bit)", who, (long long)nimg, H, W);
    return 0;
}

}  // namespace

extern "C" int64_t mumpy_photometric_workspace_bytes(int64_t nimg, int H, int W) {
    const int bad = check_sizes("photometric_workspace_bytes", nimg, H, W);
    return bad ? bad : nimg * plan_for(H, W).per_image;
}

extern "C" int mumpy_photometric_u8_fwd(const uint8_t* src, uint8_t* dst, const int32_t* params, void* workspace,
                                        int64_t workspace_bytes, int64_t nimg, int H, int W, void* stream) {
    MUMPY_REQUIRE(src && dst && params && workspace, MUMPY_ENULL, "photometric_u8: null pointer");
    const int bad = check_sizes("photometric_u8", nimg, H, W);
    if (bad) return bad;
    MUMPY_REQUIRE(aligned16(params) && aligned16(workspace), MUMPY_EALIGN, "photometric_u8: params and workspace must be 16-byte aligned");
    const Plan p = plan_for(H, W);
    MUMPY_REQUIRE(workspace_bytes >= nimg * p.per_image, MUMPY_EINVAL, "photometric_u8: workspace of %lld bytes, %lld needed",
                  (long long)workspace_bytes, (long long)(nimg * p.per_image));
    const int64_t bytes = nimg * H * W * 3;
    MUMPY_REQUIRE(src == dst || src + bytes <= dst || dst + bytes <= src, MUMPY_EINVAL,
                  "photometric_u8: dst overlaps src without being src");
    if (nimg == 0) return 0;
    uint8_t* tables = static_cast<uint8_t*>(workspace);                          // nimg tables, nimg * S slabs, nimg copies
    uint32_t* slabs = reinterpret_cast<uint32_t*>(tables + nimg * TABLE_BYTES);
    uint8_t* copies = tables + nimg * (TABLE_BYTES + (int64_t)p.S * SLAB_BYTES);
    hipLaunchKernelGGL(photo_stats_kernel, dim3(grid_for(nimg * p.S, 1 << 16)), dim3(256), 0, as_stream(stream), src, params, slabs,
                       copies, p.copy_stride, nimg * p.S, p.S, p.gps, H * W);
    MUMPY_CHECK_LAUNCH("photometric_u8 (statistics)");
    hipLaunchKernelGGL(photo_table_kernel, dim3(grid_for(nimg, 1 << 16)), dim3(256), 0, as_stream(stream), params, slabs, tables, nimg,
                       p.S, H * W);
    MUMPY_CHECK_LAUNCH("photometric_u8 (tables)");
    hipLaunchKernelGGL(photo_apply_kernel, dim3(grid_for(nimg * p.chunks, 1 << 16)), dim3(256), 0, as_stream(stream), src, dst, params,
                       tables, copies, p.copy_stride, nimg * p.chunks, p.chunks, H, W);
    MUMPY_CHECK_LAUNCH("photometric_u8 (apply)");
    return 0;
}
