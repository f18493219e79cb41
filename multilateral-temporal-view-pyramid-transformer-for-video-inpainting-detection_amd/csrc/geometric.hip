// geometric.hip — the geometric group of the reference's augmentation file (utils/randaugment.py:20-86 ShearX .. Rotate, :209-260
// Cutout) on uint8 frames and masks that stay on the device (include/mumpy_geometric.h), bit for bit what Pillow computes.
// mumpy_hip/geometric.py is the numpy statement and DESIGN.md ("Geometric operations") gives the arithmetic.
//
// One launch, a streaming gather, no floating point:
//   * a unit of work is (image, chunk of CHUNK_QUADS quads); a quad is 4 consecutive output pixels of one row (the last quad of a row
//     has W % 4 of them when that is not 0), one lane per quad, consecutive lanes on consecutive quads of the row;
//   * the image's row {mode, a0 .. a5, 0} is read once per unit as two 16-byte loads: uniform over the workgroup, so the mode
//     branches do not diverge;
//   * FIXED16 / SHIFT gather their pixels byte by byte (C bytes per pixel; neighbouring lanes read neighbouring bytes of the same or
//     the next source row for a shear or a translation) into C dwords held in registers; NONE / RECT / an unknown mode load those C
//     dwords from the same place in src and RECT clears the pixels inside the rectangle;
//   * the C dwords are stored whole when the quad is full and starts on a 4-byte boundary -- always, when W % 4 == 0 and dst is
//     4-byte aligned -- and as bytes otherwise (a row tail; the rows of an image whose W * C is no multiple of 4).
// Every byte of dst belongs to exactly one quad and is written exactly once; nothing else is written.
//
// OVERFLOW: the source coordinate (a2 + a0 x + a1 y) >> 16 is computed in 64-bit integers.  |a_i| < 2^31 and x, y < 2^13 bound every
// term by 2^44, so any row at all is safe, and the comparison against W and H happens before anything is narrowed: no row makes the
// kernel read outside src.  (Pillow walks in 32-bit ints; where check_fixed holds -- params_row refuses otherwise -- its sums stay
// below 2^31 and the two walks agree.)  Byte offsets inside one image stay below 3 * 2^24 < 2^31; the image's own offset is 64-bit.
#include "common.h"
#include "../../include/mumpy_geometric.h"
using namespace mumpy;

namespace {

constexpr int64_t LIM31 = (int64_t)1 << 31;
constexpr int SIDE_MAX = 8192;
constexpr int HW_MAX = 1 << 24;
constexpr int CHUNK_QUADS = 1024;                        // quads per unit: four per lane of a 256-lane workgroup

template <int C> struct __attribute__((packed, aligned(4))) Words { uint32_t v[C]; };

template <int C>
__global__ __launch_bounds__(256) void geometric_kernel(const uint8_t* __restrict__ src, uint8_t* __restrict__ dst,
                                                        const int32_t* __restrict__ params, int64_t units, int chunks, int H, int W) {
    const int QW = (W + 3) >> 2, NQ = H * QW;
    const int64_t image_bytes = (int64_t)H * W * C;
    for (int64_t u = blockIdx.x; u < units; u += gridDim.x) {
        const int64_t img = u / chunks;
        const int chunk = (int)(u - img * chunks);
        const int4 pa = reinterpret_cast<const int4*>(params + img * 8)[0];      // uniform over the workgroup
        const int4 pb = reinterpret_cast<const int4*>(params + img * 8)[1];
        const int mode = pa.x;
        const bool walk = mode == MUMPY_GEO_FIXED16 || mode == MUMPY_GEO_SHIFT;
        // SHIFT is the walk (x + a0, y + a1) in whole pixels: the same integers with a 16.16 one as the step
        const int64_t ax = mode == MUMPY_GEO_SHIFT ? 65536 : pa.y, bx = mode == MUMPY_GEO_SHIFT ? 0 : pa.z;
        const int64_t cx = mode == MUMPY_GEO_SHIFT ? (int64_t)pa.y * 65536 : pa.w;
        const int64_t ay = mode == MUMPY_GEO_SHIFT ? 0 : pb.x, by = mode == MUMPY_GEO_SHIFT ? 65536 : pb.y;
        const int64_t cy = mode == MUMPY_GEO_SHIFT ? (int64_t)pa.z * 65536 : pb.z;
        const uint8_t* s = src + img * image_bytes;
        uint8_t* d = dst + img * image_bytes;
        const int q1 = min((chunk + 1) * CHUNK_QUADS, NQ);
        for (int q = chunk * CHUNK_QUADS + (int)threadIdx.x; q < q1; q += 256) {
            const int y = q / QW, x = (q - y * QW) * 4;
            const int n = min(4, W - x);
            const int o = (y * W + x) * C;
            uint32_t w[C];
#pragma unroll
            for (int j = 0; j < C; ++j) w[j] = 0;
            if (walk) {
                int64_t fx = cx + ax * x + bx * y, fy = cy + ay * x + by * y;
#pragma unroll
                for (int k = 0; k < 4; ++k, fx += ax, fy += ay) {
                    const int64_t sx = fx >> 16, sy = fy >> 16;
                    if (k < n && sx >= 0 && sx < W && sy >= 0 && sy < H) {
                        const uint8_t* p = s + ((int)sy * W + (int)sx) * C;
#pragma unroll
                        for (int c = 0; c < C; ++c) w[(k * C + c) >> 2] |= (uint32_t)p[c] << (8 * ((k * C + c) & 3));
                    }
                }
            } else {
                if (n == 4 && (reinterpret_cast<uintptr_t>(s + o) & 3u) == 0) {
                    const Words<C> r = *reinterpret_cast<const Words<C>*>(s + o);
#pragma unroll
                    for (int j = 0; j < C; ++j) w[j] = r.v[j];
                } else {
#pragma unroll
                    for (int b = 0; b < 4 * C; ++b)
                        if (b < n * C) w[b >> 2] |= (uint32_t)s[o + b] << (8 * (b & 3));
                }
                if (mode == MUMPY_GEO_RECT && y >= pa.z && y <= pb.x) {
#pragma unroll
                    for (int k = 0; k < 4; ++k)
                        if (x + k >= pa.y && x + k <= pa.w) {
#pragma unroll
                            for (int c = 0; c < C; ++c) w[(k * C + c) >> 2] &= ~(0xFFu << (8 * ((k * C + c) & 3)));
                        }
                }
            }
            if (n == 4 && (reinterpret_cast<uintptr_t>(d + o) & 3u) == 0) {
                Words<C> r;
#pragma unroll
                for (int j = 0; j < C; ++j) r.v[j] = w[j];
                *reinterpret_cast<Words<C>*>(d + o) = r;
            } else {
#pragma unroll
                for (int b = 0; b < 4 * C; ++b)
                    if (b < n * C) d[o + b] = (uint8_t)(w[b >> 2] >> (8 * (b & 3)));
            }
        }
    }
}

}  // namespace

extern "C" int mumpy_geometric_u8_fwd(const uint8_t* src, uint8_t* dst, const int32_t* params, int64_t nimg, int H, int W, int C,
                                      void* stream) {
    MUMPY_REQUIRE(src && dst && params, MUMPY_ENULL, "geometric_u8: null pointer");
    MUMPY_REQUIRE(nimg >= 0 && H >= 1 && W >= 1, MUMPY_EINVAL, "geometric_u8: bad sizes nimg=%lld, %dx%d", (long long)nimg, H, W);
    MUMPY_REQUIRE(C == 1 || C == 3, MUMPY_EINVAL, "geometric_u8: C=%d must be 1 or 3", C);
    MUMPY_REQUIRE(nimg < LIM31 && H <= SIDE_MAX && W <= SIDE_MAX && (int64_t)H * W <= HW_MAX, MUMPY_ERANGE,
                  "geometric_u8: nimg=%lld is 2^31 or more, or %dx%d is above 8192 a side or 2^24 pixels", (long long)nimg, H, W);
    MUMPY_REQUIRE(aligned16(params), MUMPY_EALIGN, "geometric_u8: params must be 16-byte aligned");
    const int64_t bytes = nimg * H * W * C;
    MUMPY_REQUIRE(bytes == 0 || (src != dst && (src + bytes <= dst || dst + bytes <= src)), MUMPY_EINVAL,
                  "geometric_u8: dst overlaps src (a gather cannot run in place)");
    if (nimg == 0) return 0;
    const int quads = H * ((W + 3) / 4);
    const int chunks = (quads + CHUNK_QUADS - 1) / CHUNK_QUADS;
    const int64_t units = nimg * chunks;
    const unsigned grid = (unsigned)(units < (1 << 16) ? units : (1 << 16));
    if (C == 3)
        hipLaunchKernelGGL(geometric_kernel<3>, dim3(grid), dim3(256), 0, as_stream(stream), src, dst, params, units, chunks, H, W);
    else
        hipLaunchKernelGGL(geometric_kernel<1>, dim3(grid), dim3(256), 0, as_stream(stream), src, dst, params, units, chunks, H, W);
    MUMPY_CHECK_LAUNCH("geometric_u8");
    return 0;
}
