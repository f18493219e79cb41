// perturb.hip — ordinary post-processing of uint8 frames on the device (include/mumpy_perturb.h): the JPEG round trip and the Gaussian
// blur that the reference's augmentation code ships (utils/randaugment.py:492-512), bit for bit what Pillow computes, and the NEAREST
// gather that puts source frames on the canvas they are applied to.  mumpy_hip/perturb.py is the numpy statement of both and DESIGN.md
// ("Perturbations") gives the arithmetic; everything here is int32 / uint32.
//
// JPEG, launch 1 (jpeg_code_kernel): one wave per 16x16 MCU, four MCUs per block.  Lane (qy, qx) converts the 2x2 pixel quad it loads
// to four Y samples and one Cb / Cr sample (the 2x2 mean with libjpeg's alternating bias); the six 8x8 blocks sit in LDS as int32 with
// a row stride of 9 dwords (lanes walking rows or columns hit different banks).  Then 48 lanes work, one per block row (forward DCT
// pass 1), one per block column (forward pass 2, quantise, dequantise, inverse pass 1: the inverse goes columns first, so the column
// never leaves its lane's registers), one per block row again (inverse pass 2, + 128, clamp).  The butterflies are on eight named
// registers -- no indexed array, no scratch.  The decoded planes go to the workspace: the chroma of the neighbouring MCUs is what
// launch 2 (jpeg_merge_kernel, one thread per pixel: triangle upsampling + YCbCr -> RGB) needs, hence two launches.
//
// Blur: box_row_kernel holds one image row in LDS (two buffers of 3 W bytes) and runs the three row passes there; box_col_kernel
// holds a tile of TC columns over all H rows and runs the three column passes.  A pass sums only the samples inside the line and adds
// the clamped ones in closed form, so a window wider than the image costs no more than the image.
#include "common.h"
#include "../../include/mumpy_perturb.h"
using namespace mumpy;

namespace {

constexpr int64_t LIM31 = (int64_t)1 << 31;
constexpr int LDS_BUDGET = 64 * 1024;                    // dynamic LDS a launch may ask for without raising the limit
constexpr int BOX_LINE_MAX = LDS_BUDGET / 6;                 // two buffers of 3 bytes per sample: 10922

__device__ __forceinline__ int mini(int a, int b) { return a < b ? a : b; }
__device__ __forceinline__ int maxi(int a, int b) { return a > b ? a : b; }
__device__ __forceinline__ int clamp255(int v) { return v < 0 ? 0 : (v > 255 ? 255 : v); }
__device__ __forceinline__ int descale(int x, int n) { return (x + (1 << (n - 1))) >> n; }

// FIX(x) = round(x * 2^13) of the Loeffler-Ligtenberg-Moschytz factorisation (libjpeg's jfdctint.c / jidctint.c)
constexpr int F_0_298 = 2446, F_0_390 = 3196, F_0_541 = 4433, F_0_765 = 6270, F_0_899 = 7373, F_1_175 = 9633;
constexpr int F_1_501 = 12299, F_1_847 = 15137, F_1_961 = 16069, F_2_053 = 16819, F_2_562 = 20995, F_3_072 = 25172;
constexpr int CONST_BITS = 13, PASS1_BITS = 2;

// One pass of the slow-integer forward DCT over eight samples.  FIRST: the row pass (outputs scaled up by 2^PASS1_BITS).
template <bool FIRST>
__device__ __forceinline__ void fdct8(int& d0, int& d1, int& d2, int& d3, int& d4, int& d5, int& d6, int& d7) {
    constexpr int N = FIRST ? CONST_BITS - PASS1_BITS : CONST_BITS + PASS1_BITS;
    const int t0 = d0 + d7, t7 = d0 - d7, t1 = d1 + d6, t6 = d1 - d6, t2 = d2 + d5, t5 = d2 - d5, t3 = d3 + d4, t4 = d3 - d4;
    const int t10 = t0 + t3, t13 = t0 - t3, t11 = t1 + t2, t12 = t1 - t2;
    d0 = FIRST ? (t10 + t11) << PASS1_BITS : descale(t10 + t11, PASS1_BITS);
    d4 = FIRST ? (t10 - t11) << PASS1_BITS : descale(t10 - t11, PASS1_BITS);
    const int e1 = (t12 + t13) * F_0_541;
    d2 = descale(e1 + t13 * F_0_765, N);
    d6 = descale(e1 - t12 * F_1_847, N);
    const int z5 = (t4 + t6 + t5 + t7) * F_1_175;
    const int z1 = -(t4 + t7) * F_0_899, z2 = -(t5 + t6) * F_2_562;
    const int z3 = -(t4 + t6) * F_1_961 + z5, z4 = -(t5 + t7) * F_0_390 + z5;
    d7 = descale(t4 * F_0_298 + z1 + z3, N);
    d5 = descale(t5 * F_2_053 + z2 + z4, N);
    d3 = descale(t6 * F_3_072 + z2 + z3, N);
    d1 = descale(t7 * F_1_501 + z1 + z4, N);
}

// One pass of the slow-integer inverse DCT, descaled by N bits.
template <int N>
__device__ __forceinline__ void idct8(int& c0, int& c1, int& c2, int& c3, int& c4, int& c5, int& c6, int& c7) {
    const int e1 = (c2 + c6) * F_0_541;
    const int e2 = e1 - c6 * F_1_847, e3 = e1 + c2 * F_0_765;
    const int e0 = (c0 + c4) << CONST_BITS, e4 = (c0 - c4) << CONST_BITS;
    const int t10 = e0 + e3, t13 = e0 - e3, t11 = e4 + e2, t12 = e4 - e2;
    const int z5 = (c7 + c3 + c5 + c1) * F_1_175;
    const int z1 = -(c7 + c1) * F_0_899, z2 = -(c5 + c3) * F_2_562;
    const int z3 = -(c7 + c3) * F_1_961 + z5, z4 = -(c5 + c1) * F_0_390 + z5;
    const int o0 = c7 * F_0_298 + z1 + z3, o1 = c5 * F_2_053 + z2 + z4, o2 = c3 * F_3_072 + z2 + z3, o3 = c1 * F_1_501 + z1 + z4;
    c0 = descale(t10 + o3, N); c7 = descale(t10 - o3, N);
    c1 = descale(t11 + o2, N); c6 = descale(t11 - o2, N);
    c2 = descale(t12 + o1, N); c5 = descale(t12 - o1, N);
    c3 = descale(t13 + o0, N); c4 = descale(t13 - o0, N);
}

// level = sign(c) * ((|c| + q8/2) / q8), q8 = 8 q (the forward DCT leaves a factor 8), then level * q
__device__ __forceinline__ int requantise(int c, int q) {
    q = q < 1 ? 1 : q;
    const unsigned q8 = 8u * (unsigned)q, a = (unsigned)(c < 0 ? -c : c) + (q8 >> 1);
    const int lvl = a >= q8 ? (int)(a / q8) : 0;
    return (c < 0 ? -lvl : lvl) * q;
}

struct Ycc { int y, cb, cr; };
__device__ __forceinline__ Ycc to_ycc(const uint8_t* __restrict__ p) {
    const int r = p[0], g = p[1], b = p[2];
    return {(19595 * r + 38470 * g + 7471 * b + 32768) >> 16, (-11059 * r - 21709 * g + 32768 * b + (128 << 16) + 32767) >> 16,
            (32768 * r - 27439 * g - 5329 * b + (128 << 16) + 32767) >> 16};
}

constexpr int BROW = 9, BLK = 8 * BROW;                  // row stride and size of one 8x8 block in LDS, in dwords
constexpr int MCU_PER_WG = 4;

// does image `img` take part?  (sel is device memory: a value outside [0, ntab) means "copy through")
__device__ __forceinline__ bool table_of(const int32_t* __restrict__ sel, int64_t img, int ntab, int& t) {
    t = sel[img];
    return t >= 0 && t < ntab;
}

__global__ __launch_bounds__(256) void jpeg_code_kernel(const uint8_t* __restrict__ src, const uint16_t* __restrict__ qtab,
                                                        const int32_t* __restrict__ sel, uint8_t* __restrict__ ws, int64_t ws_stride,
                                                        int64_t units, int ntab, int H, int W, int mcus_x, int mcus) {
    __shared__ int lds[MCU_PER_WG][6 * BLK];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    int* const b = lds[wave];
    const int ch = (H + 1) >> 1, cw = (W + 1) >> 1;
    const int qy = lane >> 3, qx = lane & 7;
    const int blk = lane >> 3, k = lane & 7;             // lanes 0 .. 47: block `blk`, its row or column `k`
    for (int64_t u0 = (int64_t)blockIdx.x * MCU_PER_WG; u0 < units; u0 += (int64_t)gridDim.x * MCU_PER_WG) {      // uniform over the block
        const int64_t u = u0 + wave;
        int64_t img = 0;
        int t = 0, mcu = 0;
        bool live = u < units;
        if (live) {
            img = u / mcus;
            mcu = (int)(u - img * mcus);
            live = table_of(sel, img, ntab, t);
        }
        const int Y0 = (mcu / mcus_x) * 16, X0 = (mcu % mcus_x) * 16;
        if (live) {
            const uint8_t* s = src + img * ((int64_t)H * W * 3);
            const int x0 = mini(X0 + 2 * qx, W - 1) * 3, x1 = mini(X0 + 2 * qx + 1, W - 1) * 3;
            int r0 = mini(Y0 + 2 * qy, H - 1) * W * 3, r1 = mini(Y0 + 2 * qy + 1, H - 1) * W * 3;
            Ycc p00 = to_ycc(s + r0 + x0), p01 = to_ycc(s + r0 + x1), p10 = to_ycc(s + r1 + x0), p11 = to_ycc(s + r1 + x1);
            int* yb = b + ((qy >> 2) * 2 + (qx >> 2)) * BLK + ((2 * qy) & 7) * BROW + ((2 * qx) & 7);
            yb[0] = p00.y - 128; yb[1] = p01.y - 128; yb[BROW] = p10.y - 128; yb[BROW + 1] = p11.y - 128;
            const int ci = (Y0 >> 1) + qy;
            if (ci >= ch) {                              // a chroma row below the plane repeats the plane's last row, not the input's
                r0 = 2 * (ch - 1) * W * 3; r1 = mini(2 * ch - 1, H - 1) * W * 3;
                p00 = to_ycc(s + r0 + x0); p01 = to_ycc(s + r0 + x1); p10 = to_ycc(s + r1 + x0); p11 = to_ycc(s + r1 + x1);
            }
            const int bias = 1 + (qx & 1);               // output column X0 / 2 + qx: X0 / 2 is even
            b[4 * BLK + qy * BROW + qx] = ((p00.cb + p01.cb + p10.cb + p11.cb + bias) >> 2) - 128;
            b[5 * BLK + qy * BROW + qx] = ((p00.cr + p01.cr + p10.cr + p11.cr + bias) >> 2) - 128;
        }
        __syncthreads();
        if (live && lane < 48) {                         // forward, rows
            int* p = b + blk * BLK + k * BROW;
            int d0 = p[0], d1 = p[1], d2 = p[2], d3 = p[3], d4 = p[4], d5 = p[5], d6 = p[6], d7 = p[7];
            fdct8<true>(d0, d1, d2, d3, d4, d5, d6, d7);
            p[0] = d0; p[1] = d1; p[2] = d2; p[3] = d3; p[4] = d4; p[5] = d5; p[6] = d6; p[7] = d7;
        }
        __syncthreads();
        if (live && lane < 48) {                         // forward, columns; quantise and dequantise; inverse, columns
            int* p = b + blk * BLK + k;
            const uint16_t* q = qtab + ((int64_t)t * 2 + (blk >= 4 ? 1 : 0)) * 64 + k;
            int d0 = p[0], d1 = p[BROW], d2 = p[2 * BROW], d3 = p[3 * BROW], d4 = p[4 * BROW], d5 = p[5 * BROW], d6 = p[6 * BROW],
                d7 = p[7 * BROW];
            fdct8<false>(d0, d1, d2, d3, d4, d5, d6, d7);
            d0 = requantise(d0, q[0]); d1 = requantise(d1, q[8]); d2 = requantise(d2, q[16]); d3 = requantise(d3, q[24]);
            d4 = requantise(d4, q[32]); d5 = requantise(d5, q[40]); d6 = requantise(d6, q[48]); d7 = requantise(d7, q[56]);
            idct8<CONST_BITS - PASS1_BITS>(d0, d1, d2, d3, d4, d5, d6, d7);
            p[0] = d0; p[BROW] = d1; p[2 * BROW] = d2; p[3 * BROW] = d3; p[4 * BROW] = d4; p[5 * BROW] = d5; p[6 * BROW] = d6;
            p[7 * BROW] = d7;
        }
        __syncthreads();
        if (live && lane < 48) {                         // inverse, rows; + 128; the saturating clamp
            int* p = b + blk * BLK + k * BROW;
            int d0 = p[0], d1 = p[1], d2 = p[2], d3 = p[3], d4 = p[4], d5 = p[5], d6 = p[6], d7 = p[7];
            idct8<CONST_BITS + PASS1_BITS + 3>(d0, d1, d2, d3, d4, d5, d6, d7);
            p[0] = clamp255(d0 + 128); p[1] = clamp255(d1 + 128); p[2] = clamp255(d2 + 128); p[3] = clamp255(d3 + 128);
            p[4] = clamp255(d4 + 128); p[5] = clamp255(d5 + 128); p[6] = clamp255(d6 + 128); p[7] = clamp255(d7 + 128);
        }
        __syncthreads();
        if (live) {                                      // the quad's four Y samples and its chroma sample, where the planes hold them
            uint8_t* wy = ws + img * ws_stride;
            uint8_t* wcb = wy + (int64_t)H * W;
            uint8_t* wcr = wcb + ch * cw;
            const int* yb = b + ((qy >> 2) * 2 + (qx >> 2)) * BLK + ((2 * qy) & 7) * BROW + ((2 * qx) & 7);
            const int y = Y0 + 2 * qy, x = X0 + 2 * qx;
            if (y < H && x < W) wy[y * W + x] = (uint8_t)yb[0];
            if (y < H && x + 1 < W) wy[y * W + x + 1] = (uint8_t)yb[1];
            if (y + 1 < H && x < W) wy[(y + 1) * W + x] = (uint8_t)yb[BROW];
            if (y + 1 < H && x + 1 < W) wy[(y + 1) * W + x + 1] = (uint8_t)yb[BROW + 1];
            const int ci = (Y0 >> 1) + qy, cj = (X0 >> 1) + qx;
            if (ci < ch && cj < cw) {
                wcb[ci * cw + cj] = (uint8_t)b[4 * BLK + qy * BROW + qx];
                wcr[ci * cw + cj] = (uint8_t)b[5 * BLK + qy * BROW + qx];
            }
        }
        __syncthreads();                                 // the next unit of this wave reuses the blocks
    }
}

__global__ __launch_bounds__(256) void jpeg_merge_kernel(const uint8_t* src, uint8_t* dst, const int32_t* __restrict__ sel,
                                                         const uint8_t* __restrict__ ws, int64_t ws_stride, int64_t total, int ntab,
                                                         int H, int W) {
    const int ch = (H + 1) >> 1, cw = (W + 1) >> 1, hw = H * W;
    for (int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x; idx < total; idx += (int64_t)gridDim.x * 256) {
        const int64_t img = idx / hw;
        const int p = (int)(idx - img * hw);
        const int64_t o = (img * hw + p) * 3;
        int t;
        if (!table_of(sel, img, ntab, t)) {              // copy through (dst may be src: each thread moves its own pixel)
            const uint8_t r = src[o], g = src[o + 1], bl = src[o + 2];
            dst[o] = r; dst[o + 1] = g; dst[o + 2] = bl;
            continue;
        }
        const int y = p / W, x = p - y * W;
        const uint8_t* wy = ws + img * ws_stride;
        const uint8_t* wc = wy + hw;
        const int i = y >> 1, j = x >> 1;
        const int i2 = (y & 1) ? mini(i + 1, ch - 1) : maxi(i - 1, 0);
        const int j2 = (x & 1) ? mini(j + 1, cw - 1) : maxi(j - 1, 0);
        const int rnd = (x & 1) ? 7 : 8;
        int c[2];
#pragma unroll
        for (int pl = 0; pl < 2; ++pl) {
            const uint8_t* cp = wc + pl * (ch * cw);
            const int v = 3 * cp[i * cw + j] + cp[i2 * cw + j], vn = 3 * cp[i * cw + j2] + cp[i2 * cw + j2];
            c[pl] = ((3 * v + vn + rnd) >> 4) - 128;
        }
        const int yy = wy[p];
        dst[o] = (uint8_t)clamp255(yy + ((91881 * c[1] + 32768) >> 16));
        dst[o + 1] = (uint8_t)clamp255(yy + ((-22554 * c[0] - 46802 * c[1] + 32768) >> 16));
        dst[o + 2] = (uint8_t)clamp255(yy + ((116130 * c[0] + 32768) >> 16));
    }
}

// One extended-box pass over `lines` interleaved lines of n samples: sample i of line k is at in[i * stride + k].
__device__ __forceinline__ void box_pass(const uint8_t* in, uint8_t* out, int n, int lines, int stride, int r, unsigned ww, unsigned fw) {
    for (int e = threadIdx.x; e < n * lines; e += 256) {
        const int i = e / lines, k = e - i * lines;
        const uint8_t* p = in + k;
        const int lo = i - r, hi = i + r;
        const int jl = maxi(lo, 0), jh = mini(hi, n - 1);
        unsigned acc = 0;
        for (int j = jl; j <= jh; ++j) acc += p[j * stride];
        acc += (unsigned)(jl - lo) * p[0] + (unsigned)(hi - jh) * p[(n - 1) * stride];               // the clamped samples
        const unsigned outer = (unsigned)p[maxi(lo - 1, 0) * stride] + p[mini(hi + 1, n - 1) * stride];
        out[i * stride + k] = (uint8_t)((ww * acc + fw * outer + (1u << 23)) >> 24);
    }
}

struct BoxParams { int r; unsigned ww, fw; bool on; };
__device__ __forceinline__ BoxParams box_params_of(const int32_t* __restrict__ params, int64_t img) {
    const int4 p = *reinterpret_cast<const int4*>(params + img * 4);
    return {mini(maxi(p.x, 0), 1 << 24), (unsigned)p.y, (unsigned)p.z, p.w != 0};       // r bounded: i + r + 1 stays an int
}

// rows: one image row per block iteration, two buffers of 3 W bytes
__global__ __launch_bounds__(256) void box_row_kernel(const uint8_t* __restrict__ src, uint8_t* __restrict__ ws,
                                                      const int32_t* __restrict__ params, int64_t rows, int H, int W, int buf) {
    extern __shared__ __align__(16) uint8_t box_lds[];
    uint8_t* A = box_lds;
    uint8_t* B = box_lds + buf;
    const int n3 = 3 * W;
    for (int64_t row = blockIdx.x; row < rows; row += gridDim.x) {
        const BoxParams bp = box_params_of(params, row / H);                     // uniform over the block
        if (!bp.on) continue;
        const uint8_t* s = src + row * n3;
        for (int e = threadIdx.x; e < n3; e += 256) A[e] = s[e];
        __syncthreads();
        box_pass(A, B, W, 3, 3, bp.r, bp.ww, bp.fw);
        __syncthreads();
        box_pass(B, A, W, 3, 3, bp.r, bp.ww, bp.fw);
        __syncthreads();
        box_pass(A, B, W, 3, 3, bp.r, bp.ww, bp.fw);
        __syncthreads();
        uint8_t* d = ws + row * n3;
        for (int e = threadIdx.x; e < n3; e += 256) d[e] = B[e];
        __syncthreads();                                                         // the next row of this block reuses the buffers
    }
}

// columns: a tile of tc columns over all H rows per block iteration, two buffers of H * 3 tc bytes
__global__ __launch_bounds__(256) void box_col_kernel(const uint8_t* src, uint8_t* dst, const uint8_t* __restrict__ ws,
                                                      const int32_t* __restrict__ params, int64_t units, int H, int W, int tc, int tiles,
                                                      int buf) {
    extern __shared__ __align__(16) uint8_t box_lds[];
    uint8_t* A = box_lds;
    uint8_t* B = box_lds + buf;
    const int stride = 3 * tc;
    for (int64_t u = blockIdx.x; u < units; u += gridDim.x) {
        const int64_t img = u / tiles;
        const int x0 = (int)(u - img * tiles) * tc;
        const int lines = 3 * mini(tc, W - x0);
        const int64_t base = (img * H * W + x0) * 3;
        const BoxParams bp = box_params_of(params, img);                         // uniform over the block
        if (!bp.on) {                                    // copy through (dst may be src: each thread moves its own bytes)
            for (int e = threadIdx.x; e < H * lines; e += 256) {
                const int y = e / lines, k = e - y * lines;
                dst[base + (int64_t)y * W * 3 + k] = src[base + (int64_t)y * W * 3 + k];
            }
            continue;
        }
        for (int e = threadIdx.x; e < H * lines; e += 256) {
            const int y = e / lines, k = e - y * lines;
            A[y * stride + k] = ws[base + (int64_t)y * W * 3 + k];
        }
        __syncthreads();
        box_pass(A, B, H, lines, stride, bp.r, bp.ww, bp.fw);
        __syncthreads();
        box_pass(B, A, H, lines, stride, bp.r, bp.ww, bp.fw);
        __syncthreads();
        box_pass(A, B, H, lines, stride, bp.r, bp.ww, bp.fw);
        __syncthreads();
        for (int e = threadIdx.x; e < H * lines; e += 256) {
            const int y = e / lines, k = e - y * lines;
            dst[base + (int64_t)y * W * 3 + k] = B[y * stride + k];
        }
        __syncthreads();
    }
}

__global__ __launch_bounds__(256) void resize_nearest_u8_kernel(const uint8_t* __restrict__ src, uint8_t* __restrict__ dst,
                                                                const int32_t* __restrict__ ytab, const int32_t* __restrict__ xtab,
                                                                int64_t total, int Hs, int Ws, int H, int W, int C) {
    const int hw = H * W;
    for (int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x; idx < total; idx += (int64_t)gridDim.x * 256) {
        const int64_t img = idx / hw;
        const int p = (int)(idx - img * hw);
        const int y = p / W, x = p - y * W;
        const int sy = mini(maxi(ytab[y], 0), Hs - 1), sx = mini(maxi(xtab[x], 0), Ws - 1);
        const uint8_t* s = src + (img * Hs * Ws + (int64_t)sy * Ws + sx) * C;
        uint8_t* d = dst + idx * C;
        if (C == 3) { d[0] = s[0]; d[1] = s[1]; d[2] = s[2]; }
        else for (int c = 0; c < C; ++c) d[c] = s[c];
    }
}

inline int64_t up16(int64_t v) { return (v + 15) & ~(int64_t)15; }
inline int64_t jpeg_image_stride(int H, int W) { return up16((int64_t)H * W + 2 * (int64_t)((H + 1) / 2) * ((W + 1) / 2)); }
inline unsigned grid_for(int64_t units, int64_t cap) { return (unsigned)(units < cap ? units : cap); }

// the size checks the workspace queries and the entries share: 0 or the refusal
int check_sizes(const char* who, int64_t nimg, int H, int W) {
    MUMPY_REQUIRE(nimg >= 0 && H >= 1 && W >= 1, MUMPY_EINVAL, "%s: bad sizes nimg=%lld, %dx%d", who, (long long)nimg, H, W);
    MUMPY_REQUIRE(nimg < LIM31 && 3 * (int64_t)H * W < LIM31, MUMPY_ERANGE,
                  "%s: nimg=%lld or 3*%d*%d is 2^31 or more (offsets inside an image are 32-bit)", who, (long long)nimg, H, W);
    return 0;
}

int blur_check_sizes(const char* who, int64_t nimg, int H, int W) {
    const int bad = check_sizes(who, nimg, H, W);
    if (bad) return bad;
    MUMPY_REQUIRE(H <= BOX_LINE_MAX && W <= BOX_LINE_MAX, MUMPY_ERANGE, "%s: %dx%d: a side above %d does not fit the LDS line buffers", who, H, W,
                  BOX_LINE_MAX);
    return 0;
}

}  // namespace

extern "C" int64_t mumpy_jpeg_roundtrip_workspace_bytes(int64_t nimg, int H, int W) {
    const int bad = check_sizes("jpeg_roundtrip_workspace_bytes", nimg, H, W);
    return bad ? bad : nimg * jpeg_image_stride(H, W);
}

extern "C" int mumpy_jpeg_roundtrip_u8_fwd(const uint8_t* src, uint8_t* dst, const uint16_t* qtab, const int32_t* sel, void* workspace,
                                           int64_t workspace_bytes, int64_t nimg, int ntab, int H, int W, void* stream) {
    MUMPY_REQUIRE(src && dst && qtab && sel && workspace, MUMPY_ENULL, "jpeg_roundtrip_u8: null pointer");
    const int bad = check_sizes("jpeg_roundtrip_u8", nimg, H, W);
    if (bad) return bad;
    MUMPY_REQUIRE(ntab >= 1, MUMPY_EINVAL, "jpeg_roundtrip_u8: ntab=%d must be at least 1", ntab);
    MUMPY_REQUIRE(aligned16(qtab) && aligned16(workspace) && (reinterpret_cast<uintptr_t>(sel) & 3u) == 0, MUMPY_EALIGN,
                  "jpeg_roundtrip_u8: qtab and workspace must be 16-byte aligned, sel 4-byte aligned");
    const int64_t stride = jpeg_image_stride(H, W);
    MUMPY_REQUIRE(workspace_bytes >= nimg * stride, MUMPY_EINVAL, "jpeg_roundtrip_u8: workspace of %lld bytes, %lld needed",
                  (long long)workspace_bytes, (long long)(nimg * stride));
    if (nimg == 0) return 0;
    const int mcus_y = (H + 15) / 16, mcus_x = (W + 15) / 16, mcus = mcus_y * mcus_x;          // < 2^31 / 768
    const int64_t units = nimg * mcus, groups = (units + MCU_PER_WG - 1) / MCU_PER_WG;
    hipLaunchKernelGGL(jpeg_code_kernel, dim3(grid_for(groups, 1 << 16)), dim3(256), 0, as_stream(stream), src, qtab, sel,
                       static_cast<uint8_t*>(workspace), stride, units, ntab, H, W, mcus_x, mcus);
    MUMPY_CHECK_LAUNCH("jpeg_roundtrip_u8 (blocks)");
    const int64_t total = nimg * H * W;
    hipLaunchKernelGGL(jpeg_merge_kernel, dim3(grid_for((total + 255) / 256, 1 << 16)), dim3(256), 0, as_stream(stream), src, dst, sel,
                       static_cast<const uint8_t*>(workspace), stride, total, ntab, H, W);
    MUMPY_CHECK_LAUNCH("jpeg_roundtrip_u8 (merge)");
    return 0;
}

extern "C" int64_t mumpy_gaussian_blur_workspace_bytes(int64_t nimg, int H, int W) {
    const int bad = blur_check_sizes("gaussian_blur_workspace_bytes", nimg, H, W);
    return bad ? bad : up16(nimg * H * W * 3);
}

extern "C" int mumpy_gaussian_blur_u8_fwd(const uint8_t* src, uint8_t* dst, const int32_t* params, void* workspace,
                                          int64_t workspace_bytes, int64_t nimg, int H, int W, void* stream) {
    MUMPY_REQUIRE(src && dst && params && workspace, MUMPY_ENULL, "gaussian_blur_u8: null pointer");
    const int bad = blur_check_sizes("gaussian_blur_u8", nimg, H, W);
    if (bad) return bad;
    MUMPY_REQUIRE(aligned16(params) && aligned16(workspace), MUMPY_EALIGN, "gaussian_blur_u8: params and workspace must be 16-byte aligned");
    MUMPY_REQUIRE(workspace_bytes >= up16(nimg * H * W * 3), MUMPY_EINVAL, "gaussian_blur_u8: workspace of %lld bytes, %lld needed",
                  (long long)workspace_bytes, (long long)up16(nimg * H * W * 3));
    if (nimg == 0) return 0;
    const int row_buf = (int)up16(3 * (int64_t)W);
    hipLaunchKernelGGL(box_row_kernel, dim3(grid_for(nimg * H, 1 << 16)), dim3(256), 2 * row_buf, as_stream(stream), src,
                       static_cast<uint8_t*>(workspace), params, nimg * H, H, W, row_buf);
    MUMPY_CHECK_LAUNCH("gaussian_blur_u8 (rows)");
    int tc = 16;                                         // the widest column tile whose two buffers of H rows fit
    while (tc > 1 && 2 * up16(3 * (int64_t)tc * H) > LDS_BUDGET) tc >>= 1;
    const int col_buf = (int)up16(3 * (int64_t)tc * H), tiles = (W + tc - 1) / tc;
    hipLaunchKernelGGL(box_col_kernel, dim3(grid_for(nimg * tiles, 1 << 16)), dim3(256), 2 * col_buf, as_stream(stream), src, dst,
                       static_cast<const uint8_t*>(workspace), params, nimg * tiles, H, W, tc, tiles, col_buf);
    MUMPY_CHECK_LAUNCH("gaussian_blur_u8 (columns)");
    return 0;
}

extern "C" int mumpy_resize_nearest_u8_fwd(const uint8_t* src, uint8_t* dst, const int32_t* ytab, const int32_t* xtab, int64_t nimg,
                                           int Hs, int Ws, int H, int W, int C, void* stream) {
    MUMPY_REQUIRE(src && dst && ytab && xtab, MUMPY_ENULL, "resize_nearest_u8: null pointer");
    MUMPY_REQUIRE(nimg >= 0 && Hs >= 1 && Ws >= 1 && H >= 1 && W >= 1 && C >= 1 && C <= 4, MUMPY_EINVAL,
                  "resize_nearest_u8: bad sizes nimg=%lld, %dx%d -> %dx%d, %d channels (1 .. 4)", (long long)nimg, Hs, Ws, H, W, C);
    MUMPY_REQUIRE(((reinterpret_cast<uintptr_t>(ytab) | reinterpret_cast<uintptr_t>(xtab)) & 3u) == 0, MUMPY_EALIGN,
                  "resize_nearest_u8: the tables must be 4-byte aligned");
    MUMPY_REQUIRE(nimg < LIM31 && C * (int64_t)Hs * Ws < LIM31 && C * (int64_t)H * W < LIM31, MUMPY_ERANGE,
                  "resize_nearest_u8: nimg=%lld, C*%d*%d or C*%d*%d is 2^31 or more", (long long)nimg, Hs, Ws, H, W);
    if (nimg == 0) return 0;
    const int64_t total = nimg * H * W;
    hipLaunchKernelGGL(resize_nearest_u8_kernel, dim3(grid_for((total + 255) / 256, 1 << 16)), dim3(256), 0, as_stream(stream), src, dst,
                       ytab, xtab, total, Hs, Ws, H, W, C);
    MUMPY_CHECK_LAUNCH("resize_nearest_u8");
    return 0;
}
