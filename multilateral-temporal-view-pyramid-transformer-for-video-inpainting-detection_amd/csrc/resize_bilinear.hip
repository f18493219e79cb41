// resize_bilinear.hip — Pillow's 8-bit Image.resize(BILINEAR) of single-channel images on the device (include/mumpy_hip_ext6.h; host:
// mumpy_hip/video.py::bilinear_taps / bilinear_resize).  The reference resizes every annotation to 224 x 224 this way before it scores
// a frame (measure.py:21-40, 77); VideoPredictor(gt_hw=...) does it here, so that annotations arrive at their own size.
//
// Pillow runs two integer passes, horizontal then vertical, each clip8((2^21 + sum coef * src) >> 22) over a triangle filter that is
// stretched by the scale (a 1920 -> 224 pass has 19 taps), and rounds the image between them to uint8.  One workgroup takes a band of
// R output rows of one image: it runs the horizontal pass over just the source rows that band's vertical taps reach, keeps them in LDS
// as uint8 (W bytes per row), and runs the vertical pass out of LDS.  The full-size intermediate never reaches memory, and a source
// row is read once per band that needs it: (R * scale + taps) / (R * scale) times in all.
//
// The horizontal pass is where the work is (rows-in-band x W x taps products against R x W x taps of the vertical pass).  A thread
// takes one output column of FOUR consecutive intermediate rows, so that a coefficient is loaded once per four products; neighbouring
// lanes take neighbouring columns, so a wave's byte loads of one tap fall into 64 * scale consecutive bytes of a source row.
#include "common.h"
#include "../../include/mumpy_hip_ext6.h"
using namespace mumpy;

namespace {

constexpr int BAND = 16;             // output rows per workgroup, halved until the band's intermediate rows fit MUMPY_RESIZE_BAND_BYTES

// The clamps are unconditional: the tables are device memory that nobody validated.
__device__ __forceinline__ int clampi(int v, int hi) { return v < 0 ? 0 : (v > hi ? hi : v); }

// Pillow's clip8 of a pass's sum.  The sum is formed modulo 2^32 (unsigned: tables that are not Pillow's may wrap) and read as signed.
__device__ __forceinline__ uint8_t clip8(uint32_t acc) { return (uint8_t)clampi((int)acc >> 22, 255); }

__global__ __launch_bounds__(256) void resize_bilinear_u8_kernel(const uint8_t* __restrict__ src, uint8_t* __restrict__ out,
                                                                 const int32_t* __restrict__ ystart, const int32_t* __restrict__ ycount,
                                                                 const int32_t* __restrict__ ycoef, const int32_t* __restrict__ xstart,
                                                                 const int32_t* __restrict__ xcount, const int32_t* __restrict__ xcoef,
                                                                 int nwork, int nbands, int R, int nrcap, int Hs, int Ws, int H, int W,
                                                                 int ykmax, int xkmax) {
    extern __shared__ __align__(16) uint8_t rows[];          // (nrcap, W): the band's intermediate rows
    const int tid = threadIdx.x;
    for (int64_t w = blockIdx.x; w < nwork; w += gridDim.x) {
        const int f = (int)(w / nbands), y0 = (int)(w - (int64_t)f * nbands) * R, y1 = R < H - y0 ? y0 + R : H;
        // the source rows this band reads: [lo, hi), at most nrcap of them (the host sized nrcap so that Pillow's taps always fit)
        int lo = Hs, hi = 0;
        for (int y = y0; y < y1; ++y) {
            const int s = clampi(ystart[y], Hs - 1), c = clampi(ycount[y], ykmax);
            if (c > 0) {
                const int e = c < Hs - s ? s + c : Hs;
                lo = s < lo ? s : lo;
                hi = e > hi ? e : hi;
            }
        }
        if (hi - lo > nrcap) hi = lo + nrcap;
        const int nr = hi > lo ? hi - lo : 0;                // 0: every count of the band is 0, and nothing is read below
        const uint8_t* fsrc = src + (int64_t)f * Hs * Ws;

        // horizontal pass: (row quad, column) per thread
        const int nq = (nr + 3) >> 2;
        for (int i = tid; i < nq * W; i += 256) {            // nq * W <= (nrcap + 3) * W: far below 2^31
            const int q = i / W, x = i - q * W, r = 4 * q;   // rows lo + r .. lo + r + 3, the ones past hi - 1 folded onto it
            const int sx = clampi(xstart[x], Ws - 1), cx = clampi(xcount[x], xkmax);
            const int32_t* cf = xcoef + x * xkmax;
            const int last = nr - 1;
            const uint8_t* p0 = fsrc + (lo + r) * Ws;
            const uint8_t* p1 = fsrc + (lo + (r + 1 < last ? r + 1 : last)) * Ws;
            const uint8_t* p2 = fsrc + (lo + (r + 2 < last ? r + 2 : last)) * Ws;
            const uint8_t* p3 = fsrc + (lo + (r + 3 < last ? r + 3 : last)) * Ws;
            uint32_t a0 = 1u << 21, a1 = a0, a2 = a0, a3 = a0;
            for (int k = 0; k < cx; ++k) {
                const int xx = k < Ws - sx ? sx + k : Ws - 1;
                const uint32_t c = (uint32_t)cf[k];
                a0 += c * p0[xx]; a1 += c * p1[xx]; a2 += c * p2[xx]; a3 += c * p3[xx];
            }
            uint8_t* d = rows + r * W + x;
            d[0] = clip8(a0);
            if (r + 1 < nr) d[W] = clip8(a1);
            if (r + 2 < nr) d[2 * W] = clip8(a2);
            if (r + 3 < nr) d[3 * W] = clip8(a3);
        }
        __syncthreads();

        // vertical pass out of LDS: (output row, column) per thread, consecutive lanes on consecutive bytes
        uint8_t* fout = out + (int64_t)f * H * W;
        for (int i = tid; i < (y1 - y0) * W; i += 256) {
            const int yy = i / W, x = i - yy * W, y = y0 + yy;
            const int s = clampi(ystart[y], Hs - 1), c = nr > 0 ? clampi(ycount[y], ykmax) : 0;
            const int32_t* cf = ycoef + y * ykmax;
            uint32_t a = 1u << 21;
            for (int k = 0; k < c; ++k) {
                int r = k < hi - s ? s + k : hi - 1;         // into [lo, hi): a no-op for Pillow's taps
                r = (r < lo ? lo : r) - lo;
                a += (uint32_t)cf[k] * rows[r * W + x];
            }
            fout[y * W + x] = clip8(a);
        }
        __syncthreads();                                     // the next band of this workgroup overwrites rows
    }
}

constexpr int64_t LIM = (int64_t)1 << 31;
inline bool aligned4(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 3u) == 0; }

// intermediate rows a band of R output rows can read with Pillow's taps: the centres of its first and last row lie (R - 1) * Hs / H
// apart, each reaches `support` to either side, and kmax = 2 * ceil(support) + 1
inline int64_t band_rows(int R, int Hs, int H, int ykmax) {
    const int64_t n = ((int64_t)(R - 1) * Hs) / H + ykmax + 1;
    return n < Hs ? n : Hs;
}

}  // namespace

extern "C" int mumpy_resize_bilinear_u8_fwd(const uint8_t* src, uint8_t* out, const int32_t* ystart, const int32_t* ycount,
                                            const int32_t* ycoef, const int32_t* xstart, const int32_t* xcount, const int32_t* xcoef,
                                            int64_t n, int Hs, int Ws, int H, int W, int ykmax, int xkmax, void* stream) {
    MUMPY_REQUIRE(src && out && ystart && ycount && ycoef && xstart && xcount && xcoef, MUMPY_ENULL,
                  "resize_bilinear_u8: null pointer");
    MUMPY_REQUIRE(n >= 0 && Hs >= 1 && Ws >= 1 && H >= 1 && W >= 1, MUMPY_EINVAL,
                  "resize_bilinear_u8: bad sizes n=%lld, %dx%d -> %dx%d", (long long)n, Hs, Ws, H, W);
    MUMPY_REQUIRE(ykmax >= 1 && ykmax <= MUMPY_RESIZE_KMAX_CAP && xkmax >= 1 && xkmax <= MUMPY_RESIZE_KMAX_CAP, MUMPY_EINVAL,
                  "resize_bilinear_u8: ykmax=%d and xkmax=%d must be in 1 .. %d", ykmax, xkmax, MUMPY_RESIZE_KMAX_CAP);
    MUMPY_REQUIRE(aligned4(ystart) && aligned4(ycount) && aligned4(ycoef) && aligned4(xstart) && aligned4(xcount) && aligned4(xcoef),
                  MUMPY_EALIGN, "resize_bilinear_u8: the tables must be 4-byte aligned");
    MUMPY_REQUIRE(n < LIM && (int64_t)Hs * Ws < LIM && (int64_t)H * W < LIM && (int64_t)H * ykmax < LIM && (int64_t)W * xkmax < LIM,
                  MUMPY_ERANGE, "resize_bilinear_u8: n=%lld, %d*%d, %d*%d, %d*%d or %d*%d is 2^31 or more (32-bit offsets)",
                  (long long)n, Hs, Ws, H, W, H, ykmax, W, xkmax);
    MUMPY_REQUIRE(n * H < LIM, MUMPY_ERANGE, "resize_bilinear_u8: n*H=%lld*%d is 2^31 or more (bands are numbered in 32 bits)",
                  (long long)n, H);
    MUMPY_REQUIRE(band_rows(1, Hs, H, ykmax) * W <= MUMPY_RESIZE_BAND_BYTES, MUMPY_EINVAL,
                  "resize_bilinear_u8: min(ykmax + 1, Hs) * W = %lld bytes of intermediate rows exceed the band's %d",
                  (long long)(band_rows(1, Hs, H, ykmax) * W), MUMPY_RESIZE_BAND_BYTES);
    if (n == 0) return 0;
    int R = BAND;
    while (R > 1 && band_rows(R, Hs, H, ykmax) * W > MUMPY_RESIZE_BAND_BYTES) R >>= 1;
    const int nrcap = (int)band_rows(R, Hs, H, ykmax);
    const int nbands = (H + R - 1) / R;
    const int64_t nwork = n * nbands;                        // <= n * H < 2^31
    const unsigned grid = (unsigned)(nwork < 65536 ? nwork : 65536);
    hipLaunchKernelGGL(resize_bilinear_u8_kernel, dim3(grid), dim3(256), (size_t)nrcap * W, as_stream(stream), src, out, ystart, ycount,
                       ycoef, xstart, xcount, xcoef, (int)nwork, nbands, R, nrcap, Hs, Ws, H, W, ykmax, xkmax);
    MUMPY_CHECK_LAUNCH("resize_bilinear_u8");
    return 0;
}
