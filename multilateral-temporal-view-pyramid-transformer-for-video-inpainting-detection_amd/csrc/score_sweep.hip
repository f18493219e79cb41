// score_sweep.hip — a whole video scored at every threshold of a table in one pass (include/mumpy_hip_ext7.h; host:
// mumpy_hip/video.py, VideoPredictor(sweep=...)).  The forward's last kernel cuts the mask at ONE threshold; the logits, the
// annotation bank and the clip-to-frame table are all on the device while the graph runs, so two more launches give what a forward
// per candidate threshold would:
//   score_exceed_kernel   per frame and class, the number of pixels whose probability exceeds each threshold: one workgroup per clip,
//                         a histogram over the K + 1 bins #{k : p > t_k} in LDS, then a suffix sum;
//   sweep_metrics_kernel  per threshold, F1 / IoU of the four counts in fp64 summed over the frames in a fixed order (the expression
//                         of frame_metrics_kernel: frame_metric.h), and the counts pooled over the frames in int64.
// The probability and the comparison are those of final_conv_kernel (sigmoid_thr.h): the counts at t_k are the counts of the mask at
// thr = t_k bit for bit.  ~250 KB per clip and a few hundred KB per video; one workgroup per clip on purpose (written, not
// accumulated; no arrival order): 61 us per batch of 8 beside a 21 ms forward, 10 us per video (profiles/threshold_sweep.md).
#include "common.h"
#include "sigmoid_thr.h"
#include "frame_metric.h"
#include "../../include/mumpy_hip_ext7.h"
using namespace mumpy;

namespace {

constexpr int NBIN = MUMPY_SWEEP_MAX_THRESHOLDS + 1;        // bins per class at the cap
constexpr int NWAVE = 256 / WAVE;

__device__ __forceinline__ int wave_sum_i(int v) {
#pragma unroll
    for (int s = 1; s < WAVE; s <<= 1) v += __shfl_xor(v, s);
    return v;
}

// One workgroup per clip (a grid-stride walk only past 65536 clips); dest[c] is uniform over the workgroup, so a dropped clip is
// skipped as a whole, before any barrier.
// A pixel's bin is b = #{k : p > t_k} in 0 .. K.  With the usual sparse masks nearly every pixel lands in bin 0 (and a confident
// model puts most of the rest in bin K): those two are counted in REGISTERS, per thread, and meet in one wave reduce; only the bins
// in between go to LDS, as integer atomics into a histogram of the thread's own wave (4 x 2 x 1024 x 4 B = 32 KB at the cap), so
// that the four waves never contend.  Integer sums: no order shows in the result.
// The search is a comparison search with the contract's own strict `>`, never arithmetic on p: a lower bound whose step count
// depends on K alone, so the loop is uniform and a thread's 16 pixels walk it side by side (16 independent LDS reads per step
// hide each other's latency; a search per pixel inside a divergent branch took 145 us per launch at (8, 224 x 224, K = 255), this
// form takes 61: profiles/threshold_sweep.md).  It is bounded for ANY table: base + n <= K holds throughout, so every index read
// (base + half - 1, then base) is at most K - 1 and the bin at most K; whatever the table holds, each pixel adds one to exactly
// one bin of its class, so every value written is a sum of bin counts: in [0, npix].
__global__ __launch_bounds__(256) void score_exceed_kernel(const float* __restrict__ logits, const uint8_t* __restrict__ gt,
                                                           const int32_t* __restrict__ dest, const float* __restrict__ thr_tab,
                                                           int32_t* __restrict__ exceed, int nclips, int npix, int nbank, int K) {
    __shared__ float tab[NBIN];
    __shared__ int hist[NWAVE][2][NBIN];
    __shared__ int scan[2][256];
    const int tid = threadIdx.x, wave = tid / WAVE;
    for (int i = tid; i < K; i += 256) tab[i] = thr_tab[i];
    __syncthreads();
    int* mine = &hist[wave][0][0];
    for (int c = blockIdx.x; c < nclips; c += gridDim.x) {
        const int d = dest[c];
        if (d < 0 || d >= nbank) continue;
        for (int i = tid; i <= K; i += 256) {
#pragma unroll
            for (int w = 0; w < NWAVE; ++w) { hist[w][0][i] = 0; hist[w][1][i] = 0; }
        }
        __syncthreads();
        const f32x4* l4 = reinterpret_cast<const f32x4*>(logits + (int64_t)c * npix);
        const uint4* g4 = reinterpret_cast<const uint4*>(gt + (int64_t)d * npix);
        int none[2] = {0, 0}, all[2] = {0, 0};               // bin 0 and bin K of class 0 / 1
        for (int i = tid; i < (npix >> 4); i += 256) {
            const uint4 gv = g4[i];
            const uint32_t gw[4] = {gv.x, gv.y, gv.z, gv.w};
            float p[16];
            int base[16];
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const f32x4 z = l4[4 * i + q];
#pragma unroll
                for (int j = 0; j < 4; ++j) { p[4 * q + j] = sigmoid_prob(z[j]); base[4 * q + j] = 0; }
            }
            for (int n = K; n > 1;) {                        // the first k of [base, base + n) that p does not exceed, if any
                const int half = n >> 1;
#pragma unroll
                for (int u = 0; u < 16; ++u) base[u] = prob_exceeds(p[u], tab[base[u] + half - 1]) ? base[u] + half : base[u];
                n -= half;
            }
#pragma unroll
            for (int u = 0; u < 16; ++u) {
                const int bin = base[u] + (prob_exceeds(p[u], tab[base[u]]) ? 1 : 0);
                const int g = ((gw[u >> 2] >> (8 * (u & 3))) & 0xffu) != 0u ? 1 : 0;
                if (bin == 0) none[g] += 1;
                else if (bin == K) all[g] += 1;
                else atomicAdd(&mine[g * NBIN + bin], 1);
            }
        }
#pragma unroll
        for (int g = 0; g < 2; ++g) { none[g] = wave_sum_i(none[g]); all[g] = wave_sum_i(all[g]); }
        if ((tid & (WAVE - 1)) == 0) {                       // bins 0 and K saw no atomic (for K == 1 they are all there is)
            mine[0] = none[0]; mine[NBIN] = none[1];
            mine[K] = all[0]; mine[NBIN + K] = all[1];
        }
        __syncthreads();
        // thread t owns bins 4 t .. 4 t + 3 of both classes: the four waves summed, then a suffix sum over the threads
        int v[2][4], own[2];
#pragma unroll
        for (int g = 0; g < 2; ++g) {
            own[g] = 0;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int b = 4 * tid + j;
                v[g][j] = b <= K ? hist[0][g][b] + hist[1][g][b] + hist[2][g][b] + hist[3][g][b] : 0;
                own[g] += v[g][j];
            }
            scan[g][tid] = own[g];
        }
        __syncthreads();
        for (int off = 1; off < 256; off <<= 1) {
            const int a0 = tid + off < 256 ? scan[0][tid + off] : 0, a1 = tid + off < 256 ? scan[1][tid + off] : 0;
            __syncthreads();
            scan[0][tid] += a0; scan[1][tid] += a1;
            __syncthreads();
        }
        // exceed[k] = the pixels in bins k + 1 .. K; exceed[K] = all of them
#pragma unroll
        for (int g = 0; g < 2; ++g) {
            int32_t* row = exceed + ((int64_t)d * 2 + g) * (K + 1);
            int tail = scan[g][tid] - own[g];                // the bins of the threads above this one
#pragma unroll
            for (int j = 3; j >= 0; --j) {
                const int b = 4 * tid + j;
                tail += v[g][j];
                if (b >= 1 && b <= K) row[b - 1] = tail;
            }
            if (tid == 0) row[K] = scan[g][0];
        }
        __syncthreads();                                     // the next clip of this workgroup reuses hist and scan
    }
}

// Workgroups 0 .. K - 1: one threshold each; thread i adds frames i, i + 256, ... in order, then a fixed tree over the 256 partial
// sums (the walk of frame_metrics_kernel).  The workgroups behind them: one column of pooled per thread, summed in frame order.
__global__ __launch_bounds__(256) void sweep_metrics_kernel(const int32_t* __restrict__ exceed, int nscored, int K, double eps_g,
                                                            double* __restrict__ acc, int64_t* __restrict__ pooled, int accumulate) {
    __shared__ double red[256][2];
    const int tid = threadIdx.x, width = 2 * (K + 1);
    if ((int)blockIdx.x >= K) {                              // (launched only when pooled is given)
        const int col = ((int)blockIdx.x - K) * 256 + tid;
        if (col < width) {
            int64_t s = 0;
            for (int f = 0; f < nscored; ++f) s += exceed[(int64_t)f * width + col];
            pooled[col] = accumulate ? pooled[col] + s : s;
        }
        return;
    }
    const int k = blockIdx.x;
    double f1 = 0.0, iou = 0.0;
    for (int f = tid; f < nscored; f += 256) {
        const int32_t* e = exceed + (int64_t)f * width;
        const double inter = (double)e[K + 1 + k], sp = (double)e[k] + inter, sg = (double)e[K + 1 + K], uni = sp + sg - inter;
        double ff, fi;
        frame_f1_iou(inter, sp, sg, uni, eps_g, ff, fi);
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
        double* a = acc + 3 * (int64_t)k;
        const double n = (double)nscored;
        if (accumulate) { a[0] += red[0][0]; a[1] += red[0][1]; a[2] += n; }
        else { a[0] = red[0][0]; a[1] = red[0][1]; a[2] = n; }
    }
}

constexpr int64_t LIM = (int64_t)1 << 31;
inline bool aligned8(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 7u) == 0; }

}  // namespace

extern "C" int mumpy_score_exceed_fwd(const float* logits, const uint8_t* gt, const int32_t* dest, const float* thr_tab,
                                      int32_t* exceed, int64_t nclips, int64_t npix, int64_t nbank, int K, void* stream) {
    MUMPY_REQUIRE(logits && gt && dest && thr_tab && exceed, MUMPY_ENULL, "score_exceed: null pointer");
    MUMPY_REQUIRE(nclips >= 0 && npix >= 1 && npix % 16 == 0 && nbank >= 1 && K >= 1 && K <= MUMPY_SWEEP_MAX_THRESHOLDS, MUMPY_EINVAL,
                  "score_exceed: bad sizes nclips=%lld npix=%lld nbank=%lld K=%d (npix must be a multiple of 16, K in 1 .. %d)",
                  (long long)nclips, (long long)npix, (long long)nbank, K, MUMPY_SWEEP_MAX_THRESHOLDS);
    MUMPY_REQUIRE(aligned16(logits) && aligned16(gt) && aligned16(thr_tab) && aligned16(exceed), MUMPY_EALIGN,
                  "score_exceed: logits, gt, thr_tab and exceed must be 16-byte aligned");
    MUMPY_REQUIRE(nclips < LIM && npix < LIM && nbank < LIM && nbank * 2 * (int64_t)(K + 1) < LIM, MUMPY_ERANGE,
                  "score_exceed: nclips=%lld, npix=%lld, nbank=%lld or nbank*2*(K+1) at K=%d is 2^31 or more (dest, the counts and the "
                  "offsets into exceed are 32-bit)", (long long)nclips, (long long)npix, (long long)nbank, K);
    if (nclips == 0) return 0;
    hipLaunchKernelGGL(score_exceed_kernel, dim3((unsigned)(nclips < 65536 ? nclips : 65536)), dim3(256), 0, as_stream(stream), logits,
                       gt, dest, thr_tab, exceed, (int)nclips, (int)npix, (int)nbank, K);
    MUMPY_CHECK_LAUNCH("score_exceed");
    return 0;
}

extern "C" int mumpy_sweep_metrics_fwd(const int32_t* exceed, int64_t nscored, int64_t npix, int K, double* acc, int64_t* pooled,
                                       int accumulate, void* stream) {
    MUMPY_REQUIRE(exceed && acc, MUMPY_ENULL, "sweep_metrics: null pointer");
    MUMPY_REQUIRE(nscored >= 0 && npix >= 1 && K >= 1 && K <= MUMPY_SWEEP_MAX_THRESHOLDS, MUMPY_EINVAL,
                  "sweep_metrics: bad sizes nscored=%lld npix=%lld K=%d (K in 1 .. %d)", (long long)nscored, (long long)npix, K,
                  MUMPY_SWEEP_MAX_THRESHOLDS);
    MUMPY_REQUIRE(aligned8(acc) && aligned8(pooled), MUMPY_EALIGN, "sweep_metrics: acc and pooled must be 8-byte aligned");
    MUMPY_REQUIRE(nscored < LIM && npix < LIM && nscored * 2 * (int64_t)(K + 1) < LIM, MUMPY_ERANGE,
                  "sweep_metrics: nscored=%lld, npix=%lld or nscored*2*(K+1) at K=%d is 2^31 or more", (long long)nscored, (long long)npix,
                  K);
    const int grid = K + (pooled ? (2 * (K + 1) + 255) / 256 : 0);
    hipLaunchKernelGGL(sweep_metrics_kernel, dim3((unsigned)grid), dim3(256), 0, as_stream(stream), exceed, (int)nscored, K,
                       1e-6 * (double)npix, acc, pooled, accumulate != 0 ? 1 : 0);
    MUMPY_CHECK_LAUNCH("sweep_metrics");
    return 0;
}
