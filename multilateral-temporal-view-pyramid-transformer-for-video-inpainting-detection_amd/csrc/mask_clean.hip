// mask_clean.hip — cleaning predicted masks on the device (include/mumpy_postprocess.h): components below min_area removed, then
// holes up to max_hole filled.  mumpy_hip/postprocess.py is the numpy statement and DESIGN.md ("Mask cleaning") gives the reasoning.
//
// One launch, one workgroup of 1024 lanes per image (a grid-stride walk over the images), the frame's label image in LDS:
//   * L[p], 16 bits per pixel: the index of another pixel of p's component that is not above p (a link), p itself for a root, or a
//     mark >= FG for a pixel outside the set being labelled.  H * W <= 50176 < 0xFFFE, so an index never collides with a mark, and
//     the whole image takes at most 100,352 B (+ 6,272 B of decision bits) of the 160 KB a workgroup may hold on gfx950.
//   * labelling is union-find on that array: lane t first links the pixels of its own chunk of K consecutive pixels along the row
//     (plain stores, nobody else touches the chunk), then every pixel is united with its left neighbour across a chunk boundary and
//     with the row above (up; for connectivity 8 up-left / up-right where up is background), skipping the unions the neighbour to the
//     left already implies.  A union hooks the larger root under the smaller with a 16-bit minimum, done as a compare-and-swap on the
//     32-bit word that holds it.  Links only ever decrease, so the final root of a component is its first pixel in raster order
//     whatever the order of the unions: the labels, and everything derived from them, are the same on every run.
//   * areas live in the caller's workspace, 4 * H * W bytes per workgroup: the kernel zeroes the roots' words, every lane adds the
//     runs of equal roots of its chunk (integer atomics at the L2; a border pixel also adds 1 << 16, so bits 16 .. 30 count a
//     component's border pixels -- at most 2 (H + W) < 2^15), and the words are read back past the L1.
//   * a component's decision (keep; fill) is taken once, at its root, from the area word -- eight loads in flight per lane -- and
//     left as one bit per pixel index in H * W / 8 more bytes of LDS, where the other pixels of the component read it.
//   * pass 1 labels the foreground, drops components below min_area and re-marks the array for pass 2, which labels the background
//     of the result with the complementary connectivity and fills the components that have no border pixel and fit max_hole.
//   * the output pass turns 16 labels into 16 bytes per lane, one 16-byte store, and counts against gt on the way.
//
// LOOP BOUNDS.  Three loops have a trip count that depends on the image; each carries its bound beside it (find_root: H * W;
// min16 and unite: 2 * H * W).  A lane that reaches one raises the workgroup's flag; at the next barrier the workgroup gives up on
// the image: it copies the raw mask to out as 0 / 255 and writes status 1.  No other loop depends on the image's content.
#include "common.h"
#include "../../include/mumpy_postprocess.h"
using namespace mumpy;

namespace {

constexpr int THREADS = 1024;
constexpr int GRID_MAX = 256;                            // one workgroup per CU at the largest image; the workspace scales with it
constexpr int MAX_PIXELS = MUMPY_MASK_CLEAN_MAX_PIXELS;
constexpr int64_t LIM31 = (int64_t)1 << 31;
constexpr uint32_t FG = 0xFFFEu;                         // pass 2: a foreground pixel (not labelled)
constexpr uint32_t NONE = 0xFFFFu;                       // pass 1: a background pixel (not labelled)
constexpr uint32_t BORDER_ONE = 1u << 16;

__device__ __forceinline__ bool in_set(uint32_t v) { return v < FG; }

__device__ __forceinline__ uint32_t find_root(const volatile uint16_t* L, uint32_t p, int HW, volatile int* bail) {
    // BOUND H * W: a link points to a smaller index, so a chain visits a pixel at most once
    for (int it = 0; it < HW; ++it) {
        const uint32_t q = L[p];
        if (q >= p) return p;                            // q == p: a root (q > p never happens; it would end the walk all the same)
        p = q;
    }
    *bail = 1;
    return p;
}

// L[idx] = min(L[idx], val) on the 16-bit half of its 32-bit word; returns the value before.
__device__ __forceinline__ uint32_t min16(uint16_t* L, uint32_t idx, uint32_t val, int HW, volatile int* bail) {
    uint32_t* word = reinterpret_cast<uint32_t*>(L) + (idx >> 1);
    const int sh = (int)(idx & 1u) * 16;
    uint32_t old = *reinterpret_cast<volatile uint32_t*>(word);
    // BOUND 2 * H * W: a retry means another lane lowered one of the word's two halves, and a half can fall at most H * W times
    for (int it = 0; it < 2 * HW; ++it) {
        const uint32_t cur = (old >> sh) & 0xFFFFu;
        if (cur <= val) return cur;
        const uint32_t got = atomicCAS(word, old, (old & ~(0xFFFFu << sh)) | (val << sh));
        if (got == old) return cur;
        old = got;
    }
    *bail = 1;
    return val;
}

__device__ __forceinline__ void unite(uint16_t* L, uint32_t a, uint32_t b, int HW, volatile int* bail) {
    // BOUND 2 * H * W: a round that does not finish replaces a or b by a smaller index, so a + b falls with every round
    for (int it = 0; it < 2 * HW; ++it) {
        a = find_root(L, a, HW, bail);
        b = find_root(L, b, HW, bail);
        if (a == b || *bail) return;
        if (a > b) { const uint32_t t = a; a = b; b = t; }
        const uint32_t old = min16(L, b, a, HW, bail);
        if (old == b) return;                            // b was still a root and now hangs under a
        b = old;                                         // somebody hooked b first: go on from where it points
    }
    *bail = 1;
}

// Labels the set {p : L[p] < FG} (L[p] == p on entry for its pixels) and leaves area[root] = pixels | border pixels << 16 for every
// root.  Returns false, for the whole workgroup, when a lane reached a loop bound.
__device__ bool label_pass(uint16_t* L, uint32_t* area, int H, int W, int K, bool conn8, volatile int* bail) {
    const int HW = H * W, tid = (int)threadIdx.x;
    const volatile uint16_t* Lv = L;
    const int p0 = tid * K, p1 = min(p0 + K, HW);
    if (p0 < HW) {                                       // row links inside the lane's own chunk
        int x = p0 % W;
        uint32_t prev = NONE;
        for (int p = p0; p < p1; ++p) {
            uint32_t v = Lv[p];
            if (in_set(v) && x > 0 && in_set(prev)) { v = prev; L[p] = (uint16_t)v; }
            prev = v;
            if (++x == W) x = 0;
        }
    }
    __syncthreads();
    for (int p = tid; p < HW; p += THREADS) {
        if (!in_set(Lv[p])) continue;
        const int y = p / W, x = p - y * W;
        const bool left = x > 0 && in_set(Lv[p - 1]);
        if (left && p % K == 0) unite(L, p, p - 1, HW, bail);
        if (y > 0) {
            const bool up = in_set(Lv[p - W]), upleft = x > 0 && in_set(Lv[p - W - 1]);
            if (up) {
                if (!(left && upleft)) unite(L, p, p - W, HW, bail);          // else left -- upleft -- up already joins them
            } else if (conn8) {
                if (upleft && !left) unite(L, p, p - W - 1, HW, bail);         // with left set, left -- upleft is left's own `up`
                if (x < W - 1 && in_set(Lv[p - W + 1])) unite(L, p, p - W + 1, HW, bail);
            }
        }
    }
    __syncthreads();
    for (int p = tid; p < HW; p += THREADS) {            // flatten; a root's area word is zeroed
        if (!in_set(Lv[p])) continue;
        const uint32_t r = find_root(L, p, HW, bail);
        if (r == (uint32_t)p) __hip_atomic_store(area + p, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        else L[p] = (uint16_t)r;
    }
    __threadfence();
    __syncthreads();
    if (*bail) return false;                             // uniform: nothing writes the flag after the barrier
    if (p0 < HW) {
        int y = p0 / W, x = p0 - y * W;
        uint32_t cur = NONE, acc = 0;
        for (int p = p0; p < p1; ++p) {
            const uint32_t v = Lv[p];
            if (in_set(v)) {
                const uint32_t add = 1u + ((x == 0 || y == 0 || x == W - 1 || y == H - 1) ? BORDER_ONE : 0u);
                if (v == cur) acc += add;
                else {
                    if (acc) __hip_atomic_fetch_add(area + cur, acc, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                    cur = v;
                    acc = add;
                }
            }
            if (++x == W) { x = 0; ++y; }
        }
        if (acc) __hip_atomic_fetch_add(area + cur, acc, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    __threadfence();
    __syncthreads();
    return true;
}

__device__ __forceinline__ uint32_t area_word(const uint32_t* area, uint32_t root) {
    return __hip_atomic_load(area + root, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

constexpr int BATCH = 8;                                 // area words in flight per lane: a trip to the L2 each

// Calls f(root, area word) for every root of the labelled set, BATCH loads in flight per lane.
template <typename F>
__device__ __forceinline__ void for_each_root(const uint16_t* L, const uint32_t* area, int HW, F f) {
    for (int base = (int)threadIdx.x; base < HW; base += THREADS * BATCH) {
        bool root[BATCH];
        uint32_t w[BATCH];
#pragma unroll
        for (int j = 0; j < BATCH; ++j) {
            const int p = base + j * THREADS;
            root[j] = p < HW && L[p] == (uint16_t)p;
        }
#pragma unroll
        for (int j = 0; j < BATCH; ++j) w[j] = root[j] ? area_word(area, (uint32_t)(base + j * THREADS)) : 0u;
#pragma unroll
        for (int j = 0; j < BATCH; ++j)
            if (root[j]) f((uint32_t)(base + j * THREADS), w[j]);
    }
}

__global__ __launch_bounds__(THREADS) void mask_clean_kernel(const uint8_t* mask, uint8_t* out, const uint8_t* __restrict__ gt,
                                                             int32_t* __restrict__ counts, int32_t* __restrict__ stats,
                                                             const int32_t* __restrict__ params, uint32_t* __restrict__ workspace,
                                                             int64_t nimg, int H, int W) {
    extern __shared__ __align__(16) uint16_t L[];        // H * W labels, then one decision bit per pixel index (read at the roots')
    __shared__ int s_bail;
    __shared__ int s_stat[8];
    __shared__ int s_cnt[4];
    const int HW = H * W, tid = (int)threadIdx.x;
    const int K = (HW + THREADS - 1) / THREADS;
    uint32_t* area = workspace + (int64_t)blockIdx.x * HW;
    uint32_t* bits = reinterpret_cast<uint32_t*>(L + HW);
    const int nwords = (HW + 31) >> 5;
    for (int64_t img = blockIdx.x; img < nimg; img += gridDim.x) {
        const int4 row = *reinterpret_cast<const int4*>(params + img * 4);       // uniform over the workgroup
        const int min_area = row.x, max_hole = row.y;
        const bool conn8 = row.z != 4;
        const uint8_t* m = mask + img * HW;
        if (tid < 8) s_stat[tid] = 0;
        if (tid < 4) s_cnt[tid] = 0;
        if (tid == 0) s_bail = 0;
        for (int i = tid; i < nwords; i += THREADS) bits[i] = 0;
        for (int i = tid * 16; i < HW; i += THREADS * 16) {
            const uint4 v = *reinterpret_cast<const uint4*>(m + i);
            const uint32_t w[4] = {v.x, v.y, v.z, v.w};
            uint32_t pair[8];
#pragma unroll
            for (int k = 0; k < 8; ++k) {
                const uint32_t lo = (w[k >> 1] >> (16 * (k & 1))) & 0xFFu, hi = (w[k >> 1] >> (16 * (k & 1) + 8)) & 0xFFu;
                pair[k] = (lo ? (uint32_t)(i + 2 * k) : NONE) | ((hi ? (uint32_t)(i + 2 * k + 1) : NONE) << 16);
            }
            uint4* dst = reinterpret_cast<uint4*>(L + i);
            dst[0] = make_uint4(pair[0], pair[1], pair[2], pair[3]);
            dst[1] = make_uint4(pair[4], pair[5], pair[6], pair[7]);
        }
        __syncthreads();
        bool ok = label_pass(L, area, H, W, K, conn8, &s_bail);
        if (ok) {
            int found = 0, kept = 0, removed = 0, largest = 0;
            for_each_root(L, area, HW, [&](uint32_t r, uint32_t w) {     // the decision of a component, taken at its root
                const int a = (int)(w & 0xFFFFu);
                ++found;
                if (a >= min_area) { ++kept; largest = max(largest, a); atomicOr(&bits[r >> 5], 1u << (r & 31u)); }
                else removed += a;
            });
            if (found) { atomicAdd(&s_stat[0], found); atomicAdd(&s_stat[1], kept); atomicAdd(&s_stat[2], removed); atomicMax(&s_stat[5], largest); }
            __syncthreads();
            for (int p = tid; p < HW; p += THREADS) {    // a lane rewrites its own pixels only; roots are read through the bits
                const uint32_t v = L[p];
                const bool keep = in_set(v) && ((bits[v >> 5] >> (v & 31u)) & 1u);
                L[p] = (uint16_t)(keep ? FG : (uint32_t)p);     // what is not kept is the background pass 2 labels
            }
            __syncthreads();
            if (max_hole != 0) {
                for (int i = tid; i < nwords; i += THREADS) bits[i] = 0;     // (label_pass has barriers before the bits are set again)
                ok = label_pass(L, area, H, W, K, !conn8, &s_bail);
                if (ok) {
                    int holes = 0, pixels = 0;
                    for_each_root(L, area, HW, [&](uint32_t r, uint32_t w) {
                        const int a = (int)(w & 0xFFFFu);
                        if ((w >> 16) == 0 && (max_hole < 0 || a <= max_hole)) { ++holes; pixels += a; atomicOr(&bits[r >> 5], 1u << (r & 31u)); }
                    });
                    if (holes) { atomicAdd(&s_stat[3], holes); atomicAdd(&s_stat[4], pixels); }
                    __syncthreads();
                    for (int p = tid; p < HW; p += THREADS) {
                        const uint32_t v = L[p];
                        if (in_set(v) && ((bits[v >> 5] >> (v & 31u)) & 1u)) L[p] = (uint16_t)FG;
                    }
                    __syncthreads();
                }
            }
        }
        // output: from the labels, or -- when a bound was reached -- the raw mask (still unwritten, also in place)
        int c_pg = 0, c_p = 0, c_g = 0;
        for (int i = tid * 16; i < HW; i += THREADS * 16) {
            uint32_t o[4];
            if (ok) {
                const uint4 a = reinterpret_cast<const uint4*>(L + i)[0], b = reinterpret_cast<const uint4*>(L + i)[1];
                const uint32_t pair[8] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w};
#pragma unroll
                for (int k = 0; k < 4; ++k)
                    o[k] = ((pair[2 * k] & 0xFFFFu) == FG ? 0xFFu : 0u) | ((pair[2 * k] >> 16) == FG ? 0xFF00u : 0u) |
                           ((pair[2 * k + 1] & 0xFFFFu) == FG ? 0xFF0000u : 0u) | ((pair[2 * k + 1] >> 16) == FG ? 0xFF000000u : 0u);
            } else {
                const uint4 v = *reinterpret_cast<const uint4*>(m + i);
                const uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
                for (int k = 0; k < 4; ++k)
                    o[k] = ((w[k] & 0xFFu) ? 0xFFu : 0u) | ((w[k] & 0xFF00u) ? 0xFF00u : 0u) | ((w[k] & 0xFF0000u) ? 0xFF0000u : 0u) |
                           ((w[k] & 0xFF000000u) ? 0xFF000000u : 0u);
            }
            if (gt) {
                const uint4 g4 = *reinterpret_cast<const uint4*>(gt + img * HW + i);
                const uint32_t g[4] = {g4.x, g4.y, g4.z, g4.w};
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    const uint32_t gm = ((g[k] & 0xFFu) ? 0xFFu : 0u) | ((g[k] & 0xFF00u) ? 0xFF00u : 0u) |
                                        ((g[k] & 0xFF0000u) ? 0xFF0000u : 0u) | ((g[k] & 0xFF000000u) ? 0xFF000000u : 0u);
                    c_p += __popc(o[k]) >> 3;
                    c_g += __popc(gm) >> 3;
                    c_pg += __popc(o[k] & gm) >> 3;
                }
            }
            *reinterpret_cast<uint4*>(out + img * HW + i) = make_uint4(o[0], o[1], o[2], o[3]);
        }
        if (gt && (c_p | c_g)) { atomicAdd(&s_cnt[0], c_pg); atomicAdd(&s_cnt[1], c_p); atomicAdd(&s_cnt[2], c_g); }
        __syncthreads();
        if (gt && tid < 4) counts[img * 4 + tid] = tid < 3 ? s_cnt[tid] : s_cnt[1] + s_cnt[2] - s_cnt[0];
        if (stats && tid < 8) stats[img * 8 + tid] = ok ? (tid < 6 ? s_stat[tid] : 0) : (tid == 7 ? 1 : 0);
        __syncthreads();                                 // the next image resets the counters and the labels
    }
}

int check_shape(int64_t nimg, int H, int W, const char* who) {
    MUMPY_REQUIRE(nimg >= 0 && H >= 1 && W >= 1, MUMPY_EINVAL, "%s: bad sizes nimg=%lld, %dx%d", who, (long long)nimg, H, W);
    MUMPY_REQUIRE(nimg < LIM31 && (int64_t)H * W <= MAX_PIXELS, MUMPY_ERANGE,
                  "%s: nimg=%lld is 2^31 or more, or %dx%d is above %d pixels (the 16-bit labels of a frame must fit LDS)", who,
                  (long long)nimg, H, W, MAX_PIXELS);
    MUMPY_REQUIRE(H * W % 16 == 0, MUMPY_EINVAL, "%s: H*W=%d must be a multiple of 16", who, H * W);
    return 0;
}

}  // namespace

extern "C" int64_t mumpy_mask_clean_workspace_bytes(int64_t nimg, int H, int W) {
    const int rc = check_shape(nimg, H, W, "mask_clean_workspace_bytes");
    if (rc) return rc;
    return (nimg < GRID_MAX ? nimg : GRID_MAX) * (int64_t)H * W * 4;
}

extern "C" int mumpy_mask_clean_u8_fwd(const uint8_t* mask, uint8_t* out, const uint8_t* gt, int32_t* counts, int32_t* stats,
                                       const int32_t* params, void* workspace, int64_t workspace_bytes, int64_t nimg, int H, int W,
                                       void* stream) {
    MUMPY_REQUIRE(mask && out && params, MUMPY_ENULL, "mask_clean_u8: null mask, out or params");
    MUMPY_REQUIRE((gt == nullptr) == (counts == nullptr), MUMPY_ENULL, "mask_clean_u8: null gt or counts: they come together or not at all");
    const int rc = check_shape(nimg, H, W, "mask_clean_u8");
    if (rc) return rc;
    MUMPY_REQUIRE(aligned16(mask) && aligned16(out) && aligned16(gt) && aligned16(params) && aligned16(workspace), MUMPY_EALIGN,
                  "mask_clean_u8: mask, out, gt, params and workspace must be 16-byte aligned");
    const int64_t bytes = nimg * H * W;
    MUMPY_REQUIRE(bytes == 0 || mask == out || mask + bytes <= out || out + bytes <= mask, MUMPY_EINVAL,
                  "mask_clean_u8: out overlaps mask without being mask (in place means out == mask)");
    const int64_t need = mumpy_mask_clean_workspace_bytes(nimg, H, W);
    MUMPY_REQUIRE(need == 0 || workspace, MUMPY_ENULL, "mask_clean_u8: null workspace (%lld bytes needed)", (long long)need);
    MUMPY_REQUIRE(workspace_bytes >= need, MUMPY_EINVAL, "mask_clean_u8: workspace_bytes=%lld is too small, %lld needed",
                  (long long)workspace_bytes, (long long)need);
    if (nimg == 0) return 0;
    const size_t lds = (size_t)H * W * sizeof(uint16_t) + (size_t)((H * W + 31) / 32) * sizeof(uint32_t);     // labels + decision bits
    static bool attr_set = false;
    if (lds > 48 * 1024 && !attr_set) {                  // raise this kernel's dynamic-LDS cap once, to the largest image
        hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(mask_clean_kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                                           MAX_PIXELS * (int)sizeof(uint16_t) + MAX_PIXELS / 8);
        MUMPY_REQUIRE(e == hipSuccess, (int)e, "mask_clean_u8: cannot raise the dynamic LDS limit: %s", hipGetErrorString(e));
        attr_set = true;
    }
    const unsigned grid = (unsigned)(nimg < GRID_MAX ? nimg : GRID_MAX);
    hipLaunchKernelGGL(mask_clean_kernel, dim3(grid), dim3(THREADS), lds, as_stream(stream), mask, out, gt, counts, stats, params,
                       static_cast<uint32_t*>(workspace), nimg, H, W);
    MUMPY_CHECK_LAUNCH("mask_clean_u8");
    return 0;
}
