// cva_fused.hip — the two GEMMs of SwinDAttention (deform:324-405) whose neighbours are pure index work, with that work folded
// into the GEMM's operand loader / epilogue so that the intermediate tensors never exist in HBM (round 3):
//
//   mumpy_deform_sample_kv_fwd    kv = [proj_k | proj_v](grid_sample(x2, pos))                 (deform:353-362)
//       the bilinear sampling IS the A-operand loader: a staged A piece (row m = (kv window, point), 4 channels of a 32-deep
//       chunk) is the weighted sum of the four corner pieces of the window's 49 x C tile, which lives in L2 after its first
//       touch; the sampled map (nkv x 49 x C, 48 MB at stage 0 of config 2) is neither written nor read.  A row's corner
//       offsets and weights are recomputed only when the chunk enters the next offset group (C/3 channels share a position).
//       Tile 64 x 192: at stage 0 the whole [k|v] width (2C = 192) is one tile, so every point is sampled exactly once;
//       deeper stages sample a point once per 192-column tile (2-8 times) out of L2-resident 18-150 KB tiles.
//   mumpy_deform_out_combine_fwd  x1 + x1[window order] + reshape_(C,49)->(49,C)(proj_out(o))      (deform:402-403; mTVE:138,285-286)
//       computed TRANSPOSED -- A = W_out (rows = output channel c'), B = o (rows = (q window, point p')) -- so that a lane of
//       the accumulator owns one p' and the scrambled destination  window_base + c' * 49 + p'  (the reference re-reads the flat
//       (C,49) image as (49,C) without a permute) is consecutive across lanes: coalesced stores, and the two x1 terms of the
//       caller's residual wiring are read at the same (contiguous / row-segment) addresses.  Replaces the proj_out GEMM, its
//       (nq,49,C) output and mumpy_deform_combine_fwd.
//
// Both are 4-wave tiled kernels on v_mfma_f32_32x32x2_f32 (exact fp32 products, as every GEMM of the fp32 path), 32-deep
// chunks, two LDS buffers with 36-dword rows, global -> register -> LDS staging one chunk ahead.  They are mid-size launches
// (0.5-9 GFLOP); what they buy is two launches and two HBM round trips less on the cross-view dependency chain.
//
// MM16 = true (mumpy_deform_sample_kv_mm16_fwd / mumpy_deform_out_combine_mm16_fwd; opt-in, ops.set_cva_math("bf16")): the same
// tiling, loaders, group logic and epilogues with the two operands rounded to bf16 (nearest even) on their way to LDS and
// multiplied on v_mfma_f32_32x32x16_bf16 with fp32 accumulation.  Everything before the rounding (the bilinear sum, in the
// operation order of deform_sample_lds_kernel) and after the product (bias, residual terms) is the fp32 code of the fp32 form.
// Both LDS images stay [row][k]: a 32-deep chunk is 32 bf16 = 16 dwords per row, rows LDH = 20 dwords apart -- 5 16-byte slots,
// odd, so the 16 rows a ds_read_b128 lane group touches (distinct mod 16) fall on 16 distinct slots of the 64-bank row:
// conflict-free fragment reads (the image and the reads of the bf16 form of xgemm_kernel, gemm_bwd.hip).  Two MFMA steps per chunk instead of 16.
// Resources (hipcc -Rpass-analysis=kernel-resource-usage, gfx950; VGPRs / AGPRs / SGPRs / LDS per block / waves per SIMD; scratch 0):
//   deform_sample_kv_kernel<96 | 192 | 384 | 768, true>    132 | 134 | 130 | 130 / 0 / 44 | 44 | 47 | 47 / 40,960 B / 3
//     (the fp32 form: 154 | 184 | 172 | 172 / 0 / 44 | 44 | 47 | 47 / 73,728 B / 2)
//   deform_out_combine_kernel<96 | 192 | 384 | 768, true>  54 | 58 | 60 | 58 / 0 / 20 / 20,480 B / 8
//     (the fp32 form: 54 / 0 / 20 / 36,864 B / 4)
#include "cva_pairing.h"
#include "../../include/mumpy_hip_ext8.h"
using namespace mumpy;

namespace {

constexpr int BK = 32, LDR = 36;
constexpr int LDH = 20;   // MM16: dwords per LDS row (32 bf16 + 4 dwords of padding)

typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef __bf16 bf16x4 __attribute__((ext_vector_type(4)));

// MM16 staging: 4 fp32 -> 4 bf16 (round to nearest even), one 8-byte LDS store at dword `dw` of the image
__device__ __forceinline__ void put_bf16x4(float* img, int dw, f32x4 v) {
    *reinterpret_cast<uint2*>(img + dw) = __builtin_bit_cast(uint2, __builtin_convertvector(v, bf16x4));
}
// MM16 fragment of MFMA step st: lane (c, h) supplies k = 16 st + 8 h .. + 7 of its row (row_h = row start + 4 h dwords)
__device__ __forceinline__ bf16x8 frag_bf16(const float* row_h, int st) { return *reinterpret_cast<const bf16x8*>(row_h + 8 * st); }

// m / 49 and m % 49 for m < 2^31 / 49 (mulhi by ceil(2^37 / 49))
__device__ __forceinline__ void divmod49(unsigned m, unsigned& q, unsigned& r) {
    q = (unsigned)(((uint64_t)m * 2804876602ull) >> 37);
    r = m - 49u * q;
}

// ------------------------------------------------------------------------------------------------------------------
// GROUPED: the pairing rule of cva_pairing.h; <false> carries nq alone and is the kernel it was
template <int C, bool MM16, bool GROUPED>
__global__ __launch_bounds__(256, 2) void deform_sample_kv_kernel(const float* __restrict__ x2, const float* __restrict__ pos,
                                                                  const float* __restrict__ Wkv, const float* __restrict__ bkv,
                                                                  float* __restrict__ kv, int Hs2, int W, int nWx, int nW2,
                                                                  CvaPairing<GROUPED> pair, int M, unsigned gn) {
    constexpr int BM = 64, BN = 192, TN = 3, N = 2 * C, K = C, CG = C / 3, NK = K / BK, CPG = CG / BK;   // CPG: chunks per group
    constexpr int A_LD = BM / 32, B_LD = BN / 32;
    __shared__ __attribute__((aligned(16))) float lds[2][(BM + BN) * (MM16 ? LDH : LDR)];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int c = lane & 31, h = lane >> 5, wm = wave >> 1, wn = wave & 1;
    // XCD-major renumbering; the N tiles of one row panel are neighbours (they sample the same windows)
    const unsigned wgid = xcd_major_id(blockIdx.x, gridDim.x);
    const unsigned tm = wgid / gn, tn = wgid - tm * gn;
    const int m0 = (int)tm * BM, n0 = (int)tn * BN;
    const int ld_row = tid >> 3, ld_c4 = tid & 7;

    // per staged A row: the window's first token, the point, and (per offset group) four corner offsets + weights
    const float* abase[A_LD];
    const float* apos[A_LD];
    int aoff[A_LD][4];
    float aw[A_LD][4];
#pragma unroll
    for (int i = 0; i < A_LD; ++i) {
        int m = m0 + ld_row + 32 * i;
        if (m > M - 1) m = M - 1;                       // rows past the edge: clamped, never stored
        unsigned b2, p;
        divmod49((unsigned)m, b2, p);
        const unsigned b = b2 / (unsigned)nW2, n = b2 - b * (unsigned)nW2;
        const unsigned wy = n / (unsigned)nWx, wx = n - wy * (unsigned)nWx;
        abase[i] = x2 + (((int64_t)b * Hs2 + wy * WS) * W + wx * WS) * C + 4 * ld_c4;
        apos[i] = pos + ((int64_t)cva_q_window(b2, pair) * 3 * WT + p) * 2;
    }
    auto set_group = [&](int g) {
#pragma unroll
        for (int i = 0; i < A_LD; ++i) {
            const float gy = apos[i][g * WT * 2], gx = apos[i][g * WT * 2 + 1];
            const float iy = ((gy + 1.0f) * 0.5f) * 6.0f;       // grid_sample, align_corners=True: pixel = (g + 1) / 2 * (size - 1)
            const float ix = ((gx + 1.0f) * 0.5f) * 6.0f;
            const float y0f = floorf(iy), x0f = floorf(ix);
            const int y0 = (int)y0f, x0 = (int)x0f;
            const float wgt[4] = {(x0f + 1.0f - ix) * (y0f + 1.0f - iy), (ix - x0f) * (y0f + 1.0f - iy),
                                  (x0f + 1.0f - ix) * (iy - y0f), (ix - x0f) * (iy - y0f)};
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const int yy = y0 + (e >> 1), xx = x0 + (e & 1);
                const bool ok = (unsigned)yy < (unsigned)WS && (unsigned)xx < (unsigned)WS;      // zeros padding
                aw[i][e] = ok ? wgt[e] : 0.f;
                aoff[i][e] = ok ? (yy * W + xx) * C : 0;
            }
        }
    };
    const float* brow[B_LD];
#pragma unroll
    for (int i = 0; i < B_LD; ++i) {
        int n = n0 + ld_row + 32 * i;
        if (n > N - 1) n = N - 1;
        brow[i] = Wkv + (int64_t)n * K + 4 * ld_c4;
    }
    f32x4 areg[A_LD], breg[B_LD];
    auto gload = [&](int kc) {
        const int k0 = kc * BK;
#pragma unroll
        for (int i = 0; i < A_LD; ++i) {
            const float* s = abase[i] + k0;
            // the order of operations of deform_sample_lds_kernel (nw, ne, sw, se): the sampled values are bitwise the same
            f32x4 r = *reinterpret_cast<const f32x4*>(s + aoff[i][0]) * aw[i][0];
            r += *reinterpret_cast<const f32x4*>(s + aoff[i][1]) * aw[i][1];
            r += *reinterpret_cast<const f32x4*>(s + aoff[i][2]) * aw[i][2];
            r += *reinterpret_cast<const f32x4*>(s + aoff[i][3]) * aw[i][3];
            areg[i] = r;
        }
#pragma unroll
        for (int i = 0; i < B_LD; ++i) breg[i] = *reinterpret_cast<const f32x4*>(brow[i] + k0);
    };
    auto lstore = [&](int buf) {
        if constexpr (MM16) {                           // only the finished sample (and the W piece) is rounded
#pragma unroll
            for (int i = 0; i < A_LD; ++i) put_bf16x4(lds[buf], (ld_row + 32 * i) * LDH + 2 * ld_c4, areg[i]);
#pragma unroll
            for (int i = 0; i < B_LD; ++i) put_bf16x4(lds[buf], (BM + ld_row + 32 * i) * LDH + 2 * ld_c4, breg[i]);
        } else {
#pragma unroll
            for (int i = 0; i < A_LD; ++i) *reinterpret_cast<f32x4*>(&lds[buf][(ld_row + 32 * i) * LDR + 4 * ld_c4]) = areg[i];
#pragma unroll
            for (int i = 0; i < B_LD; ++i) *reinterpret_cast<f32x4*>(&lds[buf][(BM + ld_row + 32 * i) * LDR + 4 * ld_c4]) = breg[i];
        }
    };
    f32x16 acc[TN];
#pragma unroll
    for (int j = 0; j < TN; ++j)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[j][r] = 0.f;
    auto compute = [&](int buf) {
        if constexpr (MM16) {
            const float* a_f = &lds[buf][(wm * 32 + c) * LDH + 4 * h];
            const float* b_f = &lds[buf][(BM + wn * 96 + c) * LDH + 4 * h];
#pragma unroll
            for (int st = 0; st < 2; ++st) {
                const bf16x8 fa = frag_bf16(a_f, st);
                bf16x8 fb[TN];
#pragma unroll
                for (int j = 0; j < TN; ++j) fb[j] = frag_bf16(b_f + 32 * j * LDH, st);
#pragma unroll
                for (int j = 0; j < TN; ++j) acc[j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fa, fb[j], acc[j], 0, 0, 0);
            }
        } else {
            const float* a_f = &lds[buf][(wm * 32 + c) * LDR + 16 * h];
            const float* b_f = &lds[buf][(BM + wn * 96 + c) * LDR + 16 * h];
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const f32x4 fa = *reinterpret_cast<const f32x4*>(a_f + 4 * q);
                f32x4 fb[TN];
#pragma unroll
                for (int j = 0; j < TN; ++j) fb[j] = *reinterpret_cast<const f32x4*>(b_f + 32 * j * LDR + 4 * q);
#pragma unroll
                for (int e = 0; e < 4; ++e)
#pragma unroll
                    for (int j = 0; j < TN; ++j) acc[j] = __builtin_amdgcn_mfma_f32_32x32x2f32(fa[e], fb[j][e], acc[j], 0, 0, 0);
            }
        }
    };
    set_group(0);
    gload(0);
    lstore(0);
    __syncthreads();
    for (int kc = 0; kc < NK; ++kc) {
        if (kc + 1 < NK) {
            if ((kc + 1) % CPG == 0) set_group((kc + 1) / CPG);
            gload(kc + 1);
        }
        compute(kc & 1);
        if (kc + 1 < NK) lstore((kc + 1) & 1);          // the other buffer: its readers finished before the last barrier
        __syncthreads();
    }
    // D[row][col]: col = lane & 31, row = (r & 3) + 8 (r >> 2) + 4 h
#pragma unroll
    for (int j = 0; j < TN; ++j) {
        const int n = n0 + wn * 96 + 32 * j + c;
        if (n >= N) continue;
        const float bv = bkv[n];
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int m = m0 + wm * 32 + (r & 3) + 8 * (r >> 2) + 4 * h;
            if (m < M) kv[(int64_t)m * N + n] = acc[j][r] + bv;
        }
    }
}

// ------------------------------------------------------------------------------------------------------------------
// out[win_base + f] = x1[win_base + f] + x1[(img + tok(f / C)) C + f % C] + Yt[p'][c'],  f = c' 49 + p'
template <int C, bool MM16>
__global__ __launch_bounds__(256, 2) void deform_out_combine_kernel(const float* __restrict__ o, const float* __restrict__ Wout,
                                                                   const float* __restrict__ bout, const float* __restrict__ x1,
                                                                   float* __restrict__ out, int H, int W, int nWx, int nWf, int MO,
                                                                   unsigned gn) {
    constexpr int BM = 64, BN = 64, K = C, NK = K / BK;          // BM: output channels c' (rows of W_out); BN: rows of o
    constexpr int A_LD = BM / 32, B_LD = BN / 32;
    __shared__ __attribute__((aligned(16))) float lds[2][(BM + BN) * (MM16 ? LDH : LDR)];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int c = lane & 31, h = lane >> 5, wm = wave >> 1, wn = wave & 1;
    const unsigned wgid = xcd_major_id(blockIdx.x, gridDim.x);
    const unsigned tn = wgid / gn, tm = wgid - tn * gn;           // the channel tiles of one o row panel are neighbours
    const int c0 = (int)tm * BM, m0 = (int)tn * BN;
    const int ld_row = tid >> 3, ld_c4 = tid & 7;
    const float* arow[A_LD];
    const float* brow[B_LD];
#pragma unroll
    for (int i = 0; i < A_LD; ++i) {
        int cc = c0 + ld_row + 32 * i;
        if (cc > C - 1) cc = C - 1;
        arow[i] = Wout + (int64_t)cc * K + 4 * ld_c4;
    }
#pragma unroll
    for (int i = 0; i < B_LD; ++i) {
        int m = m0 + ld_row + 32 * i;
        if (m > MO - 1) m = MO - 1;
        brow[i] = o + (int64_t)m * K + 4 * ld_c4;
    }
    f32x4 areg[A_LD], breg[B_LD];
    auto gload = [&](int kc) {
#pragma unroll
        for (int i = 0; i < A_LD; ++i) areg[i] = *reinterpret_cast<const f32x4*>(arow[i] + kc * BK);
#pragma unroll
        for (int i = 0; i < B_LD; ++i) breg[i] = *reinterpret_cast<const f32x4*>(brow[i] + kc * BK);
    };
    auto lstore = [&](int buf) {
        if constexpr (MM16) {                           // W_out and o are rounded while staged
#pragma unroll
            for (int i = 0; i < A_LD; ++i) put_bf16x4(lds[buf], (ld_row + 32 * i) * LDH + 2 * ld_c4, areg[i]);
#pragma unroll
            for (int i = 0; i < B_LD; ++i) put_bf16x4(lds[buf], (BM + ld_row + 32 * i) * LDH + 2 * ld_c4, breg[i]);
        } else {
#pragma unroll
            for (int i = 0; i < A_LD; ++i) *reinterpret_cast<f32x4*>(&lds[buf][(ld_row + 32 * i) * LDR + 4 * ld_c4]) = areg[i];
#pragma unroll
            for (int i = 0; i < B_LD; ++i) *reinterpret_cast<f32x4*>(&lds[buf][(BM + ld_row + 32 * i) * LDR + 4 * ld_c4]) = breg[i];
        }
    };
    f32x16 acc;
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[r] = 0.f;
    auto compute = [&](int buf) {
        if constexpr (MM16) {
            const float* a_f = &lds[buf][(wm * 32 + c) * LDH + 4 * h];
            const float* b_f = &lds[buf][(BM + wn * 32 + c) * LDH + 4 * h];
#pragma unroll
            for (int st = 0; st < 2; ++st)
                acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(frag_bf16(a_f, st), frag_bf16(b_f, st), acc, 0, 0, 0);
        } else {
            const float* a_f = &lds[buf][(wm * 32 + c) * LDR + 16 * h];
            const float* b_f = &lds[buf][(BM + wn * 32 + c) * LDR + 16 * h];
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const f32x4 fa = *reinterpret_cast<const f32x4*>(a_f + 4 * q), fb = *reinterpret_cast<const f32x4*>(b_f + 4 * q);
#pragma unroll
                for (int e = 0; e < 4; ++e) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(fa[e], fb[e], acc, 0, 0, 0);
            }
        }
    };
    gload(0);
    lstore(0);
    __syncthreads();
    for (int kc = 0; kc < NK; ++kc) {
        if (kc + 1 < NK) gload(kc + 1);
        compute(kc & 1);
        if (kc + 1 < NK) lstore((kc + 1) & 1);
        __syncthreads();
    }
    // this lane's column = row m of o = (q window bw, point p'); accumulator rows = output channels c'
    const int m = m0 + wn * 32 + c;
    if (m >= MO) return;
    unsigned bw, pp;
    divmod49((unsigned)m, bw, pp);
    const unsigned b = bw / (unsigned)nWf, n = bw - b * (unsigned)nWf;
    const int wy = (int)(n / (unsigned)nWx), wx = (int)(n - (n / (unsigned)nWx) * (unsigned)nWx);
    const int64_t img = (int64_t)b * H * W;
    const int64_t win_base = (img + (int64_t)n * WT) * C;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const int cc = c0 + wm * 32 + (r & 3) + 8 * (r >> 2) + 4 * h;
        if (cc >= C) continue;
        const int f = cc * WT + (int)pp;
        const int po = f / C, co = f - po * C;                   // destination token-in-window and channel (C is a constant)
        const int tok = window_token(wy, wx, po, H, W, 0);
        out[win_base + f] = x1[win_base + f] + x1[(img + tok) * C + co] + (acc[r] + bout[cc]);
    }
}

}  // namespace

// one validation + launch body per kernel; `who` names the entry in mumpy_last_error.  groups: 1 from the frozen entries (the
// <GROUPED = false> kernels, no refusal added), any value from the grouped ones (include/mumpy_hip_ext8.h)
template <bool MM16>
static int sample_kv_launch(const char* who, const float* x2, const float* pos, const float* Wkv, const float* bkv, float* kv, int B,
                            int Hs2, int W, int C, int nq, int groups, void* stream) {
    MUMPY_REQUIRE(x2 && pos && Wkv && bkv && kv, MUMPY_ENULL, "%s: null pointer", who);
    MUMPY_REQUIRE(aligned16(x2) && aligned16(Wkv) && aligned16(kv), MUMPY_EALIGN, "%s: pointers must be 16-byte aligned", who);
    MUMPY_REQUIRE(B > 0 && Hs2 > 0 && W > 0 && Hs2 % WS == 0 && W % WS == 0 && nq > 0, MUMPY_EINVAL,
                  "%s: bad grid (%d,%d) / nq=%d", who, Hs2, W, nq);
    MUMPY_REQUIRE(C == 96 || C == 192 || C == 384 || C == 768, MUMPY_EINVAL,
                  "%s: C=%d is not one of the encoder widths 96/192/384/768", who, C);
    const int nWx = W / WS, nW2 = (Hs2 / WS) * nWx;
    const int64_t nwin = (int64_t)B * nW2, M = nwin * WT;
    MUMPY_REQUIRE(M < (1ll << 31) - 64, MUMPY_ERANGE, "%s: too many windows", who);
    const unsigned gn = (unsigned)((2 * C + 191) / 192);
    const int64_t grid = ((M + 63) / 64) * gn;
    MUMPY_REQUIRE(grid < (1ll << 31), MUMPY_ERANGE, "%s: too many tiles", who);
    CvaPairing<true> pg;
    const int bad = cva_grouping(who, nwin, nq, B, groups, &pg);
    if (bad) return bad;
    const CvaPairing<false> p1 = {nq};
#define MUMPY_SKV_AS(C_, G_, P_)                                                                                             \
    hipLaunchKernelGGL((deform_sample_kv_kernel<C_, MM16, G_>), dim3((unsigned)grid), dim3(256), 0, as_stream(stream), x2, pos, Wkv, \
                       bkv, kv, Hs2, W, nWx, nW2, P_, (int)M, gn)
#define MUMPY_SKV(C_)                                                                                                        \
    if (groups > 1) MUMPY_SKV_AS(C_, true, pg); else MUMPY_SKV_AS(C_, false, p1)
    switch (C) {
        case 96: MUMPY_SKV(96); break;
        case 192: MUMPY_SKV(192); break;
        case 384: MUMPY_SKV(384); break;
        default: MUMPY_SKV(768); break;
    }
#undef MUMPY_SKV
#undef MUMPY_SKV_AS
    MUMPY_CHECK_LAUNCH(who);
    return 0;
}

template <bool MM16>
static int out_combine_launch(const char* who, const float* o, const float* Wout, const float* bout, const float* x1, float* out,
                              int B, int H, int W, int C, void* stream) {
    MUMPY_REQUIRE(o && Wout && bout && x1 && out, MUMPY_ENULL, "%s: null pointer", who);
    MUMPY_REQUIRE(x1 != out, MUMPY_EINVAL, "%s: out must not alias x1", who);
    MUMPY_REQUIRE(aligned16(o) && aligned16(Wout), MUMPY_EALIGN, "%s: pointers must be 16-byte aligned", who);
    MUMPY_REQUIRE(B > 0 && H > 0 && W > 0 && H % WS == 0 && W % WS == 0, MUMPY_EINVAL, "%s: bad grid (%d,%d)", who, H, W);
    MUMPY_REQUIRE(C == 96 || C == 192 || C == 384 || C == 768, MUMPY_EINVAL,
                  "%s: C=%d is not one of the encoder widths 96/192/384/768", who, C);
    const int nWx = W / WS, nWf = (H / WS) * nWx;
    const int64_t MO = (int64_t)B * nWf * WT;
    MUMPY_REQUIRE(MO * 49 < (1ll << 31) && MO < (1ll << 31) - 64, MUMPY_ERANGE, "%s: too many windows", who);
    const unsigned gn = (unsigned)((C + 63) / 64);
    const int64_t grid = ((MO + 63) / 64) * gn;
#define MUMPY_OC(C_)                                                                                                         \
    hipLaunchKernelGGL((deform_out_combine_kernel<C_, MM16>), dim3((unsigned)grid), dim3(256), 0, as_stream(stream), o, Wout, bout, \
                       x1, out, H, W, nWx, nWf, (int)MO, gn)
    switch (C) {
        case 96: MUMPY_OC(96); break;
        case 192: MUMPY_OC(192); break;
        case 384: MUMPY_OC(384); break;
        default: MUMPY_OC(768); break;
    }
#undef MUMPY_OC
    MUMPY_CHECK_LAUNCH(who);
    return 0;
}

extern "C" int mumpy_deform_sample_kv_fwd(const float* x2, const float* pos, const float* Wkv, const float* bkv, float* kv, int B,
                                          int Hs2, int W, int C, int nq, void* stream) {
    return sample_kv_launch<false>("deform_sample_kv", x2, pos, Wkv, bkv, kv, B, Hs2, W, C, nq, 1, stream);
}

extern "C" int mumpy_deform_sample_kv_grouped_fwd(const float* x2, const float* pos, const float* Wkv, const float* bkv, float* kv,
                                                  int B, int Hs2, int W, int C, int nq, int groups, void* stream) {
    return sample_kv_launch<false>("deform_sample_kv_grouped", x2, pos, Wkv, bkv, kv, B, Hs2, W, C, nq, groups, stream);
}

extern "C" int mumpy_deform_sample_kv_mm16_grouped_fwd(const float* x2, const float* pos, const float* Wkv, const float* bkv,
                                                       float* kv, int B, int Hs2, int W, int C, int nq, int groups, void* stream) {
    return sample_kv_launch<true>("deform_sample_kv_mm16_grouped", x2, pos, Wkv, bkv, kv, B, Hs2, W, C, nq, groups, stream);
}

extern "C" int mumpy_deform_sample_kv_mm16_fwd(const float* x2, const float* pos, const float* Wkv, const float* bkv, float* kv,
                                               int B, int Hs2, int W, int C, int nq, void* stream) {
    return sample_kv_launch<true>("deform_sample_kv_mm16", x2, pos, Wkv, bkv, kv, B, Hs2, W, C, nq, 1, stream);
}

extern "C" int mumpy_deform_out_combine_fwd(const float* o, const float* Wout, const float* bout, const float* x1, float* out, int B,
                                            int H, int W, int C, void* stream) {
    return out_combine_launch<false>("deform_out_combine", o, Wout, bout, x1, out, B, H, W, C, stream);
}

extern "C" int mumpy_deform_out_combine_mm16_fwd(const float* o, const float* Wout, const float* bout, const float* x1, float* out,
                                                 int B, int H, int W, int C, void* stream) {
    return out_combine_launch<true>("deform_out_combine_mm16", o, Wout, bout, x1, out, B, H, W, C, stream);
}
