// window_attention_bwd.hip — backward of the Swin window attention core ("backward HIP kernels for row 5"): the fp32 pair
// win_attn_bwd_{q,kv}_kernel, the bf16-MFMA pair win_attn_bwd_{q,kv}_bf16mm_kernel, the dBias reduce and the two bias-table
// kernels they share, the workspace sizing and the entry points.  The unit (data flow, walk, helpers) is in win_attn_unit.h, the
// forward in window_attention.hip.
//
// Given dO, the unit's P = softmax(q k^T + bias + mask) is recomputed (nothing but q/k/v is kept from the forward) and
//   dV = P^T dO,   dP = dO V^T,   dS = P o (dP - rowsum(P o dP)),   dQ = scale dS K,   dK = dS^T (scale Q),   dBias += dS.
// Two kernels, one per MFMA orientation, so that every product gets its A operand straight from accumulator registers
// (the forward's accumulator->operand trick) and nothing is transposed through LDS:
//   bwd_q : lane = QUERY (S^T = K Q^T as in the forward): softmax statistics, D = rowsum(P o dP), dS^T, dQ = dS K, and the
//           per-wave running sum of dS for the bias gradient; writes {m, 1/l, D} per query for the second kernel.
//   bwd_kv: lane = KEY (S = Q K^T, the same fragments with the MFMA operands swapped): P and dS rebuilt from the saved
//           statistics, dV = P^T dO and dK = dS^T Q accumulated over the queries.
// One wave per (window, head) unit, persistent blocks of 4 waves per head as in the forward; 1 wave per SIMD (the
// operand sets of a unit need ~300 VGPRs).  Deterministic: per-wave dBias partials are reduced in a fixed order.
// Resources (hipcc -Rpass-analysis=kernel-resource-usage, gfx950): q kernel 256 VGPRs + 59 AGPRs, 87 SGPRs; kv kernel 256 + 110, 81 SGPRs;
// both no scratch, 15,376 B of LDS per block.
#include <stdlib.h>
#include "win_attn_unit.h"

namespace {

__global__ __launch_bounds__(256, 1) void win_attn_bwd_q_kernel(BwdArgs a) {
    __shared__ uint32_t tok_in[4][64];
    __shared__ uint32_t tok_out[4][64];
    __shared__ __attribute__((aligned(16))) float bias_s[WT * BLD];
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int c = lane & 31, h = lane >> 5;
    const int head = blockIdx.x % a.nH;
    const int slot = blockIdx.x / a.nH;
    const int64_t nwin = (int64_t)a.B * a.nW;
    stage_bias(bias_s, a.bias, head);
    const int64_t L = (int64_t)a.Hs * a.W;
    const uint32_t rsb = 12u * a.C, rob = 4u * a.C;
    uint32_t* ti = tok_in[wave];
    uint32_t* to = tok_out[wave];
    f32x16 dsum[2][2] = {};                                               // running sum of dS^T over this wave's units

    for (int64_t bw = (int64_t)slot * 4 + wave; bw < nwin; bw += (int64_t)a.groups * 4) {
        const int64_t b = unit_tokens(a, bw, lane, rsb, rob, ti, to);
        const char* qb = reinterpret_cast<const char*>(a.qkv + b * L * 3 * a.C + head * HD);
        const char* kb = qb + 4 * a.C;
        const char* vb = qb + 8 * a.C;
        const char* dob = reinterpret_cast<const char*>(a.dout + b * L * a.C + head * HD);
        f32x4 qf[2][4], kf[2][4], vkf[2][4], dof[2][4];
        float kv[2][16];
#pragma unroll
        for (int t = 0; t < 2; ++t) {
            const uint32_t off = ti[32 * t + c] + 64u * h;
            load_frag16(qf[t], qb, off);
            load_frag16(kf[t], kb, off);
            load_frag16(vkf[t], vb, off);
            load_frag16(dof[t], dob, to[32 * t + c] + 64u * h);
        }
        for_pv_steps([&](int jt, int g, int e) {
            kv[jt][4 * g + e] = *reinterpret_cast<const float*>(kb + (ti[32 * jt + 8 * g + 4 * h + e] + 4u * c));
        });
#pragma unroll
        for (int t = 0; t < 2; ++t)
#pragma unroll
            for (int i = 0; i < 4; ++i) qf[t][i] *= a.scale;
        const float* mask_w = unit_mask(a, bw);
        char* dqb = reinterpret_cast<char*>(a.dqkv + b * L * 3 * a.C + head * HD);
        float* st = a.stats + (bw * a.nH + head) * 192;                   // {m[64], inv[64], D[64]} of this unit
#pragma unroll
        for (int it = 0; it < 2; ++it) {
            f32x16 s[2] = {}, dp[2] = {};
            qk_product(s, kf, qf[it]);                                    // S^T = K Q^T
            const int qi = 32 * it + c;
            const auto bias_at = bias_row(bias_s, BLD, qi, h);
            float m, inv;
            if (mask_w) bias_softmax<true>(s, bias_at, mask_w, qi, h, 1.0f, &m, &inv);
            else bias_softmax<false>(s, bias_at, nullptr, qi, h, 1.0f, &m, &inv);
            qk_product(dp, vkf, dof[it]);                                 // dP^T = V dO^T
            float d = 0.f;
#pragma unroll
            for (int jt = 0; jt < 2; ++jt)
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    if (jt == 1 && r >= 9) continue;                      // P == 0 on padded keys
                    d += s[jt][r] * dp[jt][r];
                }
            d += __shfl_xor(d, 32);
            const bool qvalid = qi < WT;
#pragma unroll
            for (int jt = 0; jt < 2; ++jt)
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    if (jt == 1 && r >= 9) { s[jt][r] = 0.f; continue; }
                    const float ds = qvalid ? s[jt][r] * (dp[jt][r] - d) : 0.f;    // padded queries contribute nothing
                    s[jt][r] = ds;
                    dsum[it][jt][r] += ds;
                }
            if (h == 0 && qvalid) { st[qi] = m; st[64 + qi] = inv; st[128 + qi] = d; }
            f32x16 o = {};
            pv_product(o, s, kv);                                         // dQ = dS K   (rows = queries, lanes = channels)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                if (!acc_live(it, r)) continue;
                const int i = acc_row(it, r, h);
                if (i < WT) *reinterpret_cast<float*>(dqb + (ti[i] + 4u * c)) = o[r] * a.scale;
            }
        }
        __builtin_amdgcn_wave_barrier();
    }
    float* part = a.dbias_part + ((int64_t)blockIdx.x * 4 + wave) * 4096;  // [it][jt][r][lane]
#pragma unroll
    for (int it = 0; it < 2; ++it)
#pragma unroll
        for (int jt = 0; jt < 2; ++jt)
#pragma unroll
            for (int r = 0; r < 16; ++r) part[((it * 2 + jt) * 16 + r) * 64 + lane] = dsum[it][jt][r];
}

__global__ __launch_bounds__(256, 1) void win_attn_bwd_kv_kernel(BwdArgs a) {
    __shared__ uint32_t tok_in[4][64];
    __shared__ uint32_t tok_out[4][64];
    __shared__ __attribute__((aligned(16))) float biasT_s[WT * BLD];      // bias^T: row = key j, column = query i
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int c = lane & 31, h = lane >> 5;
    const int head = blockIdx.x % a.nH;
    const int slot = blockIdx.x / a.nH;
    const int64_t nwin = (int64_t)a.B * a.nW;
    stage_bias_T(biasT_s, a.bias, head);
    const int64_t L = (int64_t)a.Hs * a.W;
    const uint32_t rsb = 12u * a.C, rob = 4u * a.C;
    uint32_t* ti = tok_in[wave];
    uint32_t* to = tok_out[wave];
    for (int64_t bw = (int64_t)slot * 4 + wave; bw < nwin; bw += (int64_t)a.groups * 4) {
        const int64_t b = unit_tokens(a, bw, lane, rsb, rob, ti, to);
        const char* qb = reinterpret_cast<const char*>(a.qkv + b * L * 3 * a.C + head * HD);
        const char* kb = qb + 4 * a.C;
        const char* vb = qb + 8 * a.C;
        const char* dob = reinterpret_cast<const char*>(a.dout + b * L * a.C + head * HD);
        f32x4 qf[2][4], kf[2][4], vkf[2][4], dof[2][4];
        float qv[2][16], dov[2][16];                                      // query-order operands: [it][4g+e] = row 32it+8g+4h+e, lane = channel
#pragma unroll
        for (int t = 0; t < 2; ++t) {
            const uint32_t off = ti[32 * t + c] + 64u * h;
            load_frag16(qf[t], qb, off);
            load_frag16(kf[t], kb, off);
            load_frag16(vkf[t], vb, off);
            load_frag16(dof[t], dob, to[32 * t + c] + 64u * h);
        }
        for_pv_steps([&](int it, int g, int e) {
            const int i = 32 * it + 8 * g + 4 * h + e;
            qv[it][4 * g + e] = *reinterpret_cast<const float*>(qb + (ti[i] + 4u * c)) * a.scale;
            dov[it][4 * g + e] = *reinterpret_cast<const float*>(dob + (to[i] + 4u * c));
        });
#pragma unroll
        for (int t = 0; t < 2; ++t)
#pragma unroll
            for (int i = 0; i < 4; ++i) qf[t][i] *= a.scale;
        const float* mask_w = unit_mask(a, bw);
        char* dkb = reinterpret_cast<char*>(a.dqkv + b * L * 3 * a.C + head * HD) + 4 * a.C;
        char* dvb = dkb + 4 * a.C;
        const float* st = a.stats + (bw * a.nH + head) * 192;
#pragma unroll
        for (int jt = 0; jt < 2; ++jt) {
            f32x16 s[2] = {}, dp[2] = {};                                 // [query tile it]: lane = key 32jt+c, rows = queries
            qk_product(s, qf, kf[jt]);                                    // S = Q K^T   (A = q rows, B = k rows)
            qk_product(dp, dof, vkf[jt]);                                 // dP = dO V^T
            const int kj = 32 * jt + c;
            const int kjc = kj < WT ? kj : WT - 1;
            const float* brow = &biasT_s[kjc * BLD + 4 * h];
#pragma unroll
            for (int it = 0; it < 2; ++it)
#pragma unroll
                for (int g = 0; g < 4; ++g) {
                    if (it == 1 && g == 3) {                              // queries 56..63: padding
#pragma unroll
                        for (int e = 0; e < 4; ++e) { s[it][4 * g + e] = 0.f; dp[it][4 * g + e] = 0.f; }
                        continue;
                    }
                    const int i0 = 32 * it + 8 * g + 4 * h;               // this lane's 4 consecutive queries i0 .. i0+3
                    f32x4 bv = *reinterpret_cast<const f32x4*>(brow + 32 * it + 8 * g);
                    if (mask_w) bv += *reinterpret_cast<const f32x4*>(mask_w + kjc * 64 + i0);   // mask is symmetric in (i, j)
                    const f32x4 mv = *reinterpret_cast<const f32x4*>(st + i0);
                    const f32x4 iv = *reinterpret_cast<const f32x4*>(st + 64 + i0);
                    const f32x4 dv = *reinterpret_cast<const f32x4*>(st + 128 + i0);
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        const bool valid = (i0 + e < WT) && (kj < WT);
                        const float pr = valid ? __expf(s[it][4 * g + e] + bv[e] - mv[e]) * iv[e] : 0.f;
                        s[it][4 * g + e] = pr;                                             // P
                        dp[it][4 * g + e] = valid ? pr * (dp[it][4 * g + e] - dv[e]) : 0.f;   // dS
                    }
                }
            f32x16 ov = {}, ok = {};
            pv_product(ov, s, dov);                                       // dV = P^T dO   (sum over queries)
            pv_product(ok, dp, qv);                                       // dK = dS^T (scale Q)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                if (!acc_live(jt, r)) continue;
                const int j = acc_row(jt, r, h);
                if (j < WT) {
                    *reinterpret_cast<float*>(dvb + (ti[j] + 4u * c)) = ov[r];
                    *reinterpret_cast<float*>(dkb + (ti[j] + 4u * c)) = ok[r];
                }
            }
        }
        __builtin_amdgcn_wave_barrier();
    }
}

// ---------------------------------------------------------------------------------------------------------------
// bf16-MFMA form of the backward pair for the fp32-stored training tape (mumpy_window_attention_mm16_bwd; opt-in, see
// ops.set_attention_math): every product on v_mfma_f32_32x32x16_bf16 with fp32 accumulation, operands rounded to bf16 in registers
// (round to nearest even), softmax, D, dS and the bias gradient in fp32.  Arithmetic, r(x) = bf16 rounding:
//   S = scale (r(q) r(k)^T) + bias (+ mask)      (scale on the fp32 product as in the bf16-MFMA forward: q is rounded once, unscaled)
//   P = softmax(S),  dP = r(dO) r(v)^T,  D = rowsum(P o dP),  dS = P o (dP - D)                                   [all fp32]
//   dV = r(P)^T r(dO),  dQ = scale r(dS) r(k),  dK = scale r(dS)^T r(q),  dBias += dS (the fp32 dS, before it is rounded)
// Same two-orientation scheme, unit walk, statistics record {m, 1/l, D} and dBias partial layout as the fp32 pair above, so the
// reduce and table kernels are shared.  What differs: an operand fragment is 4 registers instead of 16 (2 k-steps of 8 bf16), P / dS go
// from the accumulator to the A operand by a pairwise cast (k order permuted as in the bf16-MFMA forward; the B operand is gathered in
// that order by load_perm_bf16), 8 + 8 + 8 MFMAs per unit and kernel instead of 64 + 64 + 50.  P and dS are exactly 0 on padded
// keys / queries BEFORE they are rounded, so whatever finite value a clamped slot holds in the B operand is multiplied by 0.
// Resources (hipcc -Rpass-analysis=kernel-resource-usage, gfx950): q kernel 248 VGPRs, kv kernel 240, 0 AGPRs, no scratch, 15.4 / 18.4 KB of
// LDS per block: 2 waves per SIMD (the fp32 pair: 256 + 59 / 256 + 110 registers, 1 wave per SIMD).  What that took: one branch per unit on the
// mask pointer (a branch inside the tile code lets LLVM sink the operand conversions past it, and every raw fp32 row is then live at once),
// operand rows loaded in batches that are rounded before the next batch is issued (sched_barrier), dP^T one key tile at a time and twice
// in the q kernel, one query tile at a time straight into dV / dK in the kv kernel, the unit's statistics through LDS.
// Measured against the fp32 kernels on the same input (tools/kernel_micro.py winattn_bwd16 / winattn_mm16; profiles/bf16mm_window_attention_train.md):
//   (B, Hs, W, C)      backward, all 4 launches: fp32 -> bf16 MFMA        forward: fp32 -> bf16 MFMA (fp32 I/O)   [us, MI355X, medians of 12 x 20
//                        shift 0                 shift 3                    shift 0            shift 3             alternating launches; the shapes of
//   (2, 280, 56, 128)   100.3 -> 70.2 (1.43x)   104.3 -> 73.3 (1.42x)      23.0 -> 15.2       24.2 -> 17.1        the B=2, T=5 training step]
//   (2, 140, 28, 256)    72.5 -> 48.3 (1.50x)    74.7 -> 50.4 (1.48x)      15.4 -> 10.4       16.6 -> 11.4
//   (2,  70, 14, 512)    44.2 -> 33.5 (1.32x)    46.2 -> 35.1 (1.31x)      10.3 -> 10.2       11.0 -> 10.5
//   (2,  35,  7, 1024)   40.7 -> 30.0 (1.36x)     --                       10.4 -> 10.3        --
//   (2,  56, 56,  96)    41.5 -> 31.3 (1.33x)    43.8 -> 32.6 (1.34x)      10.3 -> 10.0       10.9 -> 10.6
//   (2,  28, 28, 192)    38.2 -> 28.0 (1.36x)    40.2 -> 29.2 (1.38x)      10.4 -> 10.3       10.8 -> 10.4
//   (2,  14, 14, 384)    35.6 -> 26.1 (1.36x)    38.2 -> 28.0 (1.36x)      10.4 -> 10.3       11.2 -> 10.9
//   (2,   7,  7, 768)    33.6 -> 26.4 (1.27x)     --                       10.3 -> 10.4        --
// The backward figure is the whole entry (q, kv, dBias reduce, table kernel; four launches, so ~26 us is the eager launch rate: the six
// small shapes are paced by it with either pair, as the forward's ~10 us).  In the graphed B=2 bf16 step (rocprofv3 --kernel-trace, 60
// launches per step): q kernel 20.2 -> 15.7 us, kv kernel 19.8 -> 12.9, forward 11.8 -> 8.7; the step 34.0 -> 33.1 ms.  Persistent blocks
// (MUMPY_WA_BWD16_BLOCKS, tuning build) on (2,280,56,128,3): 256 / 384 / 512 / 640 / 1024 -> 73.5 / 66.5 / 72.8 / 79.0 / 79.8 us; no other
// training shape has more window quads than blocks, so none moves ((2,140,28,256,3): 53.8 at 256, else 49.9-50.8).  384 (96 groups for 160
// quads) beats the shipped 512 on that one shape by 6 us; not adopted on a single shape and shift.
__global__ __launch_bounds__(256, 2) void win_attn_bwd_q_bf16mm_kernel(BwdArgs a) {
    __shared__ __attribute__((aligned(16))) uint32_t tok_in[4][64];
    __shared__ __attribute__((aligned(16))) uint32_t tok_out[4][64];
    __shared__ __attribute__((aligned(16))) float bias_s[WT * BLD];
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int c = lane & 31, h = lane >> 5;
    const int head = blockIdx.x % a.nH;
    const int slot = blockIdx.x / a.nH;
    const int64_t nwin = (int64_t)a.B * a.nW;
    stage_bias(bias_s, a.bias, head);
    const int64_t L = (int64_t)a.Hs * a.W;
    const uint32_t rsb = 12u * a.C, rob = 4u * a.C;
    uint32_t* ti = tok_in[wave];
    uint32_t* to = tok_out[wave];
    f32x16 dsum[2][2] = {};                                               // running sum of the fp32 dS^T over this wave's units

    for (int64_t bw = (int64_t)slot * 4 + wave; bw < nwin; bw += (int64_t)a.groups * 4) {
        // (the mask lookup comes first: a branch between the loads and their conversions would pin all raw rows at once)
        const float* mask_w = unit_mask(a, bw);
        const int64_t b = unit_tokens(a, bw, lane, rsb, rob, ti, to);
        const char* qb = reinterpret_cast<const char*>(a.qkv + b * L * 3 * a.C + head * HD);
        const char* kb = qb + 4 * a.C;
        const char* vb = qb + 8 * a.C;
        const char* dob = reinterpret_cast<const char*>(a.dout + b * L * a.C + head * HD);
        bf16x8 qf[2][2], kf[2][2], vkf[2][2], dof[2][2];                  // [tile][k-step]
        bf16x8 kp[2][2];                                                  // K in the permuted key order of the dS operand, lane = channel
#pragma unroll
        for (int t = 0; t < 2; ++t) {
            const uint32_t off = ti[32 * t + c] + 32u * h;
            load_frag_bf16(qf[t], qb, off);
            load_frag_bf16(kf[t], kb, off);
        }
        __builtin_amdgcn_sched_barrier(0);   // fp32 rows are twice their fragments: a batch is rounded before the next is issued
#pragma unroll
        for (int t = 0; t < 2; ++t) {
            load_frag_bf16(vkf[t], vb, ti[32 * t + c] + 32u * h);
            load_frag_bf16(dof[t], dob, to[32 * t + c] + 32u * h);
        }
        load_perm_bf16(kp, kb, ti, c, h);
        __builtin_amdgcn_sched_barrier(0);
        char* dqb = reinterpret_cast<char*>(a.dqkv + b * L * 3 * a.C + head * HD);
        float* st = a.stats + (bw * a.nH + head) * 192;                   // {m[64], inv[64], D[64]} of this unit
        // one branch per unit on the mask pointer, as in the forward: the tile code is straight-line, so nothing is sunk past a branch
        auto tiles = [&](auto masked) {
        constexpr bool MASKED = decltype(masked)::value;
#pragma unroll
        for (int it = 0; it < 2; ++it) {
            f32x16 s[2] = {};
#pragma unroll
            for (int ks = 0; ks < 2; ++ks)
#pragma unroll
                for (int jt = 0; jt < 2; ++jt) s[jt] = mfma16(kf[jt][ks], qf[it][ks], s[jt]);   // S^T = K Q^T
            // dP^T = V dO^T, one key tile at a time and computed TWICE (for D, then for dS; the same bits both times): two MFMAs more
            // per tile buy the 16 registers that keep the kernel at 2 waves per SIMD without scratch.  Chosen on the register count
            // alone: the form that keeps dP^T (and spills, or runs one wave per SIMD) was never timed against this one.
            auto dp_tile = [&](int jt) {
                f32x16 t = {};
#pragma unroll
                for (int ks = 0; ks < 2; ++ks) t = mfma16(vkf[jt][ks], dof[it][ks], t);
                return t;
            };
            const int qi = 32 * it + c;
            const auto bias_at = bias_row(bias_s, BLD, qi, h);
            float m, inv;
            bias_softmax<MASKED>(s, bias_at, mask_w, qi, h, a.scale, &m, &inv);
            float d = 0.f;
#pragma unroll
            for (int jt = 0; jt < 2; ++jt) {
                const f32x16 dp = dp_tile(jt);
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    if (jt == 1 && r >= 9) continue;                      // P == 0 on padded keys
                    d += s[jt][r] * dp[r];
                }
            }
            d += __shfl_xor(d, 32);
            const bool qvalid = qi < WT;
#pragma unroll
            for (int jt = 0; jt < 2; ++jt) {
                const f32x16 dp = dp_tile(jt);
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    if (jt == 1 && r >= 9) { s[jt][r] = 0.f; continue; }
                    const float ds = qvalid ? s[jt][r] * (dp[r] - d) : 0.f;        // padded queries contribute nothing
                    s[jt][r] = ds;
                    dsum[it][jt][r] += ds;
                }
            }
            if (h == 0 && qvalid) { st[qi] = m; st[64 + qi] = inv; st[128 + qi] = d; }
            f32x16 o = {};
#pragma unroll
            for (int jt = 0; jt < 2; ++jt)
#pragma unroll
                for (int ks = 0; ks < 2; ++ks) o = mfma16(acc_frag(s[jt], ks), kp[jt][ks], o);   // dQ = dS K   (rows = queries, lanes = channels)
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                if (acc_pad(it, g)) continue;
                const u32x4 ti4 = *reinterpret_cast<const u32x4*>(&ti[32 * it + 8 * g + 4 * h]);
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    if (acc_pad(it, g, e)) continue;
                    const int i = 32 * it + 8 * g + 4 * h + e;
                    if (i < WT) *reinterpret_cast<float*>(dqb + (ti4[e] + 4u * c)) = o[4 * g + e] * a.scale;
                }
            }
            __builtin_amdgcn_sched_barrier(0);   // one query tile at a time: interleaving the two doubles the live accumulators
        }
        };
        if (mask_w) tiles(std::true_type{}); else tiles(std::false_type{});
        __builtin_amdgcn_wave_barrier();   // the token tables are rewritten by the next unit
    }
    float* part = a.dbias_part + ((int64_t)blockIdx.x * 4 + wave) * 4096;  // [it][jt][r][lane]
#pragma unroll
    for (int it = 0; it < 2; ++it)
#pragma unroll
        for (int jt = 0; jt < 2; ++jt)
#pragma unroll
            for (int r = 0; r < 16; ++r) part[((it * 2 + jt) * 16 + r) * 64 + lane] = dsum[it][jt][r];
}

__global__ __launch_bounds__(256, 2) void win_attn_bwd_kv_bf16mm_kernel(BwdArgs a) {
    __shared__ __attribute__((aligned(16))) uint32_t tok_in[4][64];
    __shared__ __attribute__((aligned(16))) uint32_t tok_out[4][64];
    __shared__ __attribute__((aligned(16))) float biasT_s[WT * BLD];      // bias^T: row = key j, column = query i
    __shared__ __attribute__((aligned(16))) float stat_s[4][192];         // the unit's {m, 1/l, D}: one coalesced read, then 16-byte LDS reads
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int c = lane & 31, h = lane >> 5;
    const int head = blockIdx.x % a.nH;
    const int slot = blockIdx.x / a.nH;
    const int64_t nwin = (int64_t)a.B * a.nW;
    stage_bias_T(biasT_s, a.bias, head);
    const int64_t L = (int64_t)a.Hs * a.W;
    const uint32_t rsb = 12u * a.C, rob = 4u * a.C;
    uint32_t* ti = tok_in[wave];
    uint32_t* to = tok_out[wave];
    float* st = stat_s[wave];
    for (int64_t bw = (int64_t)slot * 4 + wave; bw < nwin; bw += (int64_t)a.groups * 4) {
        // (the mask lookup comes first: a branch between the loads and their conversions would pin all raw rows at once)
        const float* mask_w = unit_mask(a, bw);
        uint32_t tok;
        const int64_t b = unit_token(a, bw, lane, tok);
        {
            ti[lane] = tok * rsb;
            to[lane] = tok * rob;
            // query slots 49..63 were never written by the q kernel: finite filler (their P / dS are forced to 0 below)
            const float* sg = a.stats + (bw * a.nH + head) * 192;
#pragma unroll
            for (int k = 0; k < 3; ++k) st[64 * k + lane] = lane < WT ? sg[64 * k + lane] : 0.f;
        }
        __builtin_amdgcn_wave_barrier();
        const char* qb = reinterpret_cast<const char*>(a.qkv + b * L * 3 * a.C + head * HD);
        const char* kb = qb + 4 * a.C;
        const char* vb = qb + 8 * a.C;
        const char* dob = reinterpret_cast<const char*>(a.dout + b * L * a.C + head * HD);
        bf16x8 qf[2][2], kf[2][2], vkf[2][2], dof[2][2];                  // [tile][k-step]
        bf16x8 qp[2][2], dop[2][2];                                       // q / dO in the permuted query order of the P / dS operand
#pragma unroll
        for (int t = 0; t < 2; ++t) {
            const uint32_t off = ti[32 * t + c] + 32u * h;
            load_frag_bf16(qf[t], qb, off);
            load_frag_bf16(kf[t], kb, off);
        }
        __builtin_amdgcn_sched_barrier(0);   // fp32 rows are twice their fragments: a batch is rounded before the next is issued
#pragma unroll
        for (int t = 0; t < 2; ++t) {
            load_frag_bf16(vkf[t], vb, ti[32 * t + c] + 32u * h);
            load_frag_bf16(dof[t], dob, to[32 * t + c] + 32u * h);
        }
        __builtin_amdgcn_sched_barrier(0);
        load_perm_bf16(qp, qb, ti, c, h);
        load_perm_bf16(dop, dob, to, c, h);
        __builtin_amdgcn_sched_barrier(0);
        char* dkb = reinterpret_cast<char*>(a.dqkv + b * L * 3 * a.C + head * HD) + 4 * a.C;
        char* dvb = dkb + 4 * a.C;
        auto tiles = [&](auto masked) {                                   // one branch per unit on the mask pointer: straight-line tile code
        constexpr bool MASKED = decltype(masked)::value;
#pragma unroll
        for (int jt = 0; jt < 2; ++jt) {
            const int kj = 32 * jt + c;                                   // lane = key 32jt+c, accumulator rows = queries
            const int kjc = kj < WT ? kj : WT - 1;
            const float* brow = &biasT_s[kjc * BLD + 4 * h];
            f32x16 ov = {}, ok = {};
            // one query tile at a time, straight into dV / dK: S and dP of one tile are live (32 registers), not of both
#pragma unroll
            for (int it = 0; it < 2; ++it) {
                f32x4 mk[4];                                              // the key's mask row (the mask is symmetric in (i, j)): issued before the MFMAs
                if (MASKED) {
#pragma unroll
                    for (int g = 0; g < 4; ++g)
                        if (!(it == 1 && g == 3)) mk[g] = *reinterpret_cast<const f32x4*>(mask_w + kjc * 64 + 32 * it + 8 * g + 4 * h);
                }
                f32x16 s = {}, dp = {};
#pragma unroll
                for (int ks = 0; ks < 2; ++ks) {
                    s = mfma16(qf[it][ks], kf[jt][ks], s);                // S = Q K^T   (A = q rows, B = k rows)
                    dp = mfma16(dof[it][ks], vkf[jt][ks], dp);            // dP = dO V^T
                }
#pragma unroll
                for (int g = 0; g < 4; ++g) {
                    if (it == 1 && g == 3) {                              // queries 56..63: padding
#pragma unroll
                        for (int e = 0; e < 4; ++e) { s[4 * g + e] = 0.f; dp[4 * g + e] = 0.f; }
                        continue;
                    }
                    const int i0 = 32 * it + 8 * g + 4 * h;               // this lane's 4 consecutive queries i0 .. i0+3
                    const f32x4 bv = *reinterpret_cast<const f32x4*>(brow + 32 * it + 8 * g);
                    const f32x4 mv = *reinterpret_cast<const f32x4*>(st + i0);
                    const f32x4 iv = *reinterpret_cast<const f32x4*>(st + 64 + i0);
                    const f32x4 dv = *reinterpret_cast<const f32x4*>(st + 128 + i0);
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        const bool valid = (i0 + e < WT) && (kj < WT);
                        float x = s[4 * g + e] * a.scale + bv[e];                          // the operation order of bias_softmax
                        if (MASKED) x += mk[g][e];
                        const float pr = valid ? __expf(x - mv[e]) * iv[e] : 0.f;
                        s[4 * g + e] = pr;                                                 // P
                        dp[4 * g + e] = valid ? pr * (dp[4 * g + e] - dv[e]) : 0.f;        // dS
                    }
                }
#pragma unroll
                for (int ks = 0; ks < 2; ++ks) {
                    bf16x8 pf, df;                                        // (not acc_frag: the two casts interleaved, as LLVM schedules them here)
#pragma unroll
                    for (int j = 0; j < 8; ++j) { pf[j] = (__bf16)s[8 * ks + j]; df[j] = (__bf16)dp[8 * ks + j]; }
                    ov = mfma16(pf, dop[it][ks], ov);                     // dV = P^T dO   (sum over all 64 query slots)
                    ok = mfma16(df, qp[it][ks], ok);                      // dK = dS^T Q
                }
                __builtin_amdgcn_sched_barrier(0);   // the tiles one after the other: interleaved, their accumulators are all live at once
            }
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                if (acc_pad(jt, g)) continue;
                const u32x4 ti4 = *reinterpret_cast<const u32x4*>(&ti[32 * jt + 8 * g + 4 * h]);
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    if (acc_pad(jt, g, e)) continue;
                    const int j = 32 * jt + 8 * g + 4 * h + e;
                    if (j < WT) {
                        *reinterpret_cast<float*>(dvb + (ti4[e] + 4u * c)) = ov[4 * g + e];
                        *reinterpret_cast<float*>(dkb + (ti4[e] + 4u * c)) = ok[4 * g + e] * a.scale;
                    }
                }
            }
            __builtin_amdgcn_sched_barrier(0);
        }
        };
        if (mask_w) tiles(std::true_type{}); else tiles(std::false_type{});
        __builtin_amdgcn_wave_barrier();   // the token tables are rewritten by the next unit
    }
}

// dbias_full[head][i][j] = sum over that head's wave partials (fixed order: 4 lane groups take every 4th partial, then
// the groups are combined in order); partial layout [it][jt][r][lane]
__global__ __launch_bounds__(256) void win_attn_dbias_reduce_kernel(const float* __restrict__ part, float* __restrict__ full, int nH,
                                                                    int nblocks) {
    __shared__ float red[4][64];
    const int head = blockIdx.y;
    const int col = threadIdx.x & 63, grp = threadIdx.x >> 6;
    const int idx = blockIdx.x * 64 + col;                                // element of the 4096-float partial
    const int nparts = ((nblocks - head + nH - 1) / nH) * 4;             // this head's blocks x 4 waves
    // lane group grp takes wave grp of every block of this head, blocks in order: terms nH * 4 * 4096 floats apart
    float s = 0.f;
    if (grp < nparts)
        s = ordered_sum(part[((int64_t)head * 4 + grp) * 4096 + idx], part + ((int64_t)(head + nH) * 4 + grp) * 4096 + idx,
                        (int64_t)nH * 4 * 4096, nparts / 4 - 1);
    red[grp][col] = s;
    __syncthreads();
    if (grp) return;
    s = (red[0][col] + red[1][col]) + (red[2][col] + red[3][col]);
    const int lane = idx & 63, r = (idx >> 6) & 15, jt = (idx >> 10) & 1, it = idx >> 11;
    const int i = 32 * it + (lane & 31), j = 32 * jt + (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5);
    full[(int64_t)head * 4096 + i * 64 + j] = s;
}

// dtable[t][head] = sum over the (i, j) pairs with relative_position_index[i][j] == t: one wave per (t, head), lanes
// stride over the 2401 pairs in order, then a fixed-order wave reduction
__global__ __launch_bounds__(64) void win_attn_dtable_kernel(const float* __restrict__ full, const int32_t* __restrict__ rel_index,
                                                             float* __restrict__ dtable, int nH, int ntab, int accum) {
    const int t = blockIdx.x, head = blockIdx.y, lane = threadIdx.x;
    float s = 0.f;
    for (int p = lane; p < WT * WT; p += 64) {
        const int i = p / WT, j = p - i * WT;
        if (rel_index[p] == t) s += full[(int64_t)head * 4096 + i * 64 + j];
    }
    s = wave_sum(s, 64);
    if (lane == 0) dtable[(int64_t)t * nH + head] = accum ? dtable[(int64_t)t * nH + head] + s : s;
}

// the same through the inverse of relative_position_index (built once by the caller): csr = [ptr (ntab + 1) | pairs (49*49)], the pairs
// p = 49 i + j of table entry t are pairs[ptr[t] .. ptr[t+1]) in increasing p.  A wave per (t, head) reads ITS <= 49 values (the scan
// above walks all 2401 index entries in every one of the 169 x nH waves: 20 us per Swin block of the training step, 60 blocks).
__global__ __launch_bounds__(256) void win_attn_dtable_csr_kernel(const float* __restrict__ full, const int32_t* __restrict__ csr,
                                                                 float* __restrict__ dtable, int nH, int ntab, int accum) {
    const int lane = threadIdx.x & 63, t = blockIdx.x * 4 + (threadIdx.x >> 6), head = blockIdx.y;
    if (t >= ntab) return;
    const int p0 = csr[t], p1 = csr[t + 1];
    float s = 0.f;
    for (int e = p0 + lane; e < p1; e += 64) {
        const int p = csr[ntab + 1 + e], i = p / WT, j = p - i * WT;
        s += full[(int64_t)head * 4096 + i * 64 + j];
    }
    s = wave_sum(s, 64);
    if (lane == 0) dtable[(int64_t)t * nH + head] = accum ? dtable[(int64_t)t * nH + head] + s : s;
}

}  // namespace

static int64_t wa_bwd_groups(int B, int nW, int nH, bool mm16 = false) {
    const int64_t quads = ((int64_t)B * nW + 3) / 4;
    static const int target = tune_int("MUMPY_WA_BWD_BLOCKS", 256);
    static const int target16 = tune_int("MUMPY_WA_BWD16_BLOCKS", 512);
    // fp32 pair: ~one 4-wave block per CU (1 wave per SIMD); bf16-MFMA pair: two (2 waves per SIMD)
    int64_t groups = ((mm16 ? target16 : target) + nH - 1) / nH;
    return groups > quads ? quads : groups;
}

static int64_t wa_bwd_workspace_bytes(int B, int Hs, int W, int C, bool mm16) {
    if (B <= 0 || Hs <= 0 || W <= 0 || C <= 0 || Hs % WS || W % WS || C % HD) return 0;
    const int nW = (Hs / WS) * (W / WS), nH = C / HD;
    const int64_t stats = (int64_t)B * nW * nH * 192;
    const int64_t part = wa_bwd_groups(B, nW, nH, mm16) * nH * 4 * 4096;
    return (stats + part + (int64_t)nH * 4096) * (int64_t)sizeof(float);
}

extern "C" int64_t mumpy_window_attention_bwd_workspace_bytes(int B, int Hs, int W, int C) {
    return wa_bwd_workspace_bytes(B, Hs, W, C, false);
}

extern "C" int64_t mumpy_window_attention_mm16_bwd_workspace_bytes(int B, int Hs, int W, int C) {
    return wa_bwd_workspace_bytes(B, Hs, W, C, true);
}

static int window_attention_bwd_impl(bool mm16, const float* qkv, const float* dout, const float* bias, const float* mask_tab,
                                          const int32_t* mask_id, int n_mask, const int32_t* rel_index, const int32_t* rel_csr, float* dqkv,
                                          float* dtable, void* workspace, int64_t workspace_bytes, int B, int Hs, int W, int C,
                                          int shift, float scale, int accumulate, void* stream) {
    MUMPY_REQUIRE(qkv && dout && bias && rel_index && dqkv && dtable && workspace, MUMPY_ENULL, "window_attention_bwd: null pointer");
    MUMPY_REQUIRE(accumulate == 0 || accumulate == 1, MUMPY_EINVAL, "window_attention_bwd: accumulate must be 0 or 1");
    MUMPY_REQUIRE((mask_tab == nullptr) == (mask_id == nullptr), MUMPY_ENULL,
                  "window_attention_bwd: mask_tab and mask_id must be given together");
    MUMPY_REQUIRE(aligned16(qkv) && aligned16(dout) && aligned16(bias) && aligned16(mask_tab) && aligned16(dqkv) &&
                      aligned16(workspace), MUMPY_EALIGN, "window_attention_bwd: pointers must be 16-byte aligned");
    MUMPY_REQUIRE(B > 0 && Hs > 0 && W > 0 && Hs % WS == 0 && W % WS == 0, MUMPY_EINVAL,
                  "window_attention_bwd: grid (%d,%d) not divisible by window 7", Hs, W);
    MUMPY_REQUIRE(C > 0 && C % HD == 0 && shift >= 0 && shift < WS, MUMPY_EINVAL, "window_attention_bwd: bad C=%d / shift=%d", C, shift);
    MUMPY_REQUIRE(n_mask >= 0 && (mask_id == nullptr || n_mask > 0), MUMPY_EINVAL, "window_attention_bwd: n_mask must be > 0 with a mask (and never negative)");
    MUMPY_REQUIRE(workspace_bytes >= wa_bwd_workspace_bytes(B, Hs, W, C, mm16), MUMPY_EINVAL,
                  "window_attention_bwd: workspace too small");
    BwdArgs a;
    a.qkv = qkv; a.dout = dout; a.bias = bias; a.mask_tab = mask_tab; a.mask_id = mask_id; a.dqkv = dqkv;
    a.B = B; a.Hs = Hs; a.W = W; a.C = C; a.nH = C / HD; a.shift = shift; a.nWx = W / WS; a.nW = (Hs / WS) * (W / WS);
    a.n_mask = n_mask > 0 ? n_mask : 1; a.scale = scale;
    a.groups = (int)wa_bwd_groups(B, a.nW, a.nH, mm16);
    float* ws = static_cast<float*>(workspace);
    a.stats = ws;
    a.dbias_part = ws + (int64_t)B * a.nW * a.nH * 192;
    float* full = a.dbias_part + (int64_t)a.groups * a.nH * 4 * 4096;
    const unsigned grid = (unsigned)(a.groups * a.nH);
    if (mm16) hipLaunchKernelGGL(win_attn_bwd_q_bf16mm_kernel, dim3(grid), dim3(256), 0, as_stream(stream), a);
    else hipLaunchKernelGGL(win_attn_bwd_q_kernel, dim3(grid), dim3(256), 0, as_stream(stream), a);
    MUMPY_CHECK_LAUNCH("window_attention_bwd(q)");
    if (mm16) hipLaunchKernelGGL(win_attn_bwd_kv_bf16mm_kernel, dim3(grid), dim3(256), 0, as_stream(stream), a);
    else hipLaunchKernelGGL(win_attn_bwd_kv_kernel, dim3(grid), dim3(256), 0, as_stream(stream), a);
    MUMPY_CHECK_LAUNCH("window_attention_bwd(kv)");
    hipLaunchKernelGGL(win_attn_dbias_reduce_kernel, dim3(64, a.nH), dim3(256), 0, as_stream(stream), a.dbias_part, full, a.nH,
                       (int)grid);
    MUMPY_CHECK_LAUNCH("window_attention_bwd(dbias reduce)");
    const int ntab = (2 * WS - 1) * (2 * WS - 1);
    if (rel_csr)
        hipLaunchKernelGGL(win_attn_dtable_csr_kernel, dim3((ntab + 3) / 4, a.nH), dim3(256), 0, as_stream(stream), full, rel_csr, dtable,
                           a.nH, ntab, accumulate);
    else
        hipLaunchKernelGGL(win_attn_dtable_kernel, dim3(ntab, a.nH), dim3(64), 0, as_stream(stream), full, rel_index, dtable, a.nH,
                           ntab, accumulate);
    MUMPY_CHECK_LAUNCH("window_attention_bwd(dtable)");
    return 0;
}

extern "C" int mumpy_window_attention_bwd(const float* qkv, const float* dout, const float* bias, const float* mask_tab,
                                          const int32_t* mask_id, int n_mask, const int32_t* rel_index, float* dqkv,
                                          float* dtable, void* workspace, int64_t workspace_bytes, int B, int Hs, int W, int C,
                                          int shift, float scale, int accumulate, void* stream) {
    return window_attention_bwd_impl(false, qkv, dout, bias, mask_tab, mask_id, n_mask, rel_index, nullptr, dqkv, dtable, workspace,
                                     workspace_bytes, B, Hs, W, C, shift, scale, accumulate, stream);
}

extern "C" int mumpy_window_attention_bwd_csr(const float* qkv, const float* dout, const float* bias, const float* mask_tab,
                                              const int32_t* mask_id, int n_mask, const int32_t* rel_index, const int32_t* rel_csr,
                                              float* dqkv, float* dtable, void* workspace, int64_t workspace_bytes, int B, int Hs, int W,
                                              int C, int shift, float scale, int accumulate, void* stream) {
    MUMPY_REQUIRE(rel_csr, MUMPY_ENULL, "window_attention_bwd_csr: null inverse index");
    return window_attention_bwd_impl(false, qkv, dout, bias, mask_tab, mask_id, n_mask, rel_index, rel_csr, dqkv, dtable, workspace,
                                     workspace_bytes, B, Hs, W, C, shift, scale, accumulate, stream);
}

// bf16 matrix math on the fp32-stored tape (opt-in): the argument list of mumpy_window_attention_bwd_csr; rel_csr may be null (the
// index-scanning table kernel); workspace from mumpy_window_attention_mm16_bwd_workspace_bytes.
extern "C" int mumpy_window_attention_mm16_bwd(const float* qkv, const float* dout, const float* bias, const float* mask_tab,
                                               const int32_t* mask_id, int n_mask, const int32_t* rel_index, const int32_t* rel_csr,
                                               float* dqkv, float* dtable, void* workspace, int64_t workspace_bytes, int B, int Hs, int W,
                                               int C, int shift, float scale, int accumulate, void* stream) {
    return window_attention_bwd_impl(true, qkv, dout, bias, mask_tab, mask_id, n_mask, rel_index, rel_csr, dqkv, dtable, workspace,
                                     workspace_bytes, B, Hs, W, C, shift, scale, accumulate, stream);
}
