// deform_attention.hip — the deformable cross-view attention + aggregation in window form, forward (win_attn_cross_kernel) and
// backward (deform_attn_bwd_{q,kv}_kernel), and their entry points.  Same (window, head) unit per wave as the Swin self-attention
// (win_attn_unit.h), fp32 MFMA, but not persistent: no bias table (only the 49 -> 64 key padding), the scale on the product, q
// gathered from the raster, k/v window-major.
//
// Small grids: one unit on two waves (win_attn_cross_kernel<SPLIT = true>; mumpy_deform_attention_plan bit 0).  The launches of the
// forward have 192 .. 1,536 units: one wave per unit leaves most of the chip idle while each wave walks r x 114 MFMAs alone.  Split by
// 32-query tile the chain is r x 57 MFMAs; the r kv windows stay inside each wave in the order t = 0 .. r-1, so the output is bitwise
// the same (tests/test_window_attention_schedule.py).  Fitted rule (cross_plan): split while units <= 1,024 -- what 256 CUs x 2
// resident blocks x 2 units hold, i.e. while every split block is resident at once.  Both forms of every shape of the B=8, T=5 forward
// (each launched with r = 1 against view 2 and r = 5 against view 3), timed on one MI355X against the parent commit's library
// (tools/kernel_micro.py cva_attn: medians of 12 alternating replays of 20 captured launches, us per launch; "whole" = <SPLIT = false>;
// the parent's own repeats differ by <= 0.1 us):
//   (B, H, W, C)      units   r = 1: parent  whole  split     r = 5: parent  whole  split     plan
//   (8, 56, 56,  96)  1,536          15.9   15.9   15.0             56.5   56.6   56.9      whole (r = 5 is slower split)
//   (8, 28, 28, 192)    768          10.2   10.1    9.7             35.7   35.6   32.8      split
//   (8, 14, 14, 384)    384           9.5    9.5    6.9             34.6   34.6   22.9      split
//   (8,  7,  7, 768)    192           9.3    9.2    6.7             33.3   33.3   21.6      split
//
// win_attn_cross_mm16_kernel (mumpy_deform_attention_mm16_fwd; opt-in, ops.set_cva_math("bf16")) is the forward on
// v_mfma_f32_32x32x16_bf16, built like win_attn_self_bf16mm_kernel<IO32 = true>: q / k rows rounded to bf16 in registers, S^T = K Q^T
// so that the exponentials feed P V from the accumulator registers, V gathered in that permuted key order, the scale on the fp32 scores,
// P rounded unnormalised with the fp32 row sum's reciprocal applied to the fp32 product -- here once per kv window t, as the r-tuple
// sum o += (P_t V_t) / sum_t is accumulated in registers in the order t = 0 .. r-1.
//
// Replaces: the attention + "(b t)->b t" sum of SwinDAttention (deform:360-395).
// Resources (hipcc -Rpass-analysis=kernel-resource-usage, gfx950; VGPRs + AGPRs / SGPRs / LDS per block / waves per SIMD; no scratch):
//   win_attn_cross_kernel<false> 229 + 0 / 47 / 1,024 B / 2;   win_attn_cross_kernel<true> 194 + 0 / 50 / 1,024 B / 2 (no spills);
//   win_attn_cross_mm16_kernel 160 + 0 / 46 / 3,072 B / 3;
//   deform_attn_bwd_q_kernel 180 + 80 / 40 / 0 / 1;   deform_attn_bwd_kv_kernel 256 + 62 / 44 / 0 / 1;
//   deform_attn_bwd_q_bf16mm_kernel 147 + 0 / 71 / 1,024 B / 3;   deform_attn_bwd_kv_bf16mm_kernel 199 + 0 / 48 / 5,120 B / 2
//
// deform_attn_bwd_{q,kv}_bf16mm_kernel (mumpy_deform_attention_mm16_bwd, include/mumpy_hip_ext2.h; opt-in through the same switch on the
// training tape) are the backward of win_attn_cross_mm16_kernel on the bf16 MFMA; their form, arithmetic and measurements are above them.
#include <stdlib.h>
#include "win_attn_unit.h"
#include "cva_pairing.h"
#include "../../include/mumpy_hip_ext2.h"
#include "../../include/mumpy_hip_ext8.h"
#include "../../include/mumpy_hip_ext9.h"

namespace {

// GROUPED (the three forward kernels): the pairing rule of cva_pairing.h.  <false> carries the q window count B1w alone, where it
// always was in this struct, and is the kernel it was.
template <bool GROUPED>
struct CrossArgs {
    const float* q;        // (B, H*W, C) raster
    const float* kv;       // (B2w, 49, 2C) window-major
    const float* padmask;  // (1,64,64)
    float* out;            // (B1w, 49, C) window-major
    int B, H, W, C, nH, r, nWx, nWf;
    CvaPairing<GROUPED> pair;   // .nq = B1w
    float scale;
    int64_t units;
};

// no bias in these kernels, only the 49 -> 64 key padding: 0 on real keys, -1e30 on key 52 (keys 49..51 / 53.. are skipped)
__device__ __forceinline__ f32x4 pad_bias(int jt, int g, int h) { return pad_key52(f32x4{0.f, 0.f, 0.f, 0.f}, jt, g, h); }

// ---------------------------------------------------------------------------------------------------------------
// SPLIT (small grids, see cross_plan): ONE unit on TWO waves, split by query tile.  The two 32-query tiles of a unit share only K
// and V, so wave 2p + it of a block takes tile `it` of the block's unit p: per kv window it loads all of K and V (the second reader
// hits L2) and its own 32 queries and runs one qk_product / bias_softmax / pv_product.  The loop over the r kv windows stays inside
// the wave, in the order t = 0 .. r-1, and every product and softmax is the same instruction sequence on the same values, so the
// outputs are bitwise those of the one-wave form; a unit's dependent chain is roughly half as long.
template <bool SPLIT, bool GROUPED>
__global__ __launch_bounds__(256, 2) void win_attn_cross_kernel(CrossArgs<GROUPED> a) {
    __shared__ int tok_tab[4][64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int c = lane & 31, h = lane >> 5;
    const int it0 = SPLIT ? __builtin_amdgcn_readfirstlane(wave & 1) : 0;      // SPLIT: this wave's query tile
    const int64_t u = SPLIT ? (int64_t)blockIdx.x * 2 + (wave >> 1) : (int64_t)blockIdx.x * 4 + wave;
    if (u >= a.units) return;
    const int head = (int)(u % a.nH);
    const int64_t b1 = u / a.nH;                 // output window
    int* tt = tok_tab[wave];
    const int64_t L = (int64_t)a.H * a.W;
    constexpr int NT = SPLIT ? 1 : 2;            // query tiles of this wave
    f32x16 o[NT] = {};

    for (int t = 0; t < a.r; ++t) {
        const int64_t b2 = b1 * a.r + t;                  // kv window; adjacent r-tuples are summed (deform:394-395)
        const int qw = (int)cva_q_window(b2, a.pair);     // q window = kv window mod B1 (x1.repeat, deform:330), per group
        const int qb = qw / a.nWf, qn = qw - qb * a.nWf;
        const int wy = qn / a.nWx, wx = qn - wy * a.nWx;
        __builtin_amdgcn_wave_barrier();
        tt[lane] = (lane < WT) ? window_token(wy, wx, lane, a.H, a.W, 0) : 0;
        __builtin_amdgcn_wave_barrier();
        const float* qbase = a.q + ((int64_t)qb * L) * a.C + head * HD;
        const float* kbase = a.kv + b2 * WT * 2 * a.C + head * HD;
        f32x4 qf[NT][4], kf[2][4];
#pragma unroll
        for (int tl = 0; tl < 2; ++tl) {
            const int p = 32 * tl + c;
            const bool valid = p < WT;
            if (!SPLIT) load_frag(qf[tl], qbase + (int64_t)tt[p & 63] * a.C + 16 * h, valid);
            load_frag(kf[tl], kbase + (int64_t)(valid ? p : 0) * 2 * a.C + 16 * h, valid);
        }
        if (SPLIT) {
            const int p = 32 * it0 + c;
            load_frag(qf[0], qbase + (int64_t)tt[p & 63] * a.C + 16 * h, p < WT);
        }
        float vf[2][16];
        const float* vbase = kbase + a.C;
        load_v(vf, [&](int j) { return vbase + (int64_t)j * 2 * a.C; }, c, h);

#pragma unroll
        for (int it = 0; it < NT; ++it) {
            f32x16 s[2] = {};
            qk_product(s, kf, qf[it]);
            bias_softmax<false>(s, [&](int jt, int g) { return pad_bias(jt, g, h); }, nullptr, 32 * (it0 + it) + c, h,
                                a.scale);                                       // scale on the product (deform:364)
            pv_product(o[it], s, vf);
        }
    }
    float* obase = a.out + b1 * WT * a.C + head * HD;
    if constexpr (SPLIT) {
        if (it0 == 0) store_o(o[0], 0, [&](int i) { return obase + (int64_t)i * a.C; }, c, h);
        else store_o(o[0], 1, [&](int i) { return obase + (int64_t)i * a.C; }, c, h);
    } else {
        store_o(o[0], 0, [&](int i) { return obase + (int64_t)i * a.C; }, c, h);
        store_o(o[1], 1, [&](int i) { return obase + (int64_t)i * a.C; }, c, h);
    }
}

// ---------------------------------------------------------------------------------------------------------------
// The same unit on the bf16 MFMA: 8 + 8 MFMAs per kv window instead of 64 + 50.  Token tables hold byte offsets: tq the q rows of the
// raster (rewritten per kv window, its q window changes with t), tk the kv rows of a window (slot * 8C, the same for every t); padded
// slots 49..63 are clamped to slot 48 -- finite duplicates whose scores get -1e30 (keys) or are never stored (queries).  1 / row sum
// lives on the query's lane and the product has the query in its registers: it crosses through 64 floats of LDS per wave.
template <bool GROUPED>
__global__ __launch_bounds__(256, 2) void win_attn_cross_mm16_kernel(CrossArgs<GROUPED> a) {
    __shared__ __attribute__((aligned(16))) uint32_t tok_q[4][64];
    __shared__ __attribute__((aligned(16))) uint32_t tok_k[4][64];
    __shared__ __attribute__((aligned(16))) float inv_s[4][64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int c = lane & 31, h = lane >> 5;
    const int64_t u = (int64_t)blockIdx.x * 4 + wave;
    if (u >= a.units) return;
    const int head = (int)(u % a.nH);
    const int64_t b1 = u / a.nH;                 // output window
    uint32_t* tq = tok_q[wave];
    uint32_t* tk = tok_k[wave];
    float* invw = inv_s[wave];
    const int64_t L = (int64_t)a.H * a.W;
    const int slot = lane < WT ? lane : WT - 1;
    tk[lane] = (uint32_t)slot * 8u * a.C;
    f32x16 o[2] = {};

    for (int t = 0; t < a.r; ++t) {
        const int64_t b2 = b1 * a.r + t;                  // kv window; adjacent r-tuples are summed (deform:394-395)
        const int qw = (int)cva_q_window(b2, a.pair);     // q window = kv window mod B1 (x1.repeat, deform:330), per group
        const int qb = qw / a.nWf, qn = qw - qb * a.nWf;
        const int wy = qn / a.nWx, wx = qn - wy * a.nWx;
        __builtin_amdgcn_wave_barrier();
        tq[lane] = (uint32_t)window_token(wy, wx, slot, a.H, a.W, 0) * 4u * a.C;
        __builtin_amdgcn_wave_barrier();
        const char* qbase = reinterpret_cast<const char*>(a.q + ((int64_t)qb * L) * a.C + head * HD);
        const char* kbase = reinterpret_cast<const char*>(a.kv + b2 * WT * 2 * a.C + head * HD);
        bf16x8 qf[2][2], kf[2][2], vf[2][2];
#pragma unroll
        for (int tl = 0; tl < 2; ++tl) {
            load_frag_bf16(qf[tl], qbase, tq[32 * tl + c] + 32u * h);
            load_frag_bf16(kf[tl], kbase, tk[32 * tl + c] + 32u * h);
        }
        load_perm_bf16(vf, kbase + 4 * a.C, tk, c, h);
        if (h) vf[1][1][0] = (__bf16)0.f;                 // key 52 (slot 48's value through the clamp): V is 0 on every padded key

#pragma unroll
        for (int it = 0; it < 2; ++it) {
            f32x16 s[2] = {};
#pragma unroll
            for (int st = 0; st < 2; ++st)
#pragma unroll
                for (int jt = 0; jt < 2; ++jt) s[jt] = mfma16(kf[jt][st], qf[it][st], s[jt]);       // S^T[jt] += K[jt] Q[it]^T
            const int qi = 32 * it + c;
            float m, inv;
            bias_softmax<false, false>(s, [&](int jt, int g) { return pad_bias(jt, g, h); }, nullptr, qi, h, a.scale, &m,
                                       &inv);                                   // scale on the product (deform:364)
            invw[qi] = inv;                                                     // both lane halves hold the same value
            f32x16 pv = {};
#pragma unroll
            for (int jt = 0; jt < 2; ++jt)
#pragma unroll
                for (int st = 0; st < 2; ++st) pv = mfma16(acc_frag(s[jt], st), vf[jt][st], pv);
            __builtin_amdgcn_wave_barrier();
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                if (acc_pad(it, g)) continue;
                const f32x4 iv = *reinterpret_cast<const f32x4*>(&invw[32 * it + 8 * g + 4 * h]);   // queries 32it + 8g + 4h .. +3
#pragma unroll
                for (int e = 0; e < 4; ++e) o[it][4 * g + e] += pv[4 * g + e] * iv[e];
            }
        }
    }
    float* obase = a.out + b1 * WT * a.C + head * HD;
    store_o(o[0], 0, [&](int i) { return obase + (int64_t)i * a.C; }, c, h);
    store_o(o[1], 1, [&](int i) { return obase + (int64_t)i * a.C; }, c, h);
}

// ---------------------------------------------------------------------------------------------------------------
// backward of the deformable cross-view attention core (deform:360-395 in window form): unit = (kv window b2, head);
// q from q window b2 % B1w (x1.repeat, deform:330), k/v from kv[b2], dO from output window b2 / r (the r-tuple sum,
// deform:394-395, hands the same dO to its r members).  Same two-orientation scheme as the self-attention backward;
// no bias (only the 49 -> 64 key padding), scale on the product.  dq_part holds each kv window's contribution to its q
// window; the caller sums the r contributions per q window.
// GROUPED (all four backward kernels, include/mumpy_hip_ext9.h): the pairing rule of cva_pairing.h, as in the forward kernels.  <false>
// carries the q window count alone, where it always was (.nq = B1w), and computes what it computed.
// Resources of the fp32 pair (hipcc -Rpass-analysis=kernel-resource-usage, gfx950), <false> -> <true>: q kernel 180 VGPRs + 80 AGPRs /
// 40 -> 44 SGPRs, kv kernel 256 + 62 / 44 -> 48 SGPRs; no LDS, 1 wave per SIMD, no scratch, no spill in all four.
template <bool GROUPED>
struct CrossBwdArgs {
    const float* q; const float* kv; const float* dout;
    float* dq_part; float* dkv; float* stats;
    int C, nH, r;
    CvaPairing<GROUPED> pair;   // .nq = B1w
    float scale;
    int64_t units;
};

template <bool GROUPED>
__global__ __launch_bounds__(256, 1) void deform_attn_bwd_q_kernel(CrossBwdArgs<GROUPED> a) {
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int c = lane & 31, h = lane >> 5;
    const int64_t u = (int64_t)blockIdx.x * 4 + wave;
    if (u >= a.units) return;
    const int head = (int)(u % a.nH);
    const int64_t b2 = u / a.nH;
    const int64_t qw = cva_q_window(b2, a.pair), b1 = b2 / a.r;
    const uint32_t rq = 4u * a.C, rk = 8u * a.C;                          // row pitches in bytes
    const char* qb = reinterpret_cast<const char*>(a.q + qw * WT * a.C + head * HD);
    const char* kb = reinterpret_cast<const char*>(a.kv + b2 * WT * 2 * a.C + head * HD);
    const char* vb = kb + 4 * a.C;
    const char* dob = reinterpret_cast<const char*>(a.dout + b1 * WT * a.C + head * HD);
    auto row = [](int p) { return (uint32_t)(p < WT ? p : WT - 1); };     // padded slots re-read row 48
    f32x4 qf[2][4], kf[2][4], vkf[2][4], dof[2][4];
    float kv[2][16];
#pragma unroll
    for (int t = 0; t < 2; ++t) {
        const uint32_t p = row(32 * t + c);
        load_frag16(qf[t], qb, p * rq + 64u * h);
        load_frag16(kf[t], kb, p * rk + 64u * h);
        load_frag16(vkf[t], vb, p * rk + 64u * h);
        load_frag16(dof[t], dob, p * rq + 64u * h);
    }
    for_pv_steps([&](int jt, int g, int e) {
        kv[jt][4 * g + e] = *reinterpret_cast<const float*>(kb + (row(32 * jt + 8 * g + 4 * h + e) * rk + 4u * c));
    });
    char* dqb = reinterpret_cast<char*>(a.dq_part + b2 * WT * a.C + head * HD);
    float* st = a.stats + u * 192;
#pragma unroll
    for (int it = 0; it < 2; ++it) {
        f32x16 s[2] = {}, dp[2] = {};
        qk_product(s, kf, qf[it]);
        const int qi = 32 * it + c;
        float m, inv;
        bias_softmax<false>(s, [&](int jt, int g) { return pad_bias(jt, g, h); }, nullptr, qi, h, a.scale, &m, &inv);
        qk_product(dp, vkf, dof[it]);
        float d = 0.f;
#pragma unroll
        for (int jt = 0; jt < 2; ++jt)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                if (jt == 1 && r >= 9) continue;
                d += s[jt][r] * dp[jt][r];
            }
        d += __shfl_xor(d, 32);
        const bool qvalid = qi < WT;
#pragma unroll
        for (int jt = 0; jt < 2; ++jt)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                if (jt == 1 && r >= 9) { s[jt][r] = 0.f; continue; }
                s[jt][r] = qvalid ? s[jt][r] * (dp[jt][r] - d) : 0.f;
            }
        if (h == 0 && qvalid) { st[qi] = m; st[64 + qi] = inv; st[128 + qi] = d; }
        f32x16 o = {};
        pv_product(o, s, kv);                                             // dQ = dS K
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            if (!acc_live(it, r)) continue;
            const int i = acc_row(it, r, h);
            if (i < WT) *reinterpret_cast<float*>(dqb + ((uint32_t)i * rq + 4u * c)) = o[r] * a.scale;
        }
    }
}

template <bool GROUPED>
__global__ __launch_bounds__(256, 1) void deform_attn_bwd_kv_kernel(CrossBwdArgs<GROUPED> a) {
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int c = lane & 31, h = lane >> 5;
    const int64_t u = (int64_t)blockIdx.x * 4 + wave;
    if (u >= a.units) return;
    const int head = (int)(u % a.nH);
    const int64_t b2 = u / a.nH;
    const int64_t qw = cva_q_window(b2, a.pair), b1 = b2 / a.r;
    const uint32_t rq = 4u * a.C, rk = 8u * a.C;
    const char* qb = reinterpret_cast<const char*>(a.q + qw * WT * a.C + head * HD);
    const char* kb = reinterpret_cast<const char*>(a.kv + b2 * WT * 2 * a.C + head * HD);
    const char* vb = kb + 4 * a.C;
    const char* dob = reinterpret_cast<const char*>(a.dout + b1 * WT * a.C + head * HD);
    auto row = [](int p) { return (uint32_t)(p < WT ? p : WT - 1); };
    f32x4 qf[2][4], kf[2][4], vkf[2][4], dof[2][4];
    float qv[2][16], dov[2][16];
#pragma unroll
    for (int t = 0; t < 2; ++t) {
        const uint32_t p = row(32 * t + c);
        load_frag16(qf[t], qb, p * rq + 64u * h);
        load_frag16(kf[t], kb, p * rk + 64u * h);
        load_frag16(vkf[t], vb, p * rk + 64u * h);
        load_frag16(dof[t], dob, p * rq + 64u * h);
    }
    for_pv_steps([&](int it, int g, int e) {
        const uint32_t i = row(32 * it + 8 * g + 4 * h + e);
        qv[it][4 * g + e] = *reinterpret_cast<const float*>(qb + (i * rq + 4u * c));
        dov[it][4 * g + e] = *reinterpret_cast<const float*>(dob + (i * rq + 4u * c));
    });
    char* dkb = reinterpret_cast<char*>(a.dkv + b2 * WT * 2 * a.C + head * HD);
    char* dvb = dkb + 4 * a.C;
    const float* st = a.stats + u * 192;
#pragma unroll
    for (int jt = 0; jt < 2; ++jt) {
        f32x16 s[2] = {}, dp[2] = {};
        qk_product(s, qf, kf[jt]);                                        // S = Q K^T (unscaled; scale applied below)
        qk_product(dp, dof, vkf[jt]);                                     // dP = dO V^T
        const int kj = 32 * jt + c;
#pragma unroll
        for (int it = 0; it < 2; ++it)
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                if (it == 1 && g == 3) {
#pragma unroll
                    for (int e = 0; e < 4; ++e) { s[it][4 * g + e] = 0.f; dp[it][4 * g + e] = 0.f; }
                    continue;
                }
                const int i0 = 32 * it + 8 * g + 4 * h;
                const f32x4 mv = *reinterpret_cast<const f32x4*>(st + i0);
                const f32x4 iv = *reinterpret_cast<const f32x4*>(st + 64 + i0);
                const f32x4 dv = *reinterpret_cast<const f32x4*>(st + 128 + i0);
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const bool valid = (i0 + e < WT) && (kj < WT);
                    const float pr = valid ? __expf(s[it][4 * g + e] * a.scale - mv[e]) * iv[e] : 0.f;
                    s[it][4 * g + e] = pr;
                    dp[it][4 * g + e] = valid ? pr * (dp[it][4 * g + e] - dv[e]) * a.scale : 0.f;   // scale: dS/d(q k)
                }
            }
        f32x16 ov = {}, ok = {};
        pv_product(ov, s, dov);                                           // dV = P^T dO
        pv_product(ok, dp, qv);                                           // dK = scale dS^T Q
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            if (!acc_live(jt, r)) continue;
            const int j = acc_row(jt, r, h);
            if (j < WT) {
                *reinterpret_cast<float*>(dvb + ((uint32_t)j * rk + 4u * c)) = ov[r];
                *reinterpret_cast<float*>(dkb + ((uint32_t)j * rk + 4u * c)) = ok[r];
            }
        }
    }
}

// ---------------------------------------------------------------------------------------------------------------
// The backward on the bf16 MFMA (mumpy_deform_attention_mm16_bwd): the pair of win_attn_cross_mm16_kernel, built like
// win_attn_bwd_{q,kv}_bf16mm_kernel without the bias table, the mask, the dBias sum and the persistent walk.  Rows are window-major, so
// the "token tables" are the row tables slot * pitch (4C bytes for q / dO, 8C for kv; padded slots 49..63 clamped to row 48), the same
// for every unit.  Arithmetic, r(x) = bf16 rounding (nearest even), everything else fp32:
//   S = scale (r(q) r(k)^T),  P = softmax(S) over the 49 real keys,  dP = r(dO) r(v)^T,  D = rowsum(P o dP),  dS = P o (dP - D)
//   dV = r(P)^T r(dO),  dK = scale r(dS)^T r(q),  dQ[qw] = sum over m = 0 .. r-1, in that order, of scale r(dS_b2) r(k_b2), b2 = qw + m B1w
// P and dS are exactly 0 on padded keys / queries BEFORE they are rounded, so the finite duplicates of row 48 are multiplied by 0.
// Shipped form: the preferred one.  The q kernel's unit is (q window, head, 32-query tile), one wave each (tile = unit & 1, so the two
// tiles of a (window, head) sit in neighbouring waves and share their K / V rows through L1 / L2): the wave rounds its Q tile once and
// walks the r members b2 = qw + m B1w, reloading K, V, the permuted K and the dO tile of output window b2 / r, and adds each member's
// scale * (dS K) to dQ in registers in the order m = 0 .. r-1.  dq comes out final: no per-member partials, no reduce launch, and the
// order is fixed, so the result is deterministic.  With one query tile per wave both dP^T tiles are kept (not computed twice as in
// the W-MSA q kernel) and the kernel still holds 2 waves per SIMD without scratch.  The q kernel writes the record {m, 1/l, D} of every
// (b2, head) (192 floats; each tile's wave its own queries); the kv kernel's unit is (b2, head), one query tile at a time straight into
// dV / dK.
// Resources (hipcc -Rpass-analysis=kernel-resource-usage, gfx950): q kernel 147 VGPRs / 71 SGPRs / 1,024 B of LDS per block, 3 waves per
// SIMD; kv kernel 199 / 48 / 5,120 B, 2 waves per SIMD; 0 AGPRs and no scratch in both (the fp32 pair: 180 + 80 and 256 + 62 registers,
// 1 wave per SIMD).  The <GROUPED = true> instantiations: q kernel 147 / 70 / 1,024 B, kv kernel 199 / 52 / 5,120 B, the same occupancy,
// 0 AGPRs, no scratch, no spill.
// Measured against the fp32 entry on the same input (tools/kernel_micro.py cva_attn_bwd16; profiles/bf16_cva_train.md): the eight
// (B1w, r, C) launches of the B=2, T=5 training step, us on one MI355X, medians of 12 alternating replays of 20 captured calls; the
// backward is the whole entry -- fp32: q kernel, kv kernel and the r - 1 add launches of ops.deform_attention_bwd; bf16: two launches:
//   (B1w, r, C)     backward: fp32 -> bf16 MFMA      forward: fp32 -> bf16 MFMA
//   (128, 1,  96)   25.2 -> 14.0 (1.80x)             6.9 ->  6.0
//   (128, 5,  96)   65.7 -> 31.6 (2.08x)            22.0 -> 18.8
//   ( 32, 1, 192)   24.7 -> 13.1 (1.89x)             6.8 ->  5.8
//   ( 32, 5, 192)   38.6 -> 26.8 (1.44x)            21.0 -> 16.8
//   (  8, 1, 384)   24.3 -> 12.8 (1.89x)             6.6 ->  5.7
//   (  8, 5, 384)   34.3 -> 24.0 (1.43x)            21.7 -> 16.7
//   (  2, 1, 768)   24.1 -> 12.7 (1.90x)             6.7 ->  5.8
//   (  2, 5, 768)   32.1 -> 22.0 (1.46x)            21.6 -> 16.2
// No shape is slower.  The graphed B=2 step, switch off -> on, alternating: 33.64 -> 33.53 ms under bf16 matrix math, 40.38 -> 40.28 ms
// under fp32 (eight such launches per step).  Not measured: the two kernels separately (no kernel trace was taken), and the fallback form.
template <bool GROUPED>
struct CrossBwd16Args {
    const float* q; const float* kv; const float* dout;
    float* dq; float* dkv; float* stats;
    int C, nH, r;
    CvaPairing<GROUPED> pair;       // .nq = B1w
    float scale;
    int64_t units_q, units_kv;      // B1w nH 2 and B1w r nH
};

template <bool GROUPED>
__global__ __launch_bounds__(256, 2) void deform_attn_bwd_q_bf16mm_kernel(CrossBwd16Args<GROUPED> a) {
    __shared__ __attribute__((aligned(16))) uint32_t row_k[4][64];
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int c = lane & 31, h = lane >> 5;
    const int64_t u = (int64_t)blockIdx.x * 4 + wave;
    if (u >= a.units_q) return;
    const int it = (int)(u & 1);                                          // this wave's query tile
    const int head = (int)((u >> 1) % a.nH);
    const int64_t qw = (u >> 1) / a.nH;
    const uint32_t rq = 4u * a.C, rk = 8u * a.C;                          // row pitches in bytes
    uint32_t* tk = row_k[wave];
    tk[lane] = (uint32_t)(lane < WT ? lane : WT - 1) * rk;
    __builtin_amdgcn_wave_barrier();
    const int qi = 32 * it + c;
    const bool qvalid = qi < WT;
    const uint32_t qoff = (uint32_t)(qvalid ? qi : WT - 1) * rq + 32u * h;
    bf16x8 qf[2];
    load_frag_bf16(qf, reinterpret_cast<const char*>(a.q + qw * WT * a.C + head * HD), qoff);
    f32x16 dq = {};

    for (int m = 0; m < a.r; ++m) {
        const int64_t b2 = cva_kv_window(qw, m, a.pair);                  // kv windows qw + m B1w pair with q window qw (deform:330), per group
        const int64_t b1 = b2 / a.r;                                      // ... and take dO of output window b2 / r (deform:394-395)
        const char* kb = reinterpret_cast<const char*>(a.kv + b2 * WT * 2 * a.C + head * HD);
        const char* vb = kb + 4 * a.C;
        const char* dob = reinterpret_cast<const char*>(a.dout + b1 * WT * a.C + head * HD);
        bf16x8 kf[2][2], vkf[2][2], dof[2];                               // [tile][k-step]
        bf16x8 kp[2][2];                                                  // K in the permuted key order of the dS operand, lane = channel
#pragma unroll
        for (int t = 0; t < 2; ++t) load_frag_bf16(kf[t], kb, tk[32 * t + c] + 32u * h);
        load_frag_bf16(dof, dob, qoff);
        __builtin_amdgcn_sched_barrier(0);   // fp32 rows are twice their fragments: a batch is rounded before the next is issued
#pragma unroll
        for (int t = 0; t < 2; ++t) load_frag_bf16(vkf[t], vb, tk[32 * t + c] + 32u * h);
        load_perm_bf16(kp, kb, tk, c, h);
        __builtin_amdgcn_sched_barrier(0);
        float* st = a.stats + (b2 * a.nH + head) * 192;                   // {m[64], inv[64], D[64]} of the unit (b2, head)

        f32x16 s[2] = {}, dp[2] = {};
#pragma unroll
        for (int ks = 0; ks < 2; ++ks)
#pragma unroll
            for (int jt = 0; jt < 2; ++jt) {
                s[jt] = mfma16(kf[jt][ks], qf[ks], s[jt]);                // S^T = K Q^T
                dp[jt] = mfma16(vkf[jt][ks], dof[ks], dp[jt]);            // dP^T = V dO^T
            }
        float mx, inv;
        bias_softmax<false>(s, [&](int jt, int g) { return pad_bias(jt, g, h); }, nullptr, qi, h, a.scale, &mx, &inv);
        float d = 0.f;
#pragma unroll
        for (int jt = 0; jt < 2; ++jt)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                if (jt == 1 && r >= 9) continue;                          // P == 0 on padded keys
                d += s[jt][r] * dp[jt][r];
            }
        d += __shfl_xor(d, 32);
#pragma unroll
        for (int jt = 0; jt < 2; ++jt)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                if (jt == 1 && r >= 9) { s[jt][r] = 0.f; continue; }
                s[jt][r] = qvalid ? s[jt][r] * (dp[jt][r] - d) : 0.f;     // padded queries contribute nothing
            }
        if (h == 0 && qvalid) { st[qi] = mx; st[64 + qi] = inv; st[128 + qi] = d; }
        f32x16 o = {};
#pragma unroll
        for (int jt = 0; jt < 2; ++jt)
#pragma unroll
            for (int ks = 0; ks < 2; ++ks) o = mfma16(acc_frag(s[jt], ks), kp[jt][ks], o);   // dS K   (rows = queries, lanes = channels)
#pragma unroll
        for (int r = 0; r < 16; ++r) dq[r] += o[r] * a.scale;             // the members in the order m = 0 .. r-1
        __builtin_amdgcn_sched_barrier(0);   // one member at a time: the next one's rows are not loaded over this one's live tiles
    }
    char* dqb = reinterpret_cast<char*>(a.dq + qw * WT * a.C + head * HD);
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const int i = 32 * it + (r & 3) + 8 * (r >> 2) + 4 * h;           // (the tile is a run-time value here: no static padding skip)
        if (i < WT) *reinterpret_cast<float*>(dqb + ((uint32_t)i * rq + 4u * c)) = dq[r];
    }
}

template <bool GROUPED>
__global__ __launch_bounds__(256, 2) void deform_attn_bwd_kv_bf16mm_kernel(CrossBwd16Args<GROUPED> a) {
    __shared__ __attribute__((aligned(16))) uint32_t row_q[4][64];
    __shared__ __attribute__((aligned(16))) uint32_t row_k[4][64];
    __shared__ __attribute__((aligned(16))) float stat_s[4][192];         // the unit's {m, 1/l, D}: one coalesced read, then 16-byte LDS reads
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int c = lane & 31, h = lane >> 5;
    const int64_t u = (int64_t)blockIdx.x * 4 + wave;
    if (u >= a.units_kv) return;
    const int head = (int)(u % a.nH);
    const int64_t b2 = u / a.nH;
    const int64_t qw = cva_q_window(b2, a.pair), b1 = b2 / a.r;
    const uint32_t rq = 4u * a.C, rk = 8u * a.C;
    uint32_t* tq = row_q[wave];
    uint32_t* tk = row_k[wave];
    float* st = stat_s[wave];
    {
        const uint32_t slot = (uint32_t)(lane < WT ? lane : WT - 1);
        tq[lane] = slot * rq;
        tk[lane] = slot * rk;
        // query slots 49..63 were never written by the q kernel: finite filler (their P / dS are forced to 0 below)
        const float* sg = a.stats + u * 192;
#pragma unroll
        for (int k = 0; k < 3; ++k) st[64 * k + lane] = lane < WT ? sg[64 * k + lane] : 0.f;
    }
    __builtin_amdgcn_wave_barrier();
    const char* qb = reinterpret_cast<const char*>(a.q + qw * WT * a.C + head * HD);
    const char* kb = reinterpret_cast<const char*>(a.kv + b2 * WT * 2 * a.C + head * HD);
    const char* vb = kb + 4 * a.C;
    const char* dob = reinterpret_cast<const char*>(a.dout + b1 * WT * a.C + head * HD);
    bf16x8 qf[2][2], kf[2][2], vkf[2][2], dof[2][2];                      // [tile][k-step]
    bf16x8 qp[2][2], dop[2][2];                                           // q / dO in the permuted query order of the P / dS operand
#pragma unroll
    for (int t = 0; t < 2; ++t) {
        load_frag_bf16(qf[t], qb, tq[32 * t + c] + 32u * h);
        load_frag_bf16(kf[t], kb, tk[32 * t + c] + 32u * h);
    }
    __builtin_amdgcn_sched_barrier(0);   // fp32 rows are twice their fragments: a batch is rounded before the next is issued
#pragma unroll
    for (int t = 0; t < 2; ++t) {
        load_frag_bf16(vkf[t], vb, tk[32 * t + c] + 32u * h);
        load_frag_bf16(dof[t], dob, tq[32 * t + c] + 32u * h);
    }
    __builtin_amdgcn_sched_barrier(0);
    load_perm_bf16(qp, qb, tq, c, h);
    load_perm_bf16(dop, dob, tq, c, h);
    __builtin_amdgcn_sched_barrier(0);
    char* dkb = reinterpret_cast<char*>(a.dkv + b2 * WT * 2 * a.C + head * HD);
    char* dvb = dkb + 4 * a.C;
#pragma unroll
    for (int jt = 0; jt < 2; ++jt) {
        const int kj = 32 * jt + c;                                       // lane = key 32jt+c, accumulator rows = queries
        f32x16 ov = {}, ok = {};
        // one query tile at a time, straight into dV / dK: S and dP of one tile are live (32 registers), not of both
#pragma unroll
        for (int it = 0; it < 2; ++it) {
            f32x16 s = {}, dp = {};
#pragma unroll
            for (int ks = 0; ks < 2; ++ks) {
                s = mfma16(qf[it][ks], kf[jt][ks], s);                    // S = Q K^T   (A = q rows, B = k rows)
                dp = mfma16(dof[it][ks], vkf[jt][ks], dp);                // dP = dO V^T
            }
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                if (it == 1 && g == 3) {                                  // queries 56..63: padding
#pragma unroll
                    for (int e = 0; e < 4; ++e) { s[4 * g + e] = 0.f; dp[4 * g + e] = 0.f; }
                    continue;
                }
                const int i0 = 32 * it + 8 * g + 4 * h;                   // this lane's 4 consecutive queries i0 .. i0+3
                const f32x4 mv = *reinterpret_cast<const f32x4*>(st + i0);
                const f32x4 iv = *reinterpret_cast<const f32x4*>(st + 64 + i0);
                const f32x4 dv = *reinterpret_cast<const f32x4*>(st + 128 + i0);
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const bool valid = (i0 + e < WT) && (kj < WT);
                    const float pr = valid ? __expf(s[4 * g + e] * a.scale - mv[e]) * iv[e] : 0.f;   // the operation order of bias_softmax
                    s[4 * g + e] = pr;                                                     // P
                    dp[4 * g + e] = valid ? pr * (dp[4 * g + e] - dv[e]) : 0.f;            // dS
                }
            }
#pragma unroll
            for (int ks = 0; ks < 2; ++ks) {
                ov = mfma16(acc_frag(s, ks), dop[it][ks], ov);            // dV = P^T dO   (sum over all 64 query slots)
                ok = mfma16(acc_frag(dp, ks), qp[it][ks], ok);            // dK = dS^T Q
            }
            __builtin_amdgcn_sched_barrier(0);   // the tiles one after the other: interleaved, their accumulators are all live at once
        }
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            if (acc_pad(jt, g)) continue;
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                if (acc_pad(jt, g, e)) continue;
                const int j = acc_row(jt, g, e, h);
                if (j < WT) {
                    *reinterpret_cast<float*>(dvb + ((uint32_t)j * rk + 4u * c)) = ov[4 * g + e];
                    *reinterpret_cast<float*>(dkb + ((uint32_t)j * rk + 4u * c)) = ok[4 * g + e] * a.scale;
                }
            }
        }
        __builtin_amdgcn_sched_barrier(0);
    }
}

}  // namespace

// Which form a launch of the fp32 forward takes: bit 0 = split (win_attn_cross_kernel<true>: one unit on two waves), bit 1 = ring
// (never set here: the name of the bit in mumpy_window_attention_plan).  A pure function of the unit count: split while `units` is
// at most CROSS_SPLIT_UNITS (the fitted rule and its table are in the file header).  MUMPY_CVA_SPLIT_UNITS moves the threshold in
// the tuning build; it is read per launch there so that tools/kernel_micro.py can time both forms in one process.
constexpr int CROSS_SPLIT_UNITS = 1024;
static int cross_plan(int64_t units) { return units <= tune_int("MUMPY_CVA_SPLIT_UNITS", CROSS_SPLIT_UNITS) ? 1 : 0; }

extern "C" int mumpy_deform_attention_plan(int B, int H, int W, int C, int r) {
    MUMPY_REQUIRE(B > 0 && H > 0 && W > 0 && H % WS == 0 && W % WS == 0 && r >= 1 && C > 0 && C % HD == 0, MUMPY_EINVAL,
                  "deform_attention_plan: bad shape (%d,%d,%d,%d) or ratio %d", B, H, W, C, r);
    return cross_plan((int64_t)B * (H / WS) * (W / WS) * (C / HD));
}

// one validation + launch body for the forward kernels; `who` names the entry in mumpy_last_error.  GROUPED is chosen by the
// caller below from groups > 1; the plan (cross_plan) is a function of the unit count alone, so it holds for every grouping.
template <bool MM16, bool GROUPED>
static int cross_launch(const char* who, const float* q, const float* kv, const float* padmask, float* out, int B, int H, int W, int C,
                        int r, float scale, int groups, void* stream) {
    MUMPY_REQUIRE(q && kv && padmask && out, MUMPY_ENULL, "%s: null pointer", who);
    MUMPY_REQUIRE(aligned16(q) && aligned16(kv) && aligned16(padmask) && aligned16(out), MUMPY_EALIGN,
                  "%s: pointers must be 16-byte aligned", who);
    MUMPY_REQUIRE(B > 0 && H > 0 && W > 0 && H % WS == 0 && W % WS == 0 && r >= 1, MUMPY_EINVAL,
                  "%s: bad grid (%d,%d) or ratio %d", who, H, W, r);
    MUMPY_REQUIRE(C > 0 && C % HD == 0, MUMPY_EINVAL, "%s: C=%d not a multiple of 32", who, C);
    CrossArgs<GROUPED> a;
    a.q = q; a.kv = kv; a.padmask = padmask; a.out = out;
    a.B = B; a.H = H; a.W = W; a.C = C; a.nH = C / HD; a.r = r;
    a.nWx = W / WS; a.nWf = (H / WS) * (W / WS); a.scale = scale;
    const int64_t B1w = (int64_t)B * a.nWf;
    if constexpr (GROUPED) {
        const int bad = cva_grouping(who, B1w * r, B1w, B, groups, &a.pair);
        if (bad) return bad;
    } else {
        a.pair.nq = (int)B1w;
    }
    a.units = (int64_t)a.pair.nq * a.nH;
    const int64_t grid = (a.units + 3) / 4;
    MUMPY_REQUIRE(grid < (1ll << 31), MUMPY_ERANGE, "%s: too many windows", who);
    if (MM16) {
        MUMPY_REQUIRE((int64_t)H * W * C * 4 < (1ll << 32), MUMPY_ERANGE, "%s: image too large for 32-bit row offsets", who);
        hipLaunchKernelGGL(win_attn_cross_mm16_kernel<GROUPED>, dim3((unsigned)grid), dim3(256), 0, as_stream(stream), a);
    } else {
        if (cross_plan(a.units) & 1)
            hipLaunchKernelGGL((win_attn_cross_kernel<true, GROUPED>), dim3((unsigned)((a.units + 1) / 2)), dim3(256), 0,
                               as_stream(stream), a);
        else
            hipLaunchKernelGGL((win_attn_cross_kernel<false, GROUPED>), dim3((unsigned)grid), dim3(256), 0, as_stream(stream), a);
    }
    MUMPY_CHECK_LAUNCH(who);
    return 0;
}

extern "C" int mumpy_deform_attention_fwd(const float* q, const float* kv, const float* padmask, float* out, int B,
                                          int H, int W, int C, int r, float scale, void* stream) {
    return cross_launch<false, false>("deform_attention", q, kv, padmask, out, B, H, W, C, r, scale, 1, stream);
}

extern "C" int mumpy_deform_attention_mm16_fwd(const float* q, const float* kv, const float* padmask, float* out, int B,
                                               int H, int W, int C, int r, float scale, void* stream) {
    return cross_launch<true, false>("deform_attention_mm16", q, kv, padmask, out, B, H, W, C, r, scale, 1, stream);
}

// include/mumpy_hip_ext8.h: groups == 1 is the frozen entry's launch, after the grouped entry's own refusals
extern "C" int mumpy_deform_attention_grouped_fwd(const float* q, const float* kv, const float* padmask, float* out, int B, int H,
                                                  int W, int C, int r, float scale, int groups, void* stream) {
    const char* who = "deform_attention_grouped";
    MUMPY_REQUIRE(groups >= 1, MUMPY_EINVAL, "%s: groups=%d must be at least 1", who, groups);
    if (groups == 1) return cross_launch<false, false>(who, q, kv, padmask, out, B, H, W, C, r, scale, 1, stream);
    return cross_launch<false, true>(who, q, kv, padmask, out, B, H, W, C, r, scale, groups, stream);
}

extern "C" int mumpy_deform_attention_mm16_grouped_fwd(const float* q, const float* kv, const float* padmask, float* out, int B,
                                                       int H, int W, int C, int r, float scale, int groups, void* stream) {
    const char* who = "deform_attention_mm16_grouped";
    MUMPY_REQUIRE(groups >= 1, MUMPY_EINVAL, "%s: groups=%d must be at least 1", who, groups);
    if (groups == 1) return cross_launch<true, false>(who, q, kv, padmask, out, B, H, W, C, r, scale, 1, stream);
    return cross_launch<true, true>(who, q, kv, padmask, out, B, H, W, C, r, scale, groups, stream);
}

extern "C" int64_t mumpy_deform_attention_bwd_workspace_bytes(int64_t B2w, int C) {
    return (B2w <= 0 || C <= 0) ? 0 : B2w * (C / HD) * 192 * (int64_t)sizeof(float);
}

// one validation + launch body for the frozen entry (groups = 1: the <GROUPED = false> kernels, no refusal added) and the grouped one
template <bool GROUPED>
static int cross_bwd_launch(const char* who, const float* q, const float* kv, const float* dout, float* dq_part, float* dkv,
                            void* workspace, int64_t workspace_bytes, int64_t B1w, int r, int C, float scale, int groups,
                            void* stream) {
    MUMPY_REQUIRE(q && kv && dout && dq_part && dkv && workspace, MUMPY_ENULL, "%s: null pointer", who);
    MUMPY_REQUIRE(aligned16(q) && aligned16(kv) && aligned16(dout) && aligned16(dq_part) && aligned16(dkv) && aligned16(workspace),
                  MUMPY_EALIGN, "%s: pointers must be 16-byte aligned", who);
    MUMPY_REQUIRE(B1w > 0 && r >= 1 && C > 0 && C % HD == 0, MUMPY_EINVAL, "%s: bad shape", who);
    const int64_t B2w = B1w * r;
    MUMPY_REQUIRE(workspace_bytes >= mumpy_deform_attention_bwd_workspace_bytes(B2w, C), MUMPY_EINVAL, "%s: workspace too small", who);
    CrossBwdArgs<GROUPED> a;
    a.q = q; a.kv = kv; a.dout = dout; a.dq_part = dq_part; a.dkv = dkv; a.stats = static_cast<float*>(workspace);
    a.C = C; a.nH = C / HD; a.r = r; a.scale = scale; a.units = B2w * a.nH;
    const int64_t grid = (a.units + 3) / 4;
    MUMPY_REQUIRE(grid < (1ll << 31) && B1w < (1ll << 31), MUMPY_ERANGE, "%s: too many windows", who);
    if constexpr (GROUPED) {
        const int bad = cva_grouping_windows(who, B2w, B1w, groups, &a.pair);
        if (bad) return bad;
    } else {
        a.pair.nq = (int)B1w;
    }
    hipLaunchKernelGGL(deform_attn_bwd_q_kernel<GROUPED>, dim3((unsigned)grid), dim3(256), 0, as_stream(stream), a);
    MUMPY_CHECK_LAUNCH(who);
    hipLaunchKernelGGL(deform_attn_bwd_kv_kernel<GROUPED>, dim3((unsigned)grid), dim3(256), 0, as_stream(stream), a);
    MUMPY_CHECK_LAUNCH(who);
    return 0;
}

extern "C" int mumpy_deform_attention_bwd(const float* q, const float* kv, const float* dout, float* dq_part, float* dkv,
                                          void* workspace, int64_t workspace_bytes, int64_t B1w, int r, int C, float scale,
                                          void* stream) {
    return cross_bwd_launch<false>("deform_attention_bwd", q, kv, dout, dq_part, dkv, workspace, workspace_bytes, B1w, r, C, scale, 1,
                                   stream);
}

// include/mumpy_hip_ext9.h: groups == 1 is the frozen entry's launch, after the grouped entry's own refusals
extern "C" int mumpy_deform_attention_grouped_bwd(const float* q, const float* kv, const float* dout, float* dq_part, float* dkv,
                                                  void* workspace, int64_t workspace_bytes, int64_t B1w, int r, int C, float scale,
                                                  int groups, void* stream) {
    const char* who = "deform_attention_grouped_bwd";
    MUMPY_REQUIRE(groups >= 1, MUMPY_EINVAL, "%s: groups=%d must be at least 1", who, groups);
    if (groups == 1)
        return cross_bwd_launch<false>(who, q, kv, dout, dq_part, dkv, workspace, workspace_bytes, B1w, r, C, scale, 1, stream);
    return cross_bwd_launch<true>(who, q, kv, dout, dq_part, dkv, workspace, workspace_bytes, B1w, r, C, scale, groups, stream);
}

// ---- include/mumpy_hip_ext2.h ----
// 0 when (B1w, r, C) is a shape mumpy_deform_attention_mm16_bwd takes, else the code it refuses it with.  The range limits: the grids
// (B1w r C/32 kv units, 2 B1w C/32 q units, four to a block) and the 32-bit byte offset of a row inside a kv window (49 rows of 8C bytes).
static int mm16_bwd_shape(int64_t B1w, int r, int C) {
    if (!(B1w > 0 && r >= 1 && C > 0 && C % HD == 0)) return MUMPY_EINVAL;
    if (B1w >= (1ll << 31) || B1w * r >= (1ll << 31)) return MUMPY_ERANGE;
    const int64_t nH = C / HD;
    if ((B1w * r * nH + 3) / 4 >= (1ll << 31) || (B1w * nH * 2 + 3) / 4 >= (1ll << 31)) return MUMPY_ERANGE;
    if ((int64_t)WT * 2 * C * 4 >= (1ll << 32)) return MUMPY_ERANGE;
    return 0;
}

extern "C" int64_t mumpy_deform_attention_mm16_bwd_workspace_bytes(int64_t B1w, int r, int C) {
    return mm16_bwd_shape(B1w, r, C) ? 0 : B1w * r * (C / HD) * 192 * (int64_t)sizeof(float);
}

template <bool GROUPED>
static int cross_bwd16_launch(const char* who, const float* q, const float* kv, const float* dout, float* dq, float* dkv,
                              void* workspace, int64_t workspace_bytes, int64_t B1w, int r, int C, float scale, int groups,
                              void* stream) {
    MUMPY_REQUIRE(q && kv && dout && dq && dkv && workspace, MUMPY_ENULL, "%s: null pointer", who);
    MUMPY_REQUIRE(aligned16(q) && aligned16(kv) && aligned16(dout) && aligned16(dq) && aligned16(dkv) && aligned16(workspace),
                  MUMPY_EALIGN, "%s: pointers must be 16-byte aligned", who);
    const int bad = mm16_bwd_shape(B1w, r, C);
    MUMPY_REQUIRE(bad != MUMPY_EINVAL, MUMPY_EINVAL, "%s: bad shape (B1w=%lld, r=%d, C=%d)", who, (long long)B1w, r, C);
    MUMPY_REQUIRE(bad == 0, MUMPY_ERANGE, "%s: too many windows or C=%d too wide for 32-bit row offsets", who, C);
    MUMPY_REQUIRE(workspace_bytes >= mumpy_deform_attention_mm16_bwd_workspace_bytes(B1w, r, C), MUMPY_EINVAL,
                  "%s: workspace too small", who);
    CrossBwd16Args<GROUPED> a;
    a.q = q; a.kv = kv; a.dout = dout; a.dq = dq; a.dkv = dkv; a.stats = static_cast<float*>(workspace);
    a.C = C; a.nH = C / HD; a.r = r; a.scale = scale;
    a.units_q = B1w * a.nH * 2; a.units_kv = B1w * r * a.nH;
    if constexpr (GROUPED) {
        const int badg = cva_grouping_windows(who, B1w * r, B1w, groups, &a.pair);
        if (badg) return badg;
    } else {
        a.pair.nq = (int)B1w;
    }
    hipLaunchKernelGGL(deform_attn_bwd_q_bf16mm_kernel<GROUPED>, dim3((unsigned)((a.units_q + 3) / 4)), dim3(256), 0, as_stream(stream), a);
    MUMPY_CHECK_LAUNCH(who);
    hipLaunchKernelGGL(deform_attn_bwd_kv_bf16mm_kernel<GROUPED>, dim3((unsigned)((a.units_kv + 3) / 4)), dim3(256), 0, as_stream(stream), a);
    MUMPY_CHECK_LAUNCH(who);
    return 0;
}

extern "C" int mumpy_deform_attention_mm16_bwd(const float* q, const float* kv, const float* dout, float* dq, float* dkv,
                                               void* workspace, int64_t workspace_bytes, int64_t B1w, int r, int C, float scale,
                                               void* stream) {
    return cross_bwd16_launch<false>("deform_attention_mm16_bwd", q, kv, dout, dq, dkv, workspace, workspace_bytes, B1w, r, C, scale, 1,
                                     stream);
}

// ---- include/mumpy_hip_ext9.h ----
extern "C" int mumpy_deform_attention_mm16_grouped_bwd(const float* q, const float* kv, const float* dout, float* dq, float* dkv,
                                                       void* workspace, int64_t workspace_bytes, int64_t B1w, int r, int C,
                                                       float scale, int groups, void* stream) {
    const char* who = "deform_attention_mm16_grouped_bwd";
    MUMPY_REQUIRE(groups >= 1, MUMPY_EINVAL, "%s: groups=%d must be at least 1", who, groups);
    if (groups == 1)
        return cross_bwd16_launch<false>(who, q, kv, dout, dq, dkv, workspace, workspace_bytes, B1w, r, C, scale, 1, stream);
    return cross_bwd16_launch<true>(who, q, kv, dout, dq, dkv, workspace, workspace_bytes, B1w, r, C, scale, groups, stream);
}
