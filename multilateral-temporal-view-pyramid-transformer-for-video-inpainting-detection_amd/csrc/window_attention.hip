// window_attention.hip — forward of the Swin window attention core (self-attention), one (window, head) unit per wave,
// everything in registers: win_attn_self_kernel (fp32 MFMA; fp32 or bf16 storage; the LDS-free "background" form),
// win_attn_self_split_kernel (the same unit on two waves, for grids too small to fill the chip), win_attn_self_bf16mm_kernel (bf16 MFMA; bf16 or fp32 storage), the relative-position bias expansion, their entry points.
// The unit's data flow and the helpers every attention kernel shares are in win_attn_unit.h; the backward is
// window_attention_bwd.hip, the deformable cross-view attention deform_attention.hip.
//
// Replaces: window_partition / roll / window_reverse (swin:54-83, 273, 295) + the softmax(QK^T + bias + mask)V core
// of WindowAttention.forward (swin:145-163).
//
// Resources (hipcc -Rpass-analysis=kernel-resource-usage, gfx950; VGPRs / SGPRs / scratch / LDS per block / waves per SIMD):
//   win_attn_self_kernel<DBG=0, IO16=0>         159 / 71 /   0 B / 15,376 B / 3
//   win_attn_self_kernel<DBG=0, IO16=1>         159 / 71 /   0 B / 15,376 B / 3
//   win_attn_self_kernel<DBG=0, IO16=0, NOLDS>  128 / 70 / 296 B /      0 B / 4
//   win_attn_self_kernel<DBG=1> (diagnostic)    166 / 81 /   0 B / 15,376 B / 3
//   win_attn_self_split_kernel                  136 / 46 /   0 B /  2,048 B / 3   (no spills)
//   win_attn_self_bf16mm_kernel<IO32=0>         134 / 71 /   0 B / 16,400 B / 3
//   win_attn_self_bf16mm_kernel<IO32=1>         146 / 68 /   0 B / 16,400 B / 3
// No AGPRs anywhere.
//
// The unit is below the fp32 ridge (12.25 FLOP/B): no LDS staging, ~25 KB in flight per wave, 12 waves per CU.
// Measured on the largest launch of the B=8,T=5 forward (40 frames 56x56, C=128: 10,240 units, 257 MB of q/k/v/o;
// MUMPY_WA_DBG ablation, MI355X): 65.9 us = 30 % of the 157 TFLOP/s datasheet peak in useful 49x49 FLOPs, 46 % MFMA-busy
// by SQ_VALU_MFMA_BUSY_CYCLES (114 MFMAs per unit incl. the 49->64 padding; profiles/r01_pmc_mfma.md).  Floors: 41 us of
// HBM time at the 6.3 TB/s this part sustains, 38.5 us of MFMA issue at the 124 TFLOP/s a bare fp32 MFMA loop reaches.
// Ablation: loads only 33 us, MFMAs + softmax only 46 us (80 % of the practical MFMA rate), loads + stores 41 us.
// What moved it (79.8 -> 65.9 us):
//   * addressing: wave-uniform bases in SGPRs + pre-multiplied 32-bit byte offsets from the token tables; the pointer form
//     spent 66 v_mad_u64 + 130 v_mul_lo_u32 (quarter-rate) per unit, ~40 % of the MFMA time (79.8 -> 67.8 us);
//   * one branch per unit on the mask pointer (unmasked windows run branch-free, masked ones batch their loads), no
//     exp / max / scale work on the statically padded key slots (67.8 -> 65.9 us).
// Tried and measured, not kept: staggered block starts, s_setprio per resident block or around the MFMA phase (no
// change: a per-wave s_memtime trace shows the SIMD busy in some wave's compute phase ~all the time; the remaining gap
// is the memory phase of a unit not overlapping its own wave's compute); cross-unit REGISTER prefetch at 2 waves/SIMD
// (spills) and at 1 wave/SIMD (no overlap: hipcc's waitcnt insertion drains loop-carried prefetches); row-coalesced q/k
// address pattern (-5 %, needs an LDS transpose).
// Not built: K/V of the next unit through an LDS-DMA ring at 2 waves/SIMD.  It can only help launches in which a wave walks
// several units: since the split form below, those are the 10,240- and 5,120-unit launches, FOUR launches of the B=8, T=5
// forward (2 x 58 us + 2 x 32 us).  With the memory phase hidden completely (the 46 us "MFMAs + softmax only" ablation against
// 65.9 us: 30 %) that is at most ~0.05 ms of a 21.5 ms forward, below what the benchmark resolves (profiles/window_attention_overlap.md).
//
// Small grids: one unit on two waves (win_attn_self_split_kernel; mumpy_window_attention_plan bit 0).  Up to 2,560 units the
// persistent form gives every wave ONE unit (768 blocks x 4 waves hold 3,072), so the launch is one unit's dependent chain
// with the chip's waves in lockstep: everybody loads, then everybody computes.  The split form halves that chain (one 32-query
// tile per wave), drops the bias staging round trip ahead of it, and above 1,536 units runs as two rounds of blocks whose memory
// and compute phases overlap.  Bitwise the same output (tests/test_window_attention_schedule.py).
// Fitted rule (self_plan): split while units <= 2,560.  Both forms of every self-attention shape of the B=8, T=5 forward, timed on
// one MI355X against the parent commit's library (tools/kernel_micro.py winattn_ab: medians of 12 alternating replays of 20 captured
// launches, us per launch; "whole" = this file's persistent form; the parent's own repeats differ by <= 0.1 us, 1.1 us on the largest):
//   (B, Hs, W, C)      units   shift 0: parent  whole  split     shift 3: parent  whole  split     plan
//   (8, 280, 56, 128) 10,240            57.9   58.9   63.1                58.0   57.9   64.7      whole
//   (8, 140, 28, 256)  5,120            30.7   30.7   35.9                34.3   34.4   36.5      whole
//   (8,  70, 14, 512)  2,560            22.4   22.4   21.8                24.5   24.5   22.4      split
//   (8,  56, 56,  96)  1,536            15.6   15.6   13.4                16.9   17.0   13.9      split
//   (8,  35,  7, 1024) 1,280            14.7   14.7   12.7                 --                     split
//   (8,  28, 28, 192)    768             9.8    9.9    9.5                11.2   11.1   10.5      split
//   (8,  14, 14, 384)    384             9.2    9.1    6.8                10.3   10.4    7.1      split
//   (8,   7,  7, 768)    192             8.9    8.9    6.6                 --                     split
// The split form reads K and V twice (the second wave of a pair hits L2), which is what it loses on the two HBM-bound launches.
#include <stdlib.h>
#include "win_attn_unit.h"

namespace {

// DBG = false is the shipped instantiation: the MUMPY_WA_DBG ablation switches (skip loads / MFMAs / stores) exist only in
// the diagnostic instantiation, which the launcher selects when that variable is set.
// IO16: qkv and out are bf16 in memory (config 3's activation storage); the arithmetic is the same fp32 MFMA flow.
// NOLDS: the "background" instantiation (round 3, see gemm_rd.hip): no LDS allocation at all, so that the kernel can be resident on
// a CU whose whole LDS belongs to the persistent GEMM.  The per-wave token tables live in registers and are read through
// ds_bpermute (which uses the LDS crossbar but no LDS memory); the bias rows come from global memory / L1.  Slower per unit (the
// row-strided bias reads cost L1 tag cycles), used only for the small launches of views 1 / 2 that run beside view 3's GEMMs.
template <bool DBG, bool IO16 = false, bool NOLDS = false>
__global__ __launch_bounds__(256, (NOLDS ? 4 : 3)) void win_attn_self_kernel(SelfArgs a) {
    __shared__ uint32_t tok_in[4][64];    // token * (3C*4): byte offset of the token's qkv row
    __shared__ __attribute__((aligned(16))) uint32_t tok_out[4][64];   // token * (C*4):  byte offset of the token's out row
    __shared__ __attribute__((aligned(16))) float bias_s[WT * BLD];
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int c = lane & 31, h = lane >> 5;
    // a block = ONE head x 4 consecutive windows, so that the head's bias table is staged once (stage_bias); a (window, head) unit
    // owns its 128-B q/k/v row segments exclusively, so grouping by head costs no extra HBM or L2 traffic.
    const int head = blockIdx.x % a.nH;
    const int slot = blockIdx.x / a.nH;
    const int64_t nwin = (int64_t)a.B * a.nW;
    if (!NOLDS) stage_bias(bias_s, a.bias, head);
    // staggered block starts (MUMPY_WA_STAGGER, tuning build; "tried and measured, not kept" above: 0 trips in every shipped build).  The
    // loop stays: without it <NOLDS> is allocated 344 B of scratch instead of 296 (profiles/window_attention_refactor.md, section 1).
    for (int d = 0; d < (slot % 3) * a.stagger; ++d) __builtin_amdgcn_s_sleep(127);
    const int64_t L = (int64_t)a.Hs * a.W;
    const uint32_t rsb = (IO16 ? 6u : 12u) * a.C, rob = (IO16 ? 2u : 4u) * a.C;                      // row strides in bytes
    uint32_t* ti = NOLDS ? nullptr : tok_in[wave];
    uint32_t* to = NOLDS ? nullptr : tok_out[wave];
    uint32_t ti_reg = 0, to_reg = 0;                 // NOLDS: lane l holds table entry l
    auto TI = [&](int i) -> uint32_t { return NOLDS ? (uint32_t)__shfl((int)ti_reg, i) : ti[i]; };
    auto TO = [&](int i) -> uint32_t { return NOLDS ? (uint32_t)__shfl((int)to_reg, i) : to[i]; };
    for (int64_t bw = (int64_t)slot * 4 + wave; bw < nwin; bw += (int64_t)a.groups * 4) {   // all scalar
    int64_t b;
    if (NOLDS) {
        uint32_t tok;
        b = unit_token(a, bw, lane, tok);
        ti_reg = tok * rsb; to_reg = tok * rob;
        __builtin_amdgcn_wave_barrier();
    } else b = unit_tokens(a, bw, lane, rsb, rob, ti, to);
    const char* base = IO16 ? reinterpret_cast<const char*>(reinterpret_cast<const __bf16*>(a.qkv) + b * L * 3 * a.C + head * HD)
                            : reinterpret_cast<const char*>(a.qkv + b * L * 3 * a.C + head * HD);

    // q/k/v go straight to registers (MFMA operand layout); branch-free
    f32x4 qf[2][4], kf[2][4];
    float vf[2][16];
    const int dbg = DBG ? a.dbg : 0;
    if (!(dbg & 1)) {
        if (IO16) {
            // a lane's 16 channels are 32 bytes: two 16-byte loads of 8 bf16, widened to fp32 by a shift
            typedef uint32_t u32x4v __attribute__((ext_vector_type(4)));
            auto widen = [](u32x4v w, f32x4& lo, f32x4& hi) {
                lo = f32x4{__uint_as_float(w.x << 16), __uint_as_float(w.x & 0xffff0000u), __uint_as_float(w.y << 16), __uint_as_float(w.y & 0xffff0000u)};
                hi = f32x4{__uint_as_float(w.z << 16), __uint_as_float(w.z & 0xffff0000u), __uint_as_float(w.w << 16), __uint_as_float(w.w & 0xffff0000u)};
            };
            const char* kbase = base + 2 * a.C;
#pragma unroll
            for (int t = 0; t < 2; ++t) {
                const uint32_t off = TI(32 * t + c) + 32u * h;
#pragma unroll
                for (int i = 0; i < 2; ++i) {
                    widen(*reinterpret_cast<const u32x4v*>(base + (off + 16u * i)), qf[t][2 * i], qf[t][2 * i + 1]);
                    widen(*reinterpret_cast<const u32x4v*>(kbase + (off + 16u * i)), kf[t][2 * i], kf[t][2 * i + 1]);
                }
            }
            const char* vbase = base + 4 * a.C;
            for_pv_steps([&](int jt, int g, int e) {
                const uint32_t w = *reinterpret_cast<const uint16_t*>(vbase + (TI(32 * jt + 8 * g + 4 * h + e) + 2u * c));
                vf[jt][4 * g + e] = __uint_as_float(w << 16);
            });
        } else {
        const char* kbase = base + 4 * a.C;
#pragma unroll
        for (int t = 0; t < 2; ++t) {
            const uint32_t off = TI(32 * t + c) + 64u * h;
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                qf[t][i] = *at16(base, off + 16u * i);
                kf[t][i] = *at16(kbase, off + 16u * i);
            }
        }
        const char* vbase = base + 8 * a.C;
        for_pv_steps([&](int jt, int g, int e) {
            vf[jt][4 * g + e] = *reinterpret_cast<const float*>(vbase + (TI(32 * jt + 8 * g + 4 * h + e) + 4u * c));
        });
        }
    } else {
#pragma unroll
        for (int t = 0; t < 2; ++t) { load_frag(qf[t], a.qkv, false); load_frag(kf[t], a.qkv, false); }
        for_pv_steps([&](int jt, int g, int e) { vf[jt][4 * g + e] = 1.f; });
    }
#pragma unroll
    for (int t = 0; t < 2; ++t)
#pragma unroll
        for (int i = 0; i < 4; ++i) qf[t][i] *= a.scale;   // q = q * scale before QK^T (swin:145)

    const float* mask_w = nullptr;                 // unit_mask(a, bw), spelled out: the call permutes the V registers of <DBG = true>
    if (a.mask_id) {
        const int id = a.mask_id[bw % a.n_mask];   // scalar load
        if (id >= 0) mask_w = a.mask_tab + (int64_t)id * 4096;
    }
    char* obase = IO16 ? reinterpret_cast<char*>(reinterpret_cast<__bf16*>(a.out) + b * L * a.C + head * HD)
                       : reinterpret_cast<char*>(a.out + b * L * a.C + head * HD);
    // the two 32-query tiles go one after the other: S needs 32 accumulator registers instead of 64
    auto tiles = [&](auto masked) {
        constexpr bool MASKED = decltype(masked)::value;
#pragma unroll
        for (int it = 0; it < 2; ++it) {
            f32x16 s[2];                           // element by element, not "= {}": that form costs this kernel 9 VGPRs and 8 B of scratch
#pragma unroll
            for (int jt = 0; jt < 2; ++jt)
#pragma unroll
                for (int r = 0; r < 16; ++r) s[jt][r] = 0.f;
            if (!(dbg & 2)) qk_product(s, kf, qf[it]);
            else { s[0][0] = kf[0][0][0] + qf[it][0][0]; s[1][3] = kf[1][1][1] * qf[it][2][1]; }
            const int qi = 32 * it + c;
            if (!(dbg & 2))
                bias_softmax<MASKED>(s, NOLDS ? bias_row(a.bias + (int64_t)head * 4096, 64, qi, h) : bias_row(bias_s, BLD, qi, h),
                                     mask_w, qi, h, 1.0f);
            f32x16 o = {};
            if (!(dbg & 2)) pv_product(o, s, vf);
            else { o[0] = s[0][0] + vf[0][0]; o[5] = s[1][2] * vf[1][8]; }
            if (!(dbg & 4)) {
                // row offsets of the 4 consecutive queries a lane's register group g holds: one 16-byte table read
                typedef uint32_t u32x4v __attribute__((ext_vector_type(4)));
                u32x4v to4[4];
#pragma unroll
                for (int g = 0; g < 4; ++g)
                    if (!acc_pad(it, g)) {
                        if (NOLDS) {
#pragma unroll
                            for (int e = 0; e < 4; ++e) to4[g][e] = TO(32 * it + 8 * g + 4 * h + e);
                        } else {
                            to4[g] = *reinterpret_cast<const u32x4v*>(&to[32 * it + 8 * g + 4 * h]);
                        }
                    }
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    if (!acc_live(it, r)) continue;
                    const int i = acc_row(it, r, h);
                    if (i < WT) {
                        if (IO16) *reinterpret_cast<__bf16*>(obase + (to4[r >> 2][r & 3] + 2u * c)) = (__bf16)o[r];
                        else *reinterpret_cast<float*>(obase + (to4[r >> 2][r & 3] + 4u * c)) = o[r];
                    }
                }
            } else if (o[0] == 1234.5f && o[5] == 77.f) obase[0] = 1;
        }
    };
    if (mask_w) tiles(std::true_type{}); else tiles(std::false_type{});
    __builtin_amdgcn_wave_barrier();   // the token tables are rewritten by the next unit
    }
}

// ---------------------------------------------------------------------------------------------------------------
// Small grids (window_attention_split): ONE unit on TWO waves, split by query tile.  A launch of a few hundred units leaves most
// of the chip idle while each wave walks its unit's dependent chain alone (bias staging + block barrier, token table, loads,
// 2 x (32 + 25 MFMAs around a softmax), stores).  The two 32-query tiles of a unit share only K and V, so here wave 2p + it of
// a block takes tile `it` of the block's window p: it loads all of K and V (the second reader hits L2), its own 32 queries, and
// runs ONE qk_product / bias_softmax / pv_product.  A block is one head x 2 windows and is not persistent (one unit pair per
// block, at most 1,280 blocks: see the fitted rule in the file header).  The bias row of the lane's query comes
// straight from the global table, issued with the q/k/v loads: one round trip instead of the staged table's load -> LDS ->
// block barrier ahead of them (the L1 tag cycles that made the row-strided reads slow in a streaming launch do not matter
// on a single unit's chain).
// Every value is computed by the same instructions in the same order as in win_attn_self_kernel (the MFMA k order, q * scale,
// s + bias (+ mask), max / exp / sum / normalise over the same registers, the cross-half exchanges), so outputs are bitwise
// those of the one-wave form.  fp32 storage and math only.
__global__ __launch_bounds__(256, 2) void win_attn_self_split_kernel(SelfArgs a) {
    __shared__ __attribute__((aligned(16))) uint32_t tok_in[4][64];
    __shared__ __attribute__((aligned(16))) uint32_t tok_out[4][64];
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int c = lane & 31, h = lane >> 5;
    const int head = blockIdx.x % a.nH;
    const int it = wave & 1;                                             // this wave's query tile
    const int64_t bw = (int64_t)(blockIdx.x / a.nH) * 2 + (wave >> 1);
    if (bw >= (int64_t)a.B * a.nW) return;                               // odd window count: no block barrier below
    const int64_t L = (int64_t)a.Hs * a.W;
    uint32_t* ti = tok_in[wave];
    uint32_t* to = tok_out[wave];
    const int64_t b = unit_tokens(a, bw, lane, 12u * a.C, 4u * a.C, ti, to);
    const char* base = reinterpret_cast<const char*>(a.qkv + b * L * 3 * a.C + head * HD);
    const char* kbase = base + 4 * a.C;
    const char* vbase = base + 8 * a.C;
    const int qi = 32 * it + c;

    f32x4 qf[4], kf[2][4], bq[2][4];
    float vf[2][16];
    const uint32_t qoff = ti[qi] + 64u * h;
#pragma unroll
    for (int i = 0; i < 4; ++i) qf[i] = *at16(base, qoff + 16u * i);
#pragma unroll
    for (int t = 0; t < 2; ++t) {
        const uint32_t off = ti[32 * t + c] + 64u * h;
#pragma unroll
        for (int i = 0; i < 4; ++i) kf[t][i] = *at16(kbase, off + 16u * i);
    }
    for_pv_steps([&](int jt, int g, int e) {
        vf[jt][4 * g + e] = *reinterpret_cast<const float*>(vbase + (ti[32 * jt + 8 * g + 4 * h + e] + 4u * c));
    });
    const float* brow = a.bias + (int64_t)head * 4096 + (qi < WT ? qi : WT - 1) * 64 + 4 * h;   // as bias_row: padded queries re-read row 48
#pragma unroll
    for (int jt = 0; jt < 2; ++jt)
#pragma unroll
        for (int g = 0; g < 4; ++g)
            if (!(jt == 1 && g == 3)) bq[jt][g] = *reinterpret_cast<const f32x4*>(brow + 32 * jt + 8 * g);
#pragma unroll
    for (int i = 0; i < 4; ++i) qf[i] *= a.scale;                        // q = q * scale before QK^T (swin:145)

    const float* mask_w = unit_mask(a, bw);
    f32x16 s[2];
#pragma unroll
    for (int jt = 0; jt < 2; ++jt)
#pragma unroll
        for (int r = 0; r < 16; ++r) s[jt][r] = 0.f;
    qk_product(s, kf, qf);
    auto bias_at = [&](int jt, int g) { return pad_key52(bq[jt][g], jt, g, h); };
    if (mask_w) bias_softmax<true>(s, bias_at, mask_w, qi, h, 1.0f);
    else bias_softmax<false>(s, bias_at, mask_w, qi, h, 1.0f);
    f32x16 o = {};
    pv_product(o, s, vf);
    char* obase = reinterpret_cast<char*>(a.out + b * L * a.C + head * HD);
    auto orow = [&](int i) { return reinterpret_cast<float*>(obase + to[i]); };
    if (it == 0) store_o(o, 0, orow, c, h);
    else store_o(o, 1, orow, c, h);
}

// ---------------------------------------------------------------------------------------------------------------
// bf16-MFMA form of the self-attention unit for bf16-stored qkv (mumpy_window_attention_bf16mm_fwd; opt-in, see
// ops.set_attention_math): both products on v_mfma_f32_32x32x16_bf16 with fp32 accumulation, fp32 softmax.  Same unit
// structure as win_attn_self_kernel<.., IO16>: one (window, head) unit per wave, persistent blocks of one head x 4 windows, the
// head's bias table staged once in LDS, token tables, one branch per unit on the mask pointer.  What differs:
//   * S^T = K Q^T: a head row is 32 bf16 = 64 B and lane (r, h) needs channels 16s + 8h .. +7 of row r for k-step s: ONE 16-byte
//     load is the operand fragment, nothing is widened or converted.  2 key tiles x 2 query tiles x 2 k-steps = 8 MFMAs (fp32: 64).
//   * scale is NOT folded into q (32^-0.5 is no power of two: a second rounding of q): it multiplies the fp32 scores,
//     s * scale + bias (+ mask) -- this entry applies `scale` AFTER the product.
//   * P is rounded to bf16 UNNORMALISED: the operand of P V is e_j = exp(s_j - max_j s) (in (0, 1], the largest exactly 1); the row
//     sum is taken in fp32 over the unrounded e_j and its reciprocal scales the fp32 product before the output is rounded.
//   * O = P^T-as-A . V: the accumulator tile S^T (query on the lane, key in the 16 registers) is the A operand with no lane
//     movement (acc_frag; its k order is permuted), and the V fragment of lane (c, h) holds channel c of exactly those keys in that
//     order (2-byte gathers packed in pairs).  2 query tiles x 4 k-steps = 8 MFMAs (fp32: 50).
//     Key 48 is real (jt=1, s=1, j=0, h=0), so no k-step is dropped; keys >= 49 have e_j = 0 exactly and their V slots are slot 48's
//     value (token table clamp) or zero: finite.
//   * 1/sum lives on the query's LANE, O has the query in its REGISTERS: it crosses through 64 floats of LDS per wave (one
//     ds_write_b32, four ds_read_b128 per tile).
// Resources (hipcc -Rpass-analysis=kernel-resource-usage, gfx950): <IO32 = false> 134 VGPRs and 71 SGPRs, <IO32 = true> (the training
// tape) 146 VGPRs and 68 SGPRs; both 0 AGPRs, no scratch, no spills, 16,400 B of LDS per block, 3 waves per SIMD.  (A form with the mask row folded into the bias row fits 128 VGPRs = 4 waves per SIMD without spills and
// measured the same, 42.0 vs 41.3 us on the largest masked launch: the unit is not occupancy-bound, so the simpler form stays.)
// Measured against the fp32-flow kernel on the same bf16 input (tools/kernel_micro.py winattn16; profiles/bf16mm_window_attention.md):
//   (B, Hs, W, C)       shift 0: fp32 flow -> bf16 MFMA      shift 3: fp32 flow -> bf16 MFMA     [us per launch, MI355X, medians of 12 x 20
//   (8, 280, 56, 128)     59.3 -> 38.9  (1.52x, 3.3 TB/s)      59.4 -> 41.5  (1.43x)               alternating launches; every shape of the
//   (8, 140, 28, 256)     31.9 -> 21.6  (1.48x)                34.8 -> 23.7  (1.47x)               B=8, T=5 bf16-storage forward]
//   (8,  70, 14, 512)     23.0 -> 14.4  (1.59x)                24.5 -> 16.0  (1.54x)
//   (8,  56, 56,  96)     15.3 -> 10.4  (1.48x)                16.3 -> 10.7  (1.53x)
//   (8,  35,  7, 1024)    14.3 -> 10.4  (1.37x)                 --
//   (8,  28, 28, 192)     10.5 -> 10.5                         12.0 -> 12.1   } at ~10 us a launch in an eager loop these are paced by the
//   (8,  14, 14, 384)     10.5 -> 10.0                         10.6 -> 10.6   } launch rate, not by the kernel: equal within the spread
//   (8,   7,  7, 768)     10.0 -> 10.2                          --            } (+-0.5 us)
// In the forward (rocprofv3 --kernel-trace, 60 launches): 18.4 -> 12.1 us average, 1.10 -> 0.72 ms per forward.  The largest launch moves
// 128 MB in 38.9 us = 3.3 TB/s, half of what HBM sustains: MFMA time is gone (16 MFMAs per unit) and what remains is the issue of ~100
// narrow memory instructions per unit (25 2-byte V gathers, 50 2-byte row-strided stores).  Neither 4 waves per SIMD nor the persistent
// block count (512 .. 2560, MUMPY_WA16_BLOCKS in the tuning build) moves it.  Next step: V and O through an LDS transpose, 16-byte accesses.
// IO32: qkv and out are fp32 in memory (the training tape, mumpy_window_attention_mm16_fwd): operands are rounded to bf16 in registers,
// everything after the load and before the store is the same instruction stream, so the tape's forward has the P its backward rebuilds.
template <bool IO32>
__global__ __launch_bounds__(256, 3) void win_attn_self_bf16mm_kernel(SelfArgs a) {
    __shared__ __attribute__((aligned(16))) uint32_t tok_in[4][64];    // token * (3C * esize): byte offset of the token's qkv row
    __shared__ __attribute__((aligned(16))) uint32_t tok_out[4][64];   // token * (C * esize):  byte offset of the token's out row
    __shared__ __attribute__((aligned(16))) float inv_s[4][64];        // 1 / row sum of the unit's 64 query slots
    __shared__ __attribute__((aligned(16))) float bias_s[WT * BLD];
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int c = lane & 31, h = lane >> 5;
    const int head = blockIdx.x % a.nH;
    const int slot = blockIdx.x / a.nH;
    const int64_t nwin = (int64_t)a.B * a.nW;
    stage_bias(bias_s, a.bias, head);
    const int64_t L = (int64_t)a.Hs * a.W;
    const uint32_t rsb = (IO32 ? 12u : 6u) * a.C, rob = (IO32 ? 4u : 2u) * a.C;   // row strides in bytes
    uint32_t* ti = tok_in[wave];
    uint32_t* to = tok_out[wave];
    float* invw = inv_s[wave];
    for (int64_t bw = (int64_t)slot * 4 + wave; bw < nwin; bw += (int64_t)a.groups * 4) {   // all scalar
        const int64_t b = unit_tokens(a, bw, lane, rsb, rob, ti, to);
        const char* base = IO32 ? reinterpret_cast<const char*>(a.qkv + b * L * 3 * a.C + head * HD)
                                : reinterpret_cast<const char*>(reinterpret_cast<const __bf16*>(a.qkv) + b * L * 3 * a.C + head * HD);
        const char* kbase = base + (IO32 ? 4 : 2) * a.C;
        const char* vbase = base + (IO32 ? 8 : 4) * a.C;

        // q / k: [tile][k-step] fragments, 16 bytes each, straight from memory (IO32: 32 bytes, rounded on the way)
        bf16x8 qf[2][2], kf[2][2];
#pragma unroll
        for (int t = 0; t < 2; ++t) {
            if (IO32) {
                const uint32_t off = ti[32 * t + c] + 32u * h;
                load_frag_bf16(qf[t], base, off);
                load_frag_bf16(kf[t], kbase, off);
                continue;
            }
            const uint32_t off = ti[32 * t + c] + 16u * h;
#pragma unroll
            for (int st = 0; st < 2; ++st) {
                qf[t][st] = *reinterpret_cast<const bf16x8*>(base + (off + 32u * st));
                kf[t][st] = *reinterpret_cast<const bf16x8*>(kbase + (off + 32u * st));
            }
        }
        // v: [key tile][k-step] fragments in the permuted key order of the P operand; element j = key 32jt + 16s + 8(j>>2) + 4h + (j&3)
        bf16x8 vf[2][2];
        if (IO32) load_perm_bf16(vf, vbase, ti, c, h);
#pragma unroll
        for (int jt = 0; jt < 2 && !IO32; ++jt)
#pragma unroll
            for (int st = 0; st < 2; ++st) {
                u16x8 pk = {0, 0, 0, 0, 0, 0, 0, 0};
#pragma unroll
                for (int q = 0; q < 2; ++q) {
                    if (jt == 1 && st == 1 && q == 1) continue;                            // keys 56..63: all padding
                    const u32x4 t4 = *reinterpret_cast<const u32x4*>(&ti[32 * jt + 16 * st + 8 * q + 4 * h]);
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        if (jt == 1 && st == 1 && e > 0) continue;                         // keys 49..51 / 53..55: padding in both halves
                        pk[4 * q + e] = *reinterpret_cast<const uint16_t*>(vbase + (t4[e] + 2u * c));
                    }
                }
                vf[jt][st] = __builtin_bit_cast(bf16x8, pk);
            }

        const float* mask_w = unit_mask(a, bw);
        char* obase = IO32 ? reinterpret_cast<char*>(a.out + b * L * a.C + head * HD)
                           : reinterpret_cast<char*>(reinterpret_cast<__bf16*>(a.out) + b * L * a.C + head * HD);
        auto tiles = [&](auto masked) {
            constexpr bool MASKED = decltype(masked)::value;
#pragma unroll
            for (int it = 0; it < 2; ++it) {
                f32x16 s[2] = {};
#pragma unroll
                for (int st = 0; st < 2; ++st)
#pragma unroll
                    for (int jt = 0; jt < 2; ++jt) s[jt] = mfma16(kf[jt][st], qf[it][st], s[jt]);   // S^T[jt] += K[jt] Q[it]^T
                const int qi = 32 * it + c;
                float m, inv;
                bias_softmax<MASKED, false>(s, bias_row(bias_s, BLD, qi, h), mask_w, qi, h, a.scale, &m, &inv);
                invw[qi] = inv;                                                                      // both lane halves hold the same value
                f32x16 o = {};
#pragma unroll
                for (int jt = 0; jt < 2; ++jt)
#pragma unroll
                    for (int st = 0; st < 2; ++st) o = mfma16(acc_frag(s[jt], st), vf[jt][st], o);
                __builtin_amdgcn_wave_barrier();
                // per register group g: the 4 consecutive queries 32it + 8g + 4h .. +3 -- their out-row offsets and 1/sum, one 16-byte read each
#pragma unroll
                for (int g = 0; g < 4; ++g) {
                    if (acc_pad(it, g)) continue;
                    const u32x4 to4 = *reinterpret_cast<const u32x4*>(&to[32 * it + 8 * g + 4 * h]);
                    const f32x4 iv = *reinterpret_cast<const f32x4*>(&invw[32 * it + 8 * g + 4 * h]);
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        if (acc_pad(it, g, e)) continue;
                        const int i = 32 * it + 8 * g + 4 * h + e;
                        if (i < WT) {
                            if (IO32) *reinterpret_cast<float*>(obase + (to4[e] + 4u * c)) = o[4 * g + e] * iv[e];
                            else *reinterpret_cast<__bf16*>(obase + (to4[e] + 2u * c)) = (__bf16)(o[4 * g + e] * iv[e]);
                        }
                    }
                }
            }
        };
        if (mask_w) tiles(std::true_type{}); else tiles(std::false_type{});
        __builtin_amdgcn_wave_barrier();   // the token tables are rewritten by the next unit
    }
}

// relative_position_bias_table (169, nH) + relative_position_index (49*49, int32) -> padded bias (nH, 64, 64) [head][query][key]:
// rows >= 49 zero, key columns >= 49 = -1e30 (the 49 -> 64 padding mask of the attention kernels; swin:148-151)
__global__ __launch_bounds__(256) void relpos_bias_expand_kernel(const float* __restrict__ table, const int32_t* __restrict__ rel_index,
                                                                 float* __restrict__ out, int nH) {
    // one element per thread (grid (nH, 16)): the two dependent loads of an element are the whole latency of the kernel -- sixteen
    // elements per thread in sequence made this 4096-element gather take 10 us, 60 times per training step
    const int head = blockIdx.x, e = blockIdx.y * 256 + threadIdx.x;
    const int i = e >> 6, j = e & 63;
    float v = 0.f;
    if (j >= WT) v = -1e30f;
    else if (i < WT) v = table[(int64_t)rel_index[i * WT + j] * nH + head];
    out[(int64_t)head * 4096 + e] = v;
}

}  // namespace

// What an entry point asks of the launcher: the storage of qkv / out, the MFMA of the two products, and the LDS-free "background" form
enum class Storage { F32, BF16 };
enum class Math { F32, BF16 };
struct SelfKind { Storage storage; Math math; bool background; };

// Launch geometry.  Both forms are persistent: `groups` blocks per head, each walking its head's window quads.
// fp32 flow: ~3 resident blocks per CU (3 waves/SIMD)
static int64_t fp32_flow_groups(int64_t quads, int nH) {
    static const int wa_blocks = tune_int("MUMPY_WA_BLOCKS", 768);
    const int64_t groups = (wa_blocks + nH - 1) / nH;
    return groups > quads ? quads : groups;
}
// bf16 MFMA: 4 resident blocks per CU; the quads are dealt evenly (every block walks the same number of them, +-0)
static int64_t bf16mm_groups(int64_t quads, int nH) {
    static const int wa16_blocks = tune_int("MUMPY_WA16_BLOCKS", 1024);
    int64_t groups = (wa16_blocks + nH - 1) / nH;
    if (groups > quads) groups = quads;
    const int64_t per = (quads + groups - 1) / groups;
    return (quads + per - 1) / per;
}

// Which form a launch takes: bit 0 = split (win_attn_self_split_kernel: one unit on two waves), bit 1 = K/V ring (reserved: no
// launch takes it, see the file header).  A pure function of the entry point and the shape.  Only the fp32 entry point splits, and
// only while `units` is at most SPLIT_UNITS (the fitted rule and its table are in the file header).  MUMPY_WA_SPLIT_UNITS moves the
// threshold in the tuning build; it is read per launch there so that tools/kernel_micro.py can time both forms in one process.
constexpr int SPLIT_UNITS = 2560;
static int self_plan(SelfKind kind, int64_t units) {
    if (kind.storage != Storage::F32 || kind.math != Math::F32 || kind.background) return 0;
    return units <= tune_int("MUMPY_WA_SPLIT_UNITS", SPLIT_UNITS) ? 1 : 0;
}

static int window_attention_launch(SelfKind kind, const float* qkv, float* out, const float* bias, const float* mask_tab,
                                   const int32_t* mask_id, int n_mask, int B, int Hs, int W, int C, int shift, float scale,
                                   void* stream) {
    MUMPY_REQUIRE(qkv && out && bias, MUMPY_ENULL, "window_attention: null pointer");
    MUMPY_REQUIRE((mask_tab == nullptr) == (mask_id == nullptr), MUMPY_ENULL,
                  "window_attention: mask_tab and mask_id must be given together");
    MUMPY_REQUIRE(aligned16(qkv) && aligned16(out) && aligned16(bias) && aligned16(mask_tab), MUMPY_EALIGN,
                  "window_attention: pointers must be 16-byte aligned");
    MUMPY_REQUIRE(B > 0 && Hs > 0 && W > 0 && Hs % WS == 0 && W % WS == 0, MUMPY_EINVAL,
                  "window_attention: grid (%d,%d) not divisible by window 7", Hs, W);
    MUMPY_REQUIRE(C > 0 && C % HD == 0, MUMPY_EINVAL, "window_attention: C=%d not a multiple of head width 32", C);
    MUMPY_REQUIRE(shift >= 0 && shift < WS, MUMPY_EINVAL, "window_attention: shift=%d out of [0,7)", shift);
    MUMPY_REQUIRE(n_mask >= 0 && (mask_id == nullptr || n_mask > 0), MUMPY_EINVAL, "window_attention: n_mask must be > 0 with a mask (and never negative)");
    SelfArgs a;
    a.qkv = qkv; a.out = out; a.bias = bias; a.mask_tab = mask_tab; a.mask_id = mask_id;
    a.B = B; a.Hs = Hs; a.W = W; a.C = C; a.nH = C / HD; a.shift = shift;
    a.nWx = W / WS; a.nW = (Hs / WS) * (W / WS); a.scale = scale; a.n_mask = n_mask > 0 ? n_mask : 1;
    static const int dbgmask = tune_int("MUMPY_WA_DBG", 0);
    static const int wa_stagger = tune_int("MUMPY_WA_STAGGER", 0);
    a.dbg = dbgmask; a.stagger = wa_stagger;
    a.units = (int64_t)B * a.nW * a.nH;
    const int64_t quads = ((int64_t)B * a.nW + 3) / 4;
    const bool mm16 = kind.math == Math::BF16, io16 = kind.storage == Storage::BF16;
    a.groups = (int)(mm16 ? bf16mm_groups(quads, a.nH) : fp32_flow_groups(quads, a.nH));
    const dim3 grid((unsigned)((int64_t)a.groups * a.nH)), block(256);
    hipStream_t s = as_stream(stream);
    if (mm16 && io16) hipLaunchKernelGGL(win_attn_self_bf16mm_kernel<false>, grid, block, 0, s, a);
    else if (mm16) hipLaunchKernelGGL(win_attn_self_bf16mm_kernel<true>, grid, block, 0, s, a);
    else if (kind.background) hipLaunchKernelGGL((win_attn_self_kernel<false, false, true>), grid, block, 0, s, a);
    else if (io16) hipLaunchKernelGGL((win_attn_self_kernel<false, true>), grid, block, 0, s, a);
    else if (dbgmask) hipLaunchKernelGGL((win_attn_self_kernel<true, false>), grid, block, 0, s, a);
    else if (self_plan(kind, a.units) & 1)
        hipLaunchKernelGGL(win_attn_self_split_kernel, dim3((unsigned)((((int64_t)B * a.nW + 1) / 2) * a.nH)), block, 0, s, a);
    else hipLaunchKernelGGL((win_attn_self_kernel<false, false>), grid, block, 0, s, a);
    MUMPY_CHECK_LAUNCH("window_attention");
    return 0;
}

extern "C" int mumpy_window_attention_fwd(const float* qkv, float* out, const float* bias, const float* mask_tab,
                                          const int32_t* mask_id, int n_mask, int B, int Hs, int W, int C, int shift,
                                          float scale, void* stream) {
    return window_attention_launch({Storage::F32, Math::F32, false}, qkv, out, bias, mask_tab, mask_id, n_mask, B, Hs, W, C, shift, scale,
                                   stream);
}

// The launch form of mumpy_window_attention_fwd / of the bf16-storage entry points for this shape (self_plan; no GPU needed):
// bit 0 = split, bit 1 = ring; negative = the shape is one the entry points reject.
static int window_attention_plan(SelfKind kind, int B, int Hs, int W, int C) {
    MUMPY_REQUIRE(B > 0 && Hs > 0 && W > 0 && Hs % WS == 0 && W % WS == 0 && C > 0 && C % HD == 0, MUMPY_EINVAL,
                  "window_attention_plan: bad shape (%d,%d,%d,%d)", B, Hs, W, C);
    return self_plan(kind, (int64_t)B * (Hs / WS) * (W / WS) * (C / HD));
}
extern "C" int mumpy_window_attention_plan(int B, int Hs, int W, int C) {
    return window_attention_plan({Storage::F32, Math::F32, false}, B, Hs, W, C);
}
extern "C" int mumpy_window_attention_bf16_plan(int B, int Hs, int W, int C) {
    return window_attention_plan({Storage::BF16, Math::F32, false}, B, Hs, W, C);
}

// "Background" form: identical arithmetic and results, NO LDS allocation (token tables in registers via ds_bpermute, bias rows from
// L1), so that the launch can be resident beside the persistent GEMM, which owns every CU's whole LDS (see gemm_rd.hip).
extern "C" int mumpy_window_attention_bg_fwd(const float* qkv, float* out, const float* bias, const float* mask_tab,
                                             const int32_t* mask_id, int n_mask, int B, int Hs, int W, int C, int shift,
                                             float scale, void* stream) {
    return window_attention_launch({Storage::F32, Math::F32, true}, qkv, out, bias, mask_tab, mask_id, n_mask, B, Hs, W, C, shift, scale,
                                   stream);
}

// bf16 STORAGE: qkv (B, Hs*W, 3C) and out (B, Hs*W, C) are bf16; bias / mask tables fp32; same arithmetic.
extern "C" int mumpy_window_attention_bf16_fwd(const void* qkv, void* out, const float* bias, const float* mask_tab,
                                               const int32_t* mask_id, int n_mask, int B, int Hs, int W, int C, int shift,
                                               float scale, void* stream) {
    return window_attention_launch({Storage::BF16, Math::F32, false}, static_cast<const float*>(qkv), static_cast<float*>(out), bias,
                                   mask_tab, mask_id, n_mask, B, Hs, W, C, shift, scale, stream);
}

// bf16 storage AND bf16 matrix math: Q K^T and P V on the bf16 MFMA (fp32 accumulation, fp32 softmax, P re-quantised to bf16);
// `scale` is applied to the fp32 scores after the product.  Same arguments, validation and error codes as the entry above.
extern "C" int mumpy_window_attention_bf16mm_fwd(const void* qkv, void* out, const float* bias, const float* mask_tab,
                                                 const int32_t* mask_id, int n_mask, int B, int Hs, int W, int C, int shift,
                                                 float scale, void* stream) {
    return window_attention_launch({Storage::BF16, Math::BF16, false}, static_cast<const float*>(qkv), static_cast<float*>(out), bias,
                                   mask_tab, mask_id, n_mask, B, Hs, W, C, shift, scale, stream);
}

// fp32 storage, bf16 matrix math: the forward of the training tape under ops.set_attention_math("bf16").  Same arguments, validation
// and error codes as mumpy_window_attention_fwd; `scale` multiplies the fp32 scores after the product.
extern "C" int mumpy_window_attention_mm16_fwd(const float* qkv, float* out, const float* bias, const float* mask_tab,
                                               const int32_t* mask_id, int n_mask, int B, int Hs, int W, int C, int shift,
                                               float scale, void* stream) {
    return window_attention_launch({Storage::F32, Math::BF16, false}, qkv, out, bias, mask_tab, mask_id, n_mask, B, Hs, W, C, shift, scale,
                                   stream);
}

extern "C" int mumpy_relpos_bias_expand_fwd(const float* table, const int32_t* rel_index, float* out, int nH, void* stream) {
    MUMPY_REQUIRE(table && rel_index && out, MUMPY_ENULL, "relpos_bias_expand: null pointer");
    MUMPY_REQUIRE(nH > 0, MUMPY_EINVAL, "relpos_bias_expand: bad head count %d", nH);
    hipLaunchKernelGGL(relpos_bias_expand_kernel, dim3((unsigned)nH, 16), dim3(256), 0, as_stream(stream), table, rel_index, out, nH);
    MUMPY_CHECK_LAUNCH("relpos_bias_expand");
    return 0;
}
