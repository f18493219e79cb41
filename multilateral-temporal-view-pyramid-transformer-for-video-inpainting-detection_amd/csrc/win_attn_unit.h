// win_attn_unit.h — the (window, head) attention unit shared by window_attention.hip (self-attention forward),
// window_attention_bwd.hip (its backward) and deform_attention.hip (deformable cross-view attention, forward and backward):
// one unit per wave, everything in registers, fp32 MFMA (v_mfma_f32_32x32x2_f32) or bf16 MFMA (v_mfma_f32_32x32x16_bf16).
//
// Data flow per unit (49 tokens x 32 channels per operand, padded to 64 x 32 inside the wave):
//   * Q and K rows are loaded straight into MFMA operand layout: lane (r = lane&31, h = lane>>5) holds, for the
//     rows r and r+32, the 16 consecutive channels [16h, 16h+16) -> k-slot h of MFMA step s is channel 16h+s.
//     The window gather and the cyclic shift are nothing but the row address; nothing is staged or materialised.
//   * S^T = K Q^T is accumulated (key on the MFMA row, query on the lane), so a query's scores live in ONE lane
//     pair (lane, lane^32): softmax is 32 registers + one cross-half exchange, no LDS.
//   * the normalised P stays in the accumulator registers and is fed back as the A operand of P V (the
//     accumulator->operand trick: k-slot h of step (jt,g,e) is key 32jt+8g+4h+e, which is exactly the key the
//     lane's register 4g+e holds); V rows are loaded in that same key order, one dword per lane (128-B rows).
//   * keys >= 49 are masked by the -1e30 columns of the pre-padded bias; queries >= 49 are never stored.
// The self-attention kernels (forward and backward) are persistent: a block is ONE head x 4 consecutive windows per pass,
// stages the head's bias table once in LDS and walks `groups` window quads apart; wave w of block (slot, head) takes the
// windows bw = 4 slot + w, + 4 groups, ...  Each kernel body is, in this order: stage_bias / stage_bias_T, then per unit
// unit_tokens, unit_mask, the operand loads, and per 32-row tile the products around bias_softmax.
#pragma once
#include <type_traits>
#include "common.h"

using namespace mumpy;

namespace {

struct SelfArgs {
    const float* qkv;
    float* out;
    const float* bias;      // (nH,64,64)
    const float* mask_tab;  // (nU,64,64) or null
    const int32_t* mask_id; // (n_mask) or null; window bw uses mask_id[bw % n_mask]
    int B, Hs, W, C, nH, shift, nWx, nW, n_mask, groups, stagger;
    int dbg;               // diagnostic ablation mask (MUMPY_WA_DBG): 1 skip q/k/v loads, 2 skip MFMAs+softmax, 4 skip stores
    float scale;
    int64_t units;
};

struct BwdArgs {
    const float* qkv; const float* dout; const float* bias; const float* mask_tab; const int32_t* mask_id;
    float* dqkv; float* stats; float* dbias_part;
    int B, Hs, W, C, nH, shift, nWx, nW, n_mask, groups;
    float scale;
};

__device__ __forceinline__ f32x16 mfma32(float a, float b, f32x16 c) {
    return __builtin_amdgcn_mfma_f32_32x32x2f32(a, b, c, 0, 0, 0);
}

// Accumulator rows: register r = 4g + e of the 32x32 accumulator tile t holds, in lane half h, row 32t + 8g + 4h + e (a query or a
// key, depending on the product's orientation).  Rows >= 49 are padding.  Known at compile time, for both lane halves: group 3 of
// tile 1 (rows 56..63) and registers 1..3 of its group 2 (rows 49..51 / 53..55; register 0 is row 48 in half 0 and row 52 in half 1).
// A store loop skips those statically -- acc_pad(t, g) / acc_pad(t, g, e) where it walks groups and registers, !acc_live(t, r) where
// it walks r -- and tests acc_row(..) < WT on the rest.  (The two forms of acc_row add the same terms in the order their callers
// always did: LLVM schedules the stores after it.)
__device__ __forceinline__ constexpr bool acc_pad(int t, int g) { return t == 1 && g == 3; }
__device__ __forceinline__ constexpr bool acc_pad(int t, int g, int e) { return t == 1 && g == 2 && e > 0; }
__device__ __forceinline__ constexpr bool acc_live(int t, int r) { return !(acc_pad(t, r >> 2) || acc_pad(t, r >> 2, r & 3)); }
__device__ __forceinline__ constexpr int acc_row(int t, int g, int e, int h) { return 32 * t + 8 * g + 4 * h + e; }
__device__ __forceinline__ constexpr int acc_row(int t, int r, int h) { return 32 * t + (r & 3) + 8 * (r >> 2) + 4 * h; }

// load the 16 channels [16h,16h+16) of one 32-channel head row.  Padded rows (token slot >= 49) are CLAMPED to slot 48 by
// the token table instead of predicated: the duplicates are finite, their scores are overwritten with -1e30 (keys) or
// never stored (queries), and branch-free loads keep the compiler's vmcnt bookkeeping exact, which the cross-unit
// prefetch depends on (an exec-masked load made it wait vmcnt(0) and drain the prefetch).
__device__ __forceinline__ void load_frag(f32x4 (&f)[4], const float* row, bool valid) {
#pragma unroll
    for (int i = 0; i < 4; ++i) f[i] = valid ? *reinterpret_cast<const f32x4*>(row + 4 * i) : f32x4{0, 0, 0, 0};
}

// S^T[jt] += K[jt] Q^T for ONE query tile (32 queries on the lanes); q already scaled
__device__ __forceinline__ void qk_product(f32x16 (&s)[2], const f32x4 (&kf)[2][4], const f32x4 (&qf)[4]) {
#pragma unroll
    for (int st = 0; st < 16; ++st) {
#pragma unroll
        for (int jt = 0; jt < 2; ++jt) s[jt] = mfma32(kf[jt][st >> 2][st & 3], qf[st >> 2][st & 3], s[jt]);
    }
}

// add bias (+mask) rows and run the softmax over keys for the query column this lane owns (query i = 32*it + c).
// MASKED is a compile-time switch: the caller branches once per unit on the (wave-uniform) mask pointer, so unmasked
// windows run branch-free and a masked window issues its 7 mask loads back to back (one wait) instead of load-wait pairs.
// NORMALISE = false leaves the exponentials e_j = exp(s_j - max) in s (their fp32 sum's reciprocal goes to *inv_out): the bf16-MFMA
// kernel rounds those to bf16 and scales the product instead.
template <bool MASKED, bool NORMALISE = true, typename BIAS>
__device__ __forceinline__ void bias_softmax(f32x16 (&s)[2], BIAS bias_at, const float* mask_w, int i, int h,
                                             float post_scale, float* m_out = nullptr, float* inv_out = nullptr) {
    constexpr float NEG = -1e30f;
#pragma unroll
    for (int jt = 0; jt < 2; ++jt)
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            if (jt == 1 && g == 3) continue;                             // keys 56..63: all padding
            const f32x4 b = bias_at(jt, g);                              // keys 32jt+8g+4h .. +3 of query i
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                if (jt == 1 && g == 2 && e > 0) continue;                // keys 49..51 / 53..55: padding in both halves
                s[jt][4 * g + e] = s[jt][4 * g + e] * post_scale + b[e];
            }
        }
    if (MASKED) {                                                        // (s + bias) + mask, as swin:153-157
#pragma unroll
        for (int jt = 0; jt < 2; ++jt) {
            f32x4 mk[4];
#pragma unroll
            for (int g = 0; g < 4; ++g)
                if (!(jt == 1 && g == 3)) mk[g] = *reinterpret_cast<const f32x4*>(mask_w + i * 64 + 32 * jt + 8 * g + 4 * h);
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                if (jt == 1 && g == 3) continue;
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    if (jt == 1 && g == 2 && e > 0) continue;
                    s[jt][4 * g + e] += mk[g][e];
                }
            }
        }
    }
    float m = NEG;
#pragma unroll
    for (int jt = 0; jt < 2; ++jt)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            if (jt == 1 && r >= 9) continue;
            m = fmaxf(m, s[jt][r]);
        }
    m = fmaxf(m, __shfl_xor(m, 32));
    float sum = 0.f;
#pragma unroll
    for (int jt = 0; jt < 2; ++jt)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            if (jt == 1 && r >= 9) { s[jt][r] = 0.f; continue; }        // padded keys: exp(-1e30 - m) == 0 exactly
            const float e = __expf(s[jt][r] - m);
            s[jt][r] = e;
            sum += e;
        }
    sum += __shfl_xor(sum, 32);
    const float inv = 1.0f / sum;
    if (NORMALISE) {
#pragma unroll
        for (int jt = 0; jt < 2; ++jt)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                if (jt == 1 && r >= 9) continue;
                s[jt][r] *= inv;
            }
    }
    if (m_out) { *m_out = m; *inv_out = inv; }
}

// the 25 (jt,g,e) MFMA steps of P V that can hold a key < 49; key of lane half h is 32jt+8g+4h+e
template <typename F>
__device__ __forceinline__ void for_pv_steps(F&& body) {
#pragma unroll
    for (int jt = 0; jt < 2; ++jt)
#pragma unroll
        for (int g = 0; g < 4; ++g)
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                if (jt == 1 && (g == 3 || (g == 2 && e > 0))) continue;
                body(jt, g, e);
            }
}

template <typename VROW>
__device__ __forceinline__ void load_v(float (&vf)[2][16], VROW vrow, int c, int h) {
    for_pv_steps([&](int jt, int g, int e) {
        const int j = 32 * jt + 8 * g + 4 * h + e;
        vf[jt][4 * g + e] = (j < WT) ? vrow(j)[c] : 0.f;
    });
}

__device__ __forceinline__ void pv_product(f32x16& o, const f32x16 (&s)[2], const float (&vf)[2][16]) {
    for_pv_steps([&](int jt, int g, int e) { o = mfma32(s[jt][4 * g + e], vf[jt][4 * g + e], o); });
}

template <typename OROW>
__device__ __forceinline__ void store_o(const f32x16& o, int it, OROW orow, int c, int h) {
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        if (!acc_live(it, r)) continue;
        const int i = acc_row(it, r, h);
        if (i < WT) orow(i)[c] = o[r];
    }
}

// ---------------------------------------------------------------------------------------------------------------
constexpr int BLD = 68;   // LDS row stride of the staged bias table: 68 floats -> conflict-free ds_read_b128 across rows

// byte-offset addressing: base is wave-uniform (SGPR pair), the per-lane part a 32-bit byte offset from the token tables,
// so every access is "global_* v, v_off, s[base]" with one v_add at most -- the 64-bit token*stride products the
// pointer form needs (2 v_mul_lo + v_mad_u64 + ... per access, all quarter-rate) cost ~40 % of the MFMA time of a unit.
__device__ __forceinline__ const f32x4* at16(const char* base, uint32_t off) {
    return reinterpret_cast<const f32x4*>(base + off);
}

// 16 consecutive channels [16h, 16h+16) of a 32-channel head row (MFMA A/B fragment layout of the forward)
__device__ __forceinline__ void load_frag16(f32x4 (&f)[4], const char* base, uint32_t off) {
#pragma unroll
    for (int i = 0; i < 4; ++i) f[i] = *reinterpret_cast<const f32x4*>(base + (off + 16u * i));
}

// The head's 49x64 bias table, staged ONCE per persistent block in LDS, rows BLD apart (the per-lane row-strided reads of it would
// otherwise cost as many L1 tag cycles as the MFMAs).  Ends with the block barrier.
__device__ __forceinline__ void stage_bias(float* bias_s, const float* bias, int head) {
    const float* bsrc = bias + (int64_t)head * 4096;
    for (int idx = threadIdx.x; idx < WT * 16; idx += 256) {
        const int row = idx >> 4, c4 = idx & 15;
        *reinterpret_cast<f32x4*>(&bias_s[row * BLD + 4 * c4]) = *reinterpret_cast<const f32x4*>(bsrc + row * 64 + 4 * c4);
    }
    __syncthreads();
}

// The same table transposed (row = key j, column = query i) for the key-on-the-lane orientation of the kv kernels; the query columns
// 49..63 of every key row get a finite filler.  Ends with the block barrier.
__device__ __forceinline__ void stage_bias_T(float* biasT_s, const float* bias, int head) {
    const float* bsrc = bias + (int64_t)head * 4096;
    for (int idx = threadIdx.x; idx < WT * WT; idx += 256) {
        const int i = idx / WT, j = idx - i * WT;
        biasT_s[j * BLD + i] = bsrc[i * 64 + j];
    }
    for (int idx = threadIdx.x; idx < WT * (64 - WT); idx += 256) {
        const int j = idx / (64 - WT), i = WT + idx % (64 - WT);
        biasT_s[j * BLD + i] = 0.f;
    }
    __syncthreads();
}

// Window bw of the walk -> image b (returned) and this lane's raster token of the window (padded slots 49..63 -> slot 48); all but
// the token is scalar.
template <typename ARGS>
__device__ __forceinline__ int64_t unit_token(const ARGS& a, int64_t bw, int lane, uint32_t& tok) {
    const int n = (int)(bw % a.nW);
    const int wy = n / a.nWx, wx = n - wy * a.nWx;
    tok = (uint32_t)window_token(wy, wx, lane < WT ? lane : WT - 1, a.Hs, a.W, a.shift);
    return bw / a.nW;
}

// ... and the wave's token tables in LDS: ti[p] / to[p] = byte offset of window slot p's qkv row (pitch rsb) / out row (pitch rob).
// The wave barrier orders the fill (and whatever else the caller wrote to its LDS just before) ahead of the reads.
template <typename ARGS>
__device__ __forceinline__ int64_t unit_tokens(const ARGS& a, int64_t bw, int lane, uint32_t rsb, uint32_t rob, uint32_t* ti,
                                               uint32_t* to) {
    uint32_t tok;
    const int64_t b = unit_token(a, bw, lane, tok);
    ti[lane] = tok * rsb;
    to[lane] = tok * rob;
    __builtin_amdgcn_wave_barrier();
    return b;
}

// The unit's 64x64 shift-mask table, or null for an unmasked window (scalar load; wave-uniform, so the caller can branch on it once)
template <typename ARGS>
__device__ __forceinline__ const float* unit_mask(const ARGS& a, int64_t bw) {
    const float* mask_w = nullptr;
    if (a.mask_id) {
        const int id = a.mask_id[bw % a.n_mask];
        if (id >= 0) mask_w = a.mask_tab + (int64_t)id * 4096;
    }
    return mask_w;
}

// The 49 -> 64 key padding of a bias vector of keys 32jt + 8g + 4h .. +3: key 52 is padding while key 48 (lane half 0 of the same
// register) is real, so it cannot be skipped statically like keys 49..51 / 53..63 (bias_softmax) and is masked here.
__device__ __forceinline__ f32x4 pad_key52(f32x4 bv, int jt, int g, int h) {
    if (jt == 1 && g == 2 && h) bv.x = -1e30f;
    return bv;
}

// bias_at(jt, g) of bias_softmax for query qi from a bias table with rows `ld` floats apart (the LDS copy: BLD; global memory: 64);
// padded queries re-read row 48
__device__ __forceinline__ auto bias_row(const float* tab, int ld, int qi, int h) {
    const float* brow = tab + (qi < WT ? qi : WT - 1) * ld + 4 * h;
    return [brow, h](int jt, int g) { return pad_key52(*reinterpret_cast<const f32x4*>(brow + 32 * jt + 8 * g), jt, g, h); };
}

// ---------------------------------------------------------------------------------------------------------------
// bf16-MFMA operands
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
typedef uint16_t u16x8 __attribute__((ext_vector_type(8)));

__device__ __forceinline__ f32x16 mfma16(bf16x8 a, bf16x8 b, f32x16 c) {
    return __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, b, c, 0, 0, 0);
}

// 8 fp32 values -> one bf16 operand fragment, round to nearest even (v_cvt_pk_bf16_f32)
__device__ __forceinline__ bf16x8 cvt8(f32x4 lo, f32x4 hi) {
    bf16x8 r;
#pragma unroll
    for (int i = 0; i < 4; ++i) { r[i] = (__bf16)lo[i]; r[4 + i] = (__bf16)hi[i]; }
    return r;
}

// the accumulator tile as an A operand with no lane movement: registers 8ks .. 8ks+7, cast pairwise to bf16, are k-step ks.  The k
// order inside a step is permuted: element j of lane half h is row 32t + 16ks + 8(j>>2) + 4h + (j&3) (see load_perm_bf16).
__device__ __forceinline__ bf16x8 acc_frag(const f32x16& s, int ks) {
    bf16x8 f;
#pragma unroll
    for (int j = 0; j < 8; ++j) f[j] = (__bf16)s[8 * ks + j];
    return f;
}

// the [k-step] operand fragments of an fp32 head row: channels 16 st + 8h .. +7, rounded to bf16 in registers (off includes 32h)
__device__ __forceinline__ void load_frag_bf16(bf16x8 (&f)[2], const char* base, uint32_t off) {
#pragma unroll
    for (int st = 0; st < 2; ++st) f[st] = cvt8(*at16(base, off + 64u * st), *at16(base, off + 64u * st + 16u));
}

// channel c of an fp32 operand's rows in the permuted order of an accumulator-fed A operand: element j of fragment [tile t][k-step st]
// is row 32t + 16st + 8(j>>2) + 4h + (j&3) (4-byte gathers, rounded to bf16).  Rows 49..51 / 53.. are zero, row 52 is slot 48's value
// (token table clamp): the A operand is exactly 0 on all of them.
__device__ __forceinline__ void load_perm_bf16(bf16x8 (&f)[2][2], const char* base, const uint32_t* tab, int c, int h) {
#pragma unroll
    for (int t = 0; t < 2; ++t)
#pragma unroll
        for (int st = 0; st < 2; ++st) {
            bf16x8 v;
#pragma unroll
            for (int j = 0; j < 8; ++j) v[j] = (__bf16)0.f;
#pragma unroll
            for (int q = 0; q < 2; ++q) {
                if (t == 1 && st == 1 && q == 1) continue;                                 // rows 56..63: all padding
                const u32x4 t4 = *reinterpret_cast<const u32x4*>(&tab[32 * t + 16 * st + 8 * q + 4 * h]);
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    if (t == 1 && st == 1 && e > 0) continue;                              // rows 49..51 / 53..55: padding in both halves
                    v[4 * q + e] = (__bf16)*reinterpret_cast<const float*>(base + (t4[e] + 4u * c));
                }
            }
            f[t][st] = v;
        }
}

}  // namespace
