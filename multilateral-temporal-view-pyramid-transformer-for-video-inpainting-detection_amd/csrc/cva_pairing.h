// cva_pairing.h — which q window a kv window of the cross-view attention attends with: the one rule the sampling kernels
// (deform.hip, cva_fused.hip), the attention core (deform_attention.hip) and their backward kernels (deform_bwd.hip,
// deform_attention.hip) share, and the host check of its arguments.
//
// The reference pairs kv window i with q window i mod nq (`x1.repeat`, deform:330) and sums ADJACENT r-tuples of kv windows into
// output window i / r (deform:394-395); nq is every q window of every clip of the batch, so the clips of a batch are coupled.
// Grouped pairing (include/mumpy_hip_ext8.h) cuts the launch into G independent groups of nqg = nq / G q windows and r nqg kv
// windows each and applies the reference's rule inside every group:
//   g = i / (r nqg),   q(i) = g nqg + ((i - g r nqg) mod nqg),   out(i) = i / r  (unchanged: r nqg is a multiple of r)
// G = 1 is the reference's rule; G = B treats every clip as the reference treats a batch of one; for r = 1 both give q(i) = i.
// The inverse, for the kernels that start from a q window (the bf16 backward's q kernel, include/mumpy_hip_ext9.h): with
//   g = qw / nqg,  j = qw - g nqg,   the m-th kv window of q window qw is  kv(qw, m) = g span + j + m nqg,  m = 0 .. r-1
// (ascending in m and in the window index: the order a group's r contributions are summed in; G = 1: qw + m nq).
//
// GROUPED is a template parameter of the kernels: the <false> instantiations carry one int, exactly the `nq` / `B1w` they
// carried before the rule had a second form, and compute `i % nq` in the index type they computed it in -- their code is
// unchanged.  The <true> instantiations pay one more integer division per kv window (per staged row in cva_fused.hip), next
// to the 49 x C floats of work behind each.
#pragma once
#include "common.h"

namespace mumpy {

template <bool GROUPED> struct CvaPairing;
template <> struct CvaPairing<false> { int nq; };
template <> struct CvaPairing<true> { int nq, nqg, span; };      // nqg = nq / G q windows and span = r nqg kv windows per group

template <bool GROUPED, typename I>
__device__ __forceinline__ I cva_q_window(I i, const CvaPairing<GROUPED>& p) {
    if constexpr (!GROUPED) {
        return i % p.nq;
    } else {
        const I g = i / p.span;
        return g * p.nqg + (i - g * p.span) % p.nqg;
    }
}

// the m-th kv window that attends with q window qw (cva_q_window(cva_kv_window(qw, m, p), p) == qw)
template <bool GROUPED, typename I>
__device__ __forceinline__ I cva_kv_window(I qw, int m, const CvaPairing<GROUPED>& p) {
    if constexpr (!GROUPED) {
        return qw + (I)m * p.nq;
    } else {
        const I g = qw / p.nqg;
        return g * p.span + (qw - g * p.nqg) + (I)m * p.nqg;
    }
}

// Host side of a grouped entry that takes window counts (the backward entries, include/mumpy_hip_ext9.h): MUMPY_EINVAL unless
// 1 <= groups, groups | nq and nq | nkv; fills the pairing of a launch with groups > 1 -- a group is nq / groups q windows with
// their kv windows, whatever number of clips that is.  (groups == 1 launches the <false> instantiations and needs none of this.)
inline int cva_grouping_windows(const char* who, int64_t nkv, int64_t nq, int groups, CvaPairing<true>* p) {
    MUMPY_REQUIRE(groups >= 1, MUMPY_EINVAL, "%s: groups=%d must be at least 1", who, groups);
    MUMPY_REQUIRE(nq > 0 && nq % groups == 0, MUMPY_EINVAL, "%s: groups=%d must divide the %lld q windows", who, groups, (long long)nq);
    MUMPY_REQUIRE(groups == 1 || nkv % nq == 0, MUMPY_EINVAL, "%s: %lld kv windows are not a multiple of %lld q windows", who,
                  (long long)nkv, (long long)nq);
    MUMPY_REQUIRE(nkv < (1ll << 31) && nq < (1ll << 31), MUMPY_ERANGE, "%s: too many windows", who);
    p->nq = (int)nq;
    p->nqg = (int)(nq / groups);
    p->span = (int)(nkv / nq) * p->nqg;
    return 0;
}

// ... and of one that takes the batch size as well (the forward entries, include/mumpy_hip_ext8.h): groups | B on top of that
inline int cva_grouping(const char* who, int64_t nkv, int64_t nq, int B, int groups, CvaPairing<true>* p) {
    MUMPY_REQUIRE(groups >= 1, MUMPY_EINVAL, "%s: groups=%d must be at least 1", who, groups);
    MUMPY_REQUIRE(B % groups == 0, MUMPY_EINVAL, "%s: groups=%d must divide the %lld q windows and the batch %d", who, groups,
                  (long long)nq, B);
    return cva_grouping_windows(who, nkv, nq, groups, p);
}

}  // namespace mumpy
