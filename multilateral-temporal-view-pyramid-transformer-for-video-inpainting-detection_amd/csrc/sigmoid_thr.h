// sigmoid_thr.h — the sigmoid-and-compare expression of the eval tail: final_conv_kernel / final_conv_wide_kernel (decoder.hip) turn a
// logit into the 0 / 1 mask with it, score_exceed_kernel (score_sweep.hip) classifies the same logit against a table of thresholds.
// One definition, so the mask at thr = t and the exceed counts at t compare bit for bit by construction.
#pragma once
#include "common.h"

namespace mumpy {

// The probability the mask is cut from.  NaN stays NaN, and NaN > thr is false: a NaN logit exceeds nothing.
__device__ __forceinline__ float sigmoid_prob(float z) { return 1.0f / (1.0f + __expf(-z)); }

// strict: a probability equal to the threshold is background
__device__ __forceinline__ bool prob_exceeds(float p, float thr) { return p > thr; }

__device__ __forceinline__ bool sigmoid_exceeds(float z, float thr) { return prob_exceeds(sigmoid_prob(z), thr); }

}  // namespace mumpy
