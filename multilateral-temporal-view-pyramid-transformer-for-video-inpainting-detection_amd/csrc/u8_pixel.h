// u8_pixel.h — the pixel expression of the uint8 staging kernels that gather through x tables: resize_normalize_u8_kernel (norm.hip)
// and clip_window_u8_kernel (video_stage.hip).  One definition, so the two compare bit for bit by construction.
#pragma once
#include "common.h"

namespace mumpy {

// ToTensor + Normalize of one 8-bit value (torchvision: u8 / 255, then (v - mean) / std), in this order.
__device__ __forceinline__ float normalize_u8_value(uint8_t v, float mean, float stdv) { return ((float)v / 255.0f - mean) / stdv; }

// Four consecutive output pixels of one channel: `row` points at that channel of source pixel 0 of the source row (pixels are 3
// bytes apart), xi holds the four source columns.
__device__ __forceinline__ f32x4 normalize_u8_gather4(const uint8_t* __restrict__ row, int4 xi, float mean, float stdv) {
    f32x4 v;
    v[0] = normalize_u8_value(row[3 * (int64_t)xi.x], mean, stdv);
    v[1] = normalize_u8_value(row[3 * (int64_t)xi.y], mean, stdv);
    v[2] = normalize_u8_value(row[3 * (int64_t)xi.z], mean, stdv);
    v[3] = normalize_u8_value(row[3 * (int64_t)xi.w], mean, stdv);
    return v;
}

}  // namespace mumpy
