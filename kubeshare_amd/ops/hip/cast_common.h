// f32 <-> bf16 conversion with torch's rounding
// (c10::detail::round_to_nearest_even): round to nearest even, every NaN
// becomes the canonical quiet NaN 0x7FC0. Shared by cast.hip and
// grad_bucket.hip. The f32_to_bf16 helper of bn_relu.hip is NOT that (a
// NaN whose payload sits in the low mantissa bits comes out as inf
// there).
#pragma once
#include <hip/hip_runtime.h>

__device__ __forceinline__ unsigned short cast_f32_to_bf16(float f) {
  union {
    float f;
    unsigned int i;
  } v;
  v.f = f;
  if ((v.i & 0x7fffffffu) > 0x7f800000u) return 0x7FC0;  // any NaN
  v.i += 0x7fffu + ((v.i >> 16) & 1);
  return (unsigned short)(v.i >> 16);
}

__device__ __forceinline__ float cast_bf16_to_f32(unsigned short u) {
  union {
    unsigned int i;
    float f;
  } v;
  v.i = ((unsigned int)u) << 16;
  return v.f;
}
