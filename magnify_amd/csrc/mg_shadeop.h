// The per-pixel arithmetic of the shading apply, once: v = (x - dark) / flat, IEEE operations, integer outputs clamped
// to [0, max] and truncated.  mg_shading.hip (apply fused with the stitch crop) and mg_blend.hip (the same with the
// seams blended) call the same functions, so their pixels agree by construction.
#pragma once
#include "mg_common.h"

namespace {

template <typename T>
struct ShadeOp {
  static constexpr bool kInt = true;
  static constexpr float kMax = 255.0f;
  __device__ static T apply(T x, float dk, float fl) {
    float v = ((float)x - dk) / fl;
    v = v > 0.0f ? v : 0.0f;
    v = v < kMax ? v : kMax;
    return (T)(uint32_t)v;
  }
};
template <>
struct ShadeOp<uint16_t> {
  static constexpr bool kInt = true;
  __device__ static uint16_t apply(uint16_t x, float dk, float fl) {
    float v = ((float)x - dk) / fl;
    v = v > 0.0f ? v : 0.0f;
    v = v < 65535.0f ? v : 65535.0f;
    return (uint16_t)(uint32_t)v;
  }
};
template <>
struct ShadeOp<float> {
  static constexpr bool kInt = false;
  __device__ static float apply(float x, float dk, float fl) { return (x - dk) / fl; }
};
template <>
struct ShadeOp<double> {
  static constexpr bool kInt = false;
  __device__ static double apply(double x, float dk, float fl) { return (x - (double)dk) / (double)fl; }
};

}  // namespace
