// What the stitch passes share (mg_flatfield.hip: crop / concat; mg_blend.hip: the same with the seams blended): the
// chunk of N pixels a lane handles, its 16-byte accesses, the dark / flat operands of a chunk and the launch grid.
#pragma once
#include <algorithm>

#include "mg_common.h"

namespace {

template <typename T>
struct VecOf;
template <>
struct VecOf<uint8_t> {
  static constexpr int N = 16;
};
template <>
struct VecOf<uint16_t> {
  static constexpr int N = 8;
};
template <>
struct VecOf<float> {
  static constexpr int N = 4;
};
template <>
struct VecOf<double> {
  static constexpr int N = 2;
};

// Load N consecutive elements; one 16-byte load when the address is aligned.
template <typename T, int N>
__device__ __forceinline__ void load_vec(const T* p, T (&v)[N]) {
  if ((reinterpret_cast<uintptr_t>(p) & 15) == 0) {
    const uint4 raw = *reinterpret_cast<const uint4*>(p);
    __builtin_memcpy(v, &raw, 16);
  } else {
#pragma unroll
    for (int j = 0; j < N; ++j) v[j] = p[j];
  }
}
template <typename T, int N>
__device__ __forceinline__ void store_vec(T* p, const T (&v)[N]) {
  if ((reinterpret_cast<uintptr_t>(p) & 15) == 0) {
    uint4 raw;
    __builtin_memcpy(&raw, v, 16);
    *reinterpret_cast<uint4*>(p) = raw;
  } else {
#pragma unroll
    for (int j = 0; j < N; ++j) p[j] = v[j];
  }
}

// N consecutive dark/flat operands as float64 (image of float32/float64, or the scalar).
template <int N>
__device__ __forceinline__ void load_field(const void* __restrict__ img, int dt, int64_t p, double scalar,
                                           double (&out)[N]) {
  if (!img) {
#pragma unroll
    for (int j = 0; j < N; ++j) out[j] = scalar;
  } else if (dt == MG_F32) {
    const float* f = (const float*)img + p;
    if ((N % 4) == 0 && (reinterpret_cast<uintptr_t>(f) & 15) == 0) {
#pragma unroll
      for (int q = 0; q < N / 4; ++q) {
        const float4 v = reinterpret_cast<const float4*>(f)[q];
        out[4 * q] = v.x;
        out[4 * q + 1] = v.y;
        out[4 * q + 2] = v.z;
        out[4 * q + 3] = v.w;
      }
    } else {
#pragma unroll
      for (int j = 0; j < N; ++j) out[j] = f[j];
    }
  } else {
    const double* d = (const double*)img + p;
#pragma unroll
    for (int j = 0; j < N; ++j) out[j] = d[j];
  }
}

constexpr int ROWS_PER_BLOCK = 32;  // rows of a workgroup at large batches; fewer when the grid would not fill the chip
constexpr int PLANES_PER_BLOCK = 8;

// The grid of a stitch pass (256 lanes x N pixels wide, `rows` output rows per row group, PLANES_PER_BLOCK planes deep)
// and its rows per row group.
template <int N>
inline dim3 stitch_grid(int h_out, int w_out, int64_t n_planes, int& rows) {
  // rows per workgroup: 32 when that still gives ~8 workgroups per CU, down to 2 for a single assay
  rows = ROWS_PER_BLOCK;
  const int64_t cols_planes = (int64_t)((w_out + 256 * N - 1) / (256 * N)) * ((n_planes + PLANES_PER_BLOCK - 1) / PLANES_PER_BLOCK);
  while (rows > 2 && cols_planes * ((h_out + rows - 1) / rows) < 2048) rows /= 2;
  // ... and at most ~1024 workgroups per plane group walk them (each ends with min/max atomics on the plane's one
  // cache line: 2048 workgroups finishing together took 100 us over them)
  int y_blocks = (h_out + rows - 1) / rows;
  if (rows < ROWS_PER_BLOCK) y_blocks = (int)std::min<int64_t>(y_blocks, std::max<int64_t>(1, 1024 / std::max<int64_t>(1, cols_planes)));
  return dim3((w_out + 256 * N - 1) / (256 * N), y_blocks, (unsigned)((n_planes + PLANES_PER_BLOCK - 1) / PLANES_PER_BLOCK));
}

}  // namespace
