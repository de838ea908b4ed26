// Exact order statistics of masked windows, shared by mg_roi.hip (k_masked_median) and mg_roistats.hip
// (k_masked_stats): the order-preserving key of a pixel and the byte-wise radix select over a window in global memory.
#pragma once
#include "mg_common.h"

// (an unnamed namespace: every file that includes this gets copies of its own, as if it had written them)
namespace {

constexpr int MG_SELECT_THREADS = 256;  // the workgroup size of every kernel that calls select_kth

// Keys are the order-preserving unsigned images of the values: an unsigned integer is its own key, an IEEE float has
// its sign bit flipped (positive) or all bits inverted (negative).  A NaN pixel counts as masked out (nanmedian).
template <typename T> struct median_key;
template <> struct median_key<uint8_t> {
  typedef uint32_t type; static constexpr int LEVELS = 1;
  __device__ static bool key(uint8_t x, uint32_t* k) { *k = x; return true; }
  __device__ static double value(uint32_t k) { return (double)k; }
};
template <> struct median_key<uint16_t> {
  typedef uint32_t type; static constexpr int LEVELS = 2;
  __device__ static bool key(uint16_t x, uint32_t* k) { *k = x; return true; }
  __device__ static double value(uint32_t k) { return (double)k; }
};
template <> struct median_key<float> {
  typedef uint32_t type; static constexpr int LEVELS = 4;
  __device__ static bool key(float x, uint32_t* k) {
    const uint32_t b = __float_as_uint(x);
    *k = (b & 0x80000000u) ? ~b : (b | 0x80000000u);
    return x == x;
  }
  __device__ static double value(uint32_t k) {
    return (double)__uint_as_float((k & 0x80000000u) ? (k & 0x7FFFFFFFu) : ~k);
  }
};
template <> struct median_key<double> {
  typedef uint64_t type; static constexpr int LEVELS = 8;
  __device__ static bool key(double x, uint64_t* k) {
    const uint64_t b = (uint64_t)__double_as_longlong(x);
    *k = (b >> 63) ? ~b : (b | 0x8000000000000000ull);
    return x == x;
  }
  __device__ static double value(uint64_t k) {
    return __longlong_as_double((long long)((k >> 63) ? (k & 0x7FFFFFFFFFFFFFFFull) : ~k));
  }
};

// the k-th smallest (0-based) key among the unmasked, non-NaN values: one 256-bin histogram per key byte, most
// significant first, only the values that share the prefix found so far take part
template <typename T>
__device__ typename median_key<T>::type select_kth(const T* __restrict__ v, const uint8_t* __restrict__ mask, int n,
                                                   int k, uint32_t* hist) {
  typedef typename median_key<T>::type K;
  constexpr int LV = median_key<T>::LEVELS;
  constexpr int NT = MG_SELECT_THREADS;
  __shared__ int s_bin, s_rank;
  K prefix = 0;
  int rank = k;
  for (int level = 0; level < LV; ++level) {
    const int shift = 8 * (LV - 1 - level);
    for (int i = threadIdx.x; i < 256; i += NT) hist[i] = 0;
    __syncthreads();
    for (int p = threadIdx.x; p < n; p += NT) {
      K key;
      if (!mask[p] || !median_key<T>::key(v[p], &key)) continue;
      if (level == 0 || (key >> (shift + 8)) == prefix) atomicAdd(&hist[(uint32_t)(key >> shift) & 255u], 1u);
    }
    __syncthreads();
    if (threadIdx.x == 0) {
      int acc = 0, b = 0;
      for (; b < 255; ++b) {
        if (acc + (int)hist[b] > rank) break;
        acc += hist[b];
      }
      s_bin = b;
      s_rank = rank - acc;
    }
    __syncthreads();
    prefix = (prefix << 8) | (K)s_bin;
    rank = s_rank;
    __syncthreads();
  }
  return prefix;
}

}  // namespace
