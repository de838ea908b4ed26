// Exact order statistics: the order-preserving key of a pixel (k_masked_stats in mg_roistats.hip, pc_key in
// mg_percentile.hip) and the byte-wise radix select over the keys of a window, wherever they lie.  And the chunk loader
// of the kernels that stream whole ROI windows (k_masked_stats, k_radial_profile in mg_profile.hip).
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

// A chunk as it comes from memory: VW pixels (16 bytes of them, or one) and their mask bytes, byte j in mw[j / 4].
// Pixels beyond the window have mask byte 0.  MASKED = false: there is no mask to read, every pixel of the window has
// byte 1.
template <typename T, int VW>
struct RawChunk {
  T px[VW];
  uint32_t mw[4];
};
// VW (2, 4, 8 or 16) bytes from p, which is aligned to VW, as one load: byte j in w[j / 4].
template <int VW>
__device__ __forceinline__ void load_bytes(const uint8_t* p, uint32_t* w) {
  if constexpr (VW == 16) {
    const uint4 t = *reinterpret_cast<const uint4*>(p);
    w[0] = t.x, w[1] = t.y, w[2] = t.z, w[3] = t.w;
  } else if constexpr (VW == 8) {
    const uint2 t = *reinterpret_cast<const uint2*>(p);
    w[0] = t.x, w[1] = t.y;
  } else if constexpr (VW == 4) {
    w[0] = *reinterpret_cast<const uint32_t*>(p);
  } else {
    w[0] = *reinterpret_cast<const uint16_t*>(p);
  }
}
template <typename T, int VW, bool MASKED = true>
__device__ __forceinline__ RawChunk<T, VW> fetch(const T* __restrict__ v, const uint8_t* __restrict__ mask, int n, int c,
                                                 int end) {
  RawChunk<T, VW> r = {};
  if (c >= end) return r;
  if (VW > 1 && (c + 1) * VW <= n) {
    const uint4 bits = *reinterpret_cast<const uint4*>(v + (int64_t)c * VW);
    __builtin_memcpy(r.px, &bits, 16);
    const uint8_t* mp = mask + (int64_t)c * VW;
    if constexpr (!MASKED) {
#pragma unroll
      for (int j = 0; j < VW; j += 4) r.mw[j >> 2] = VW >= 4 ? 0x01010101u : 0x0101u;
    } else {
      load_bytes<VW>(mp, r.mw);
    }
  } else {  // VW = 1, or the window's last, partial chunk
#pragma unroll
    for (int j = 0; j < VW; ++j) {
      const int p = c * VW + j;
      if (p < n) r.px[j] = v[p], r.mw[j >> 2] |= (uint32_t)(MASKED ? mask[p] : (uint8_t)1) << (8 * (j & 3));
    }
  }
  return r;
}

// The k-th smallest (0-based) of the keys of `count` items: one 256-bin histogram per key byte, most significant first,
// only the keys that share the prefix found so far take part.  key_at(i, &key) gives the key of item i, false where it
// has none (masked out, NaN); k < the number of items that have one.  The bin that holds the rank is picked by wave 0:
// four bins a lane, a scan of the lanes' totals, then the bin inside one lane.  hist[256] is all zero on entry and on
// return; s_pick[2] is written only behind the first barrier of a call, when every thread has read the last call's.
// Called by all MG_SELECT_THREADS threads (it synchronises).
template <typename K, int LV, class KeyAt>
__device__ __forceinline__ K select_kth(int count, KeyAt key_at, int k, uint32_t* hist, int* s_pick) {
  const int lane = threadIdx.x & 63;
  K prefix = 0;
  int rank = k;
  for (int level = 0; level < LV; ++level) {
    const int shift = 8 * (LV - 1 - level);
    for (int i = threadIdx.x; i < count; i += MG_SELECT_THREADS) {
      K key;
      if (!key_at(i, &key)) continue;
      if (level == 0 || (key >> (shift + 8)) == prefix) atomicAdd(&hist[(uint32_t)(key >> shift) & 255u], 1u);
    }
    __syncthreads();
    if (threadIdx.x < 64) {
      uint32_t h[4];
#pragma unroll
      for (int j = 0; j < 4; ++j) h[j] = hist[4 * lane + j], hist[4 * lane + j] = 0u;
      const int total = (int)(h[0] + h[1] + h[2] + h[3]);
      const int incl = mg_wave_scan_incl_i32(total);
      const unsigned long long reached = __ballot(incl > rank);
      const int owner = reached ? __ffsll((long long)reached) - 1 : 63;  // (rank < the keys counted: some lane reaches it)
      if (lane == owner) {
        int acc = incl - total, b = 0;
#pragma unroll
        for (; b < 3; ++b) {
          if (acc + (int)h[b] > rank) break;
          acc += (int)h[b];
        }
        s_pick[0] = 4 * lane + b;
        s_pick[1] = rank - acc;
      }
    }
    __syncthreads();
    prefix = (prefix << 8) | (K)s_pick[0];
    rank = s_pick[1];
  }
  return prefix;
}

}  // namespace
