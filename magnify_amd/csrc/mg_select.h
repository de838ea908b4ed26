// Exact order statistics: the order-preserving key of a pixel (k_masked_stats in mg_roistats.hip, pc_key in
// mg_percentile.hip), the byte-wise radix select over the keys of a window, wherever they lie (select_kth), the next
// key up from a selected one (next_above) and the walk over a list of fractions that both quantile kernels take
// (order_pairs: k_masked_stats, k_unmix_stats in mg_unmix.hip).  What the kernels that stream whole ROI windows share
// beyond that is mg_windows.h.
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

// sorted[rank + 1] from below = sorted[rank], in one pass over the items instead of one pass per key byte: `below`
// again where more than rank + 1 keys are <= it, else the smallest key above it (there is one: rank + 1 < the number of
// items that have a key).  each(see) calls see(key) for every key of this thread's items, wherever the kernel keeps
// them -- a kernel with two key sources has its two loops there, in front of one pair of folds.  Called by all
// MG_SELECT_THREADS threads (mg_block_fold synchronises); the same key in every thread.
template <typename K, class Each>
__device__ __forceinline__ K next_above(K below, int rank, Each each) {
  int le = 0;
  K above = ~(K)0;
  each([&](K key) {
    if (key <= below) ++le;
    else above = key < above ? key : above;
  });
  const int le_all = mg_block_fold(le, [](int a, int b) { return a + b; });
  const K above_all = mg_block_fold(above, [](K a, K b) { return a < b ? a : b; });
  return le_all > rank + 1 ? below : above_all;
}

// NaN in the 2 n_q places of a window's order statistics: nothing takes part.  Called by all threads.
__device__ __forceinline__ void order_pairs_of_none(int n_q, double* order) {
  for (int i = threadIdx.x; i < 2 * n_q; i += MG_SELECT_THREADS) order[i] = MG_QNAN;
}

// sorted[lo], sorted[hi] of every fraction q[j], j < n_q, of `count` keys of pixel type T, as values: pos =
// (count - 1) q, lo = the floor of pos, hi = min(lo + 1, count - 1); order[2 j] and order[2 j + 1], written by thread
// 0, NaN in all 2 n_q where count is 0 (order_pairs_of_none).  select(rank) gives sorted[rank]; next(below, rank)
// gives sorted[rank + 1] from below = sorted[rank] -- next_above, or a second select.  The last rank found is kept:
// hi of one q is often lo of the next, or lo itself.  Called by all threads with block-uniform arguments (select and
// next synchronise).
template <typename T, class Select, class Next>
__device__ __forceinline__ void order_pairs(int count, const double* q, int n_q, Select select, Next next, double* order) {
  typedef typename median_key<T>::type K;
  if (count == 0) return order_pairs_of_none(n_q, order);
  int have_rank = -1;
  K have_key = 0;
  for (int j = 0; j < n_q; ++j) {
    const double pos = (double)(count - 1) * q[j];
    const int lo = (int)floor(pos), hi = min(lo + 1, count - 1);
    if (lo != have_rank) have_key = select(lo);
    const K key_lo = have_key;
    if (hi != lo) have_key = next(key_lo, lo);
    have_rank = hi;
    if (threadIdx.x == 0) {
      order[2 * j] = median_key<T>::value(key_lo);
      order[2 * j + 1] = median_key<T>::value(have_key);
    }
  }
}

}  // namespace
