// The median of N keys held in registers (N odd), by compare-exchanges only: "forgetful selection".  Of any N / 2 + 2
// of the keys neither the smallest nor the largest can be the median, so both are dropped and the next key is taken
// in, until three are left; their middle one is the median (rank N / 2 of the ascending sort).  Every index is a
// compile-time constant once the loops are unrolled: the keys never leave the registers.  20 exchanges for N = 9, 132
// for N = 25.  For a 3 x 3 window whose rows are kept sorted there is a shorter way (mg_net_median9_rows).  All of it
// is min / max: right for all inputs if right for all inputs of zeros and ones.
#pragma once
#include "mg_common.h"

namespace {

template <class K>
__host__ __device__ __forceinline__ void mg_net_cx(K& a, K& b) {  // a <= b afterwards
  const K lo = a < b ? a : b, hi = a < b ? b : a;
  a = lo;
  b = hi;
}

// The smallest of v[lo .. hi] to v[lo], the largest to v[hi]; the others stay in between, in some order.
template <class K>
__host__ __device__ __forceinline__ void mg_net_minmax(K* v, int lo, int hi) {
  const int m = hi - lo + 1;
#pragma unroll
  for (int i = 0; i < m / 2; ++i) mg_net_cx(v[lo + i], v[hi - i]);  // the minimum is now in the lower half ...
#pragma unroll
  for (int i = lo + 1; i <= lo + (m - 1) / 2; ++i) mg_net_cx(v[lo], v[i]);
#pragma unroll
  for (int i = hi - 1; i >= hi - (m - 1) / 2; --i) mg_net_cx(v[i], v[hi]);  // ... the maximum in the upper one
}

template <class K, int N>
__host__ __device__ __forceinline__ K mg_net_median(const K* in) {
  static_assert(N % 2 == 1 && N >= 3, "an odd number of keys");
  constexpr int S = N / 2 + 2;
  K v[S];
#pragma unroll
  for (int i = 0; i < S; ++i) v[i] = in[i];
#pragma unroll
  for (int lo = 0; lo <= S - 3; ++lo) {
    mg_net_minmax(v, lo, S - 1);
    if (lo < S - 3) v[S - 1] = in[S + lo];  // the largest is forgotten: its place takes the next key
  }
  return v[S - 2];
}

// a <= b <= c afterwards (32-bit keys: one min3, one med3, one max3).
template <class K>
__host__ __device__ __forceinline__ void mg_net_sort3(K& a, K& b, K& c) {
  const K lo = a < b ? a : b, hi = a < b ? b : a;
  const K top = hi < c ? c : hi, rest = hi < c ? hi : c;
  a = lo < rest ? lo : rest;
  b = lo < rest ? rest : lo;
  c = top;
}
template <class K>
__host__ __device__ __forceinline__ K mg_net_med3(K a, K b, K c) {
  const K lo = a < b ? a : b, hi = a < b ? b : a;
  const K rest = hi < c ? hi : c;
  return lo < rest ? rest : lo;
}
// The median of nine keys given as three sorted rows (lo[i] <= mid[i] <= hi[i]): the largest of the rows' smallest, the
// middle one of their middle ones and the smallest of their largest are the only candidates; it is their middle one.
template <class K>
__host__ __device__ __forceinline__ K mg_net_median9_rows(const K* lo, const K* mid, const K* hi) {
  const K a = lo[0] < lo[1] ? lo[1] : lo[0], top_lo = a < lo[2] ? lo[2] : a;
  const K b = hi[0] < hi[1] ? hi[0] : hi[1], low_hi = b < hi[2] ? b : hi[2];
  return mg_net_med3(top_lo, mg_net_med3(mid[0], mid[1], mid[2]), low_hi);
}

}  // namespace
