// The per-pixel arithmetic of the flat-field correction (preprocess.py:83-87), once: the correction pass
// (mg_flatfield.hip) and the ROI gather that corrects raw channels on the fly (mg_roi.hip) call the same functions, so
// their pixels agree by construction.
//   out = trunc(((t / fl) * M1) / M2),  t = max(x - dark, 0),  M1, M2 the two maxima of the pixel's group.
// Integer outputs avoid the two float64 divisions: v = t * rk with rk = refined_rcp(fl) * (M1 / M2) agrees with the
// reference's three roundings to ~1e-15 relative, so the truncation is the same unless v lies within 1e-6 of an
// integer -- those (rare) pixels take the exact path (exact_quotient).
#pragma once
#include "mg_common.h"

namespace {

template <typename T>
__device__ __forceinline__ T cast_trunc(double v);
// NumPy's astype from float64 truncates toward zero.
template <>
__device__ __forceinline__ uint8_t cast_trunc<uint8_t>(double v) {
  return (uint8_t)(unsigned int)v;
}
template <>
__device__ __forceinline__ uint16_t cast_trunc<uint16_t>(double v) {
  return (uint16_t)(unsigned int)v;
}
template <>
__device__ __forceinline__ float cast_trunc<float>(double v) {
  return (float)v;
}
template <>
__device__ __forceinline__ double cast_trunc<double>(double v) {
  return v;
}

// the range of flat values the reciprocal paths are valid in
__device__ __forceinline__ bool flat_in_range(double fl) { return fl > 1e-30 && fl < 1e30; }
// the same test on a float32 flat value (the float32 filters of pass 1)
__device__ __forceinline__ bool flat_in_range_f32(float fl) { return fl > 1e-30f && fl < 1e30f; }

// Newton-refined reciprocal of a flat-field value (float32 seed, two steps in float64: ~1e-16).
// Returns 0 when the value is outside the range in which the fast path is valid.
__device__ __forceinline__ double refined_rcp(double fl) {
  if (!flat_in_range(fl)) return 0.0;
  double r = (double)__builtin_amdgcn_rcpf((float)fl);
  r = r * (2.0 - fl * r);
  r = r * (2.0 - fl * r);
  return r;
}

// the reference's own operations, in its order
__device__ __forceinline__ double exact_quotient(double t, double fl, double m1, double m2) {
  double e = t / fl;
  e = e * m1;
  e = e / m2;
  return e;
}

template <typename T>
struct IsIntegral {
  static constexpr bool value = false;
};
template <>
struct IsIntegral<uint8_t> {
  static constexpr bool value = true;
};
template <>
struct IsIntegral<uint16_t> {
  static constexpr bool value = true;
};

// out = trunc(((t / fl) * m1) / m2) for an integer output type.  With r = refined_rcp(fl) != 0 and
// k = m1 / m2, v = t * r * k agrees with the reference's three roundings to ~1e-15 relative, so the
// truncation is the same unless v lies within 1e-6 of an integer -- those (rare) pixels, and every
// non-integer output type, take the exact two-division path.
template <typename T>
__device__ __forceinline__ T correct_pixel(double t, double fl, double r, double m1, double m2, double k, bool fast_ok) {
  if (IsIntegral<T>::value && fast_ok && r != 0.0) {
    if (t == 0.0) return (T)0;  // 0 / fl * m1 / m2 == 0 exactly (m1, m2 finite and positive here)
    const double v = t * r * k;
    const double fv = floor(v);
    const double fr = v - fv;
    if (fr > 1e-6 && fr < 1.0 - 1e-6 && v < 4.0e9) return (T)(unsigned int)fv;
  }
  return cast_trunc<T>(exact_quotient(t, fl, m1, m2));
}

// k = M1 / M2 of a group; whether the fast path holds for these maxima
__device__ __forceinline__ bool group_quotient(double m1, double m2, double& kk) {
  kk = m1 / m2;
  return kk > 0.0 && kk < 1e30 && m1 > 0.0 && m1 < 1e300 && m2 > 0.0 && m2 < 1e300;
}

// A value that is the same in every lane, held in scalar registers (the compiler keeps uniform float64 values in
// vector registers otherwise: 2 per value and lane).
__device__ __forceinline__ double uniform_f64(double v) {
  const unsigned long long u = (unsigned long long)__double_as_longlong(v);
  const uint32_t lo = __builtin_amdgcn_readfirstlane((uint32_t)u), hi = __builtin_amdgcn_readfirstlane((uint32_t)(u >> 32));
  return __longlong_as_double((long long)(((unsigned long long)hi << 32) | lo));
}

// max(x - d, 0) of N integer pixels in the integer domain (d: an integer-valued scalar dark in [0, 65535]); uint16
// pixels two at a time (v_pk_sub_u16 with clamp).
typedef unsigned short mg_u16x2 __attribute__((ext_vector_type(2)));
template <typename T, int N>
__device__ __forceinline__ void sub_dark_int(const T (&x)[N], uint32_t d, uint32_t (&ti)[N]) {
#pragma unroll
  for (int j = 0; j < N; ++j) {
    const uint32_t xi = (uint32_t)x[j];
    ti[j] = xi > d ? xi - d : 0u;
  }
}
template <>
__device__ __forceinline__ void sub_dark_int<uint16_t, 8>(const uint16_t (&x)[8], uint32_t d, uint32_t (&ti)[8]) {
  uint32_t w[4];
  __builtin_memcpy(w, x, 16);
  const mg_u16x2 dd = {(unsigned short)d, (unsigned short)d};
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const mg_u16x2 r = __builtin_elementwise_sub_sat(__builtin_bit_cast(mg_u16x2, w[q]), dd);
    ti[2 * q] = r.x;
    ti[2 * q + 1] = r.y;
  }
}
template <>
__device__ __forceinline__ void sub_dark_int<uint16_t, 2>(const uint16_t (&x)[2], uint32_t d, uint32_t (&ti)[2]) {
  uint32_t w;
  __builtin_memcpy(&w, x, 4);
  const mg_u16x2 dd = {(unsigned short)d, (unsigned short)d};
  const mg_u16x2 r = __builtin_elementwise_sub_sat(__builtin_bit_cast(mg_u16x2, w), dd);
  ti[0] = r.x;
  ti[1] = r.y;
}

// The fast products of a chunk against per-position factors rk = rcp(flat) * (M1 / M2) (made once per position and
// group, not per pixel): v = t * rk agrees with the reference's three roundings to ~1e-15 relative; the integer part
// is the conversion's own truncation (v >= 0), the distance to the next integer comes from v_fract_f64.  Returns
// whether any pixel sits within 1e-6 of an integer (t == 0 gives exactly 0 either way and does not count).
template <typename T, int N>
__device__ __forceinline__ bool fast_chunk_int(const uint32_t (&ti)[N], const double (&rk)[N], T (&o)[N]) {
  bool unsure = false;
#pragma unroll
  for (int j = 0; j < N; ++j) {
    const double v = (double)ti[j] * rk[j];
    const double fr = __builtin_amdgcn_fract(v);
    o[j] = (T)(unsigned int)v;
    unsure |= !(fr > 1e-6 && fr < 1.0 - 1e-6) && ti[j] != 0u;
  }
  return unsure;
}
template <typename T, int N>
__device__ __forceinline__ bool fast_chunk_f64(const double (&t)[N], const double (&rk)[N], T (&o)[N]) {
  bool unsure = false;
#pragma unroll
  for (int j = 0; j < N; ++j) {
    const double v = t[j] * rk[j];
    const double fr = __builtin_amdgcn_fract(v);
    o[j] = (T)(unsigned int)v;
    unsure |= !(fr > 1e-6 && fr < 1.0 - 1e-6) && t[j] != 0.0;
  }
  return unsure;
}

// rk[j] = rr[j] * kk for the positions of a chunk (rr: refined_rcp of the flat values, kk: the group's quotient).
// Returns whether a factor is too large for the fast path: t <= 65535, so v = t rk stays below 4e9 (the unsigned
// conversion) while rk < 61035.
template <int N>
__device__ __forceinline__ bool chunk_factors(const double (&rr)[N], double kk, double (&rk)[N]) {
  bool large = false;
#pragma unroll
  for (int j = 0; j < N; ++j) {
    rk[j] = rr[j] * kk;
    large |= !(rk[j] < 61035.0);
  }
  return large;
}

// N integer pixels of one plane against the factors of their positions: the fast products of all N first
// (straight-line code), ONE test whether any of them sits too close to an integer, and only then -- a few chunks in a
// million, or `rk_bad`: the factors, the flat values or the group's maxima are outside the fast path's range -- the
// reference's own operations with the maxima of group plane / planes_per_group.
// INT_DARK: an integer-valued scalar dark, subtracted in the integer domain (dk is not read); else dk per position.
template <typename T, int N, bool INT_DARK>
__device__ __forceinline__ void correct_chunk_rk(const T (&x)[N], uint32_t dark_i, const double (&dk)[N],
                                                 const double (&fl)[N], const double (&rk)[N], bool rk_bad,
                                                 const double* __restrict__ d_max2, int plane, int planes_per_group,
                                                 T (&o)[N]) {
  bool unsure;
  uint32_t ti[N];
  double t[N];
  if (INT_DARK) {
    sub_dark_int<T, N>(x, dark_i, ti);
    unsure = fast_chunk_int<T, N>(ti, rk, o);
  } else {
#pragma unroll
    for (int j = 0; j < N; ++j) {
      t[j] = (double)x[j] - dk[j];
      t[j] = t[j] < 0.0 ? 0.0 : t[j];
    }
    unsure = fast_chunk_f64<T, N>(t, rk, o);
  }
  if (unsure || rk_bad) {  // a few chunks in a million: the reference's own operations
    const int group = plane / planes_per_group;
    const double m1 = d_max2[2 * group], m2 = d_max2[2 * group + 1];
#pragma unroll
    for (int j = 0; j < N; ++j) {
      const double tj = INT_DARK ? (double)ti[j] : t[j];
      o[j] = cast_trunc<T>(exact_quotient(tj, fl[j], m1, m2));
    }
  }
}

// an integer-valued scalar dark inside the pixel range: subtracted in the integer domain
inline bool dark_is_int(const void* d_dark, double dark) {
  return !d_dark && dark >= 0.0 && dark <= 65535.0 && dark == (double)(uint32_t)dark;
}

}  // namespace
