// The radius decision of a circle candidate without its square root.
//
// filter_circles step 4 (utils.py:157-166) keeps a candidate whose float32 radius rad = sqrtf(s), s = fl(fl(c_row^2) +
// fl(c_col^2)), lies in [min_r, max_r], and files it under irad = rint(rad).  Correctly rounded sqrtf is monotone and so
// is rintf, so both are step functions of s: the range test is  lo <= s <= hi  and irad is the number of thresholds
// T_k = min{ s : rint(sqrtf(s)) >= k } at or below s.  The thresholds are found on the host by bisection over the bit
// patterns of the non-negative floats with the same sqrtf / rintf; a kernel then needs an integer GUESS of the root
// that is off by one at most (the hardware's 1-ulp square root) and two compares against the table.
//
// Plain C++ (no HIP header needed): tests/candidate_radius_main.cpp builds it for the host alone.
#pragma once
#include <math.h>
#include <stdint.h>
#include <string.h>

#if defined(__HIPCC__)
#define MG_RADIUS_HD __host__ __device__ inline
#else
#define MG_RADIUS_HD inline
#endif

constexpr int MG_RADIUS_MAX_LAYERS = 32;  // = MG_KEY_MAX_LAYERS: the radius layers a 32-bit key has

struct MgRadiusTable {
  float lo, hi;                          // sqrtf(s) >= min_r  <=>  s >= lo;   sqrtf(s) <= max_r  <=>  s <= hi
  float t[MG_RADIUS_MAX_LAYERS + 1];     // t[i] = T_(min_r + i), i = 0 .. max_r - min_r + 1
  int min_r, max_r;
};

// The radius decision of a candidate with squared radius s: whether the range test holds (it fails for NaN and +inf:
// every compare with a NaN is false, and hi is finite) and, where it does, the layer irad - min_r in *layer (anything
// where it does not).  `guess` is any float within 1 of sqrtf(s) after rounding to an integer -- sqrtf itself, or an
// approximation of it a few ulp off; what it is for an s out of range does not matter, NaN included: it is clamped
// to [min_r, max_r] first, which moves it no further from an irad that lies in there.  No branch: every lane of a wave
// reads the table.  `t` may be the table's copy in LDS.
MG_RADIUS_HD bool mg_radius_decide(float s, float guess, float lo, float hi, const float* t, int min_r, int max_r,
                                   int* layer) {
#if defined(__HIP_DEVICE_COMPILE__)
  const float g = __builtin_amdgcn_fmed3f(rintf(guess), (float)min_r, (float)max_r);  // (a NaN gives min_r)
#else
  const float g = fminf(fmaxf(rintf(guess), (float)min_r), (float)max_r);
#endif
  const int i = (int)g - min_r;
  *layer = i - (s < t[i] ? 1 : 0) + (s >= t[i + 1] ? 1 : 0);
  return s >= lo && s <= hi;
}
// As one number: the layer, or -1 where the range test fails.
MG_RADIUS_HD int mg_radius_layer(float s, float guess, float lo, float hi, const float* t, int min_r, int max_r) {
  int layer;
  return mg_radius_decide(s, guess, lo, hi, t, min_r, max_r, &layer) ? layer : -1;
}

// ---- host: the table -------------------------------------------------------------------------------
inline float mg_radius_from_bits(uint32_t b) {
  float f;
  memcpy(&f, &b, sizeof f);
  return f;
}

// The smallest non-negative float s (by bit pattern, +inf the last) for which pred(s) holds; pred is monotone (false ..
// false true .. true) and holds at +inf.
template <class Pred>
inline float mg_radius_first(Pred pred) {
  uint32_t lo = 0u, hi = 0x7F800000u;  // the answer is in [lo, hi]
  while (lo < hi) {
    const uint32_t mid = lo + (hi - lo) / 2u;
    if (pred(mg_radius_from_bits(mid))) hi = mid;
    else lo = mid + 1u;
  }
  return mg_radius_from_bits(lo);
}

// 0 <= min_r <= max_r, max_r - min_r < MG_RADIUS_MAX_LAYERS.  `volatile`: the roots are taken at run time, in float32,
// by the library's sqrtf, whatever the host compiler would like to fold or widen.
inline void mg_radius_table(int min_r, int max_r, MgRadiusTable* tab) {
  auto root = [](float s) -> float {
    volatile float v = s;
    volatile float r = sqrtf(v);
    return r;
  };
  tab->min_r = min_r;
  tab->max_r = max_r;
  const float fmin = (float)min_r, fmax = (float)max_r;
  tab->lo = mg_radius_first([&](float s) { return root(s) >= fmin; });
  // the last s with sqrtf(s) <= max_r is the one in front of the first with sqrtf(s) > max_r
  const float above = mg_radius_first([&](float s) { return root(s) > fmax; });
  uint32_t b;
  memcpy(&b, &above, sizeof b);
  tab->hi = mg_radius_from_bits(b - 1u);  // (above > 0: sqrtf(0) = 0 <= max_r)
  for (int i = 0; i <= MG_RADIUS_MAX_LAYERS; ++i) {
    const float k = (float)(min_r + i);
    tab->t[i] = i <= max_r - min_r + 1 ? mg_radius_first([&](float s) { return rintf(root(s)) >= k; }) : INFINITY;
  }
}
