// The per-pixel pieces of the blended stitch, once: which tiles cover a canvas coordinate and with what numerators
// (Axis, axis_term), what the plain pass writes for one pixel of one tile (tile_value, from the StitchSrc of
// mg_stitch.h) and the mix of up to four such values (mix_tiles).  The generic kernel (mg_stitch_kernel.h, blended in
// mg_blend.hip) and mg_register.hip (the stitch of shifted tiles) call the same functions, so their pixels agree by
// construction.
#pragma once
#include "mg_common.h"
#include "mg_flatcorr.h"
#include "mg_shadeop.h"
#include "mg_stitch.h"

namespace {

struct Axis {
  int v, clip, rem, h, n;
};
// Owner tile i, offset j in its kept part: the other tile of the mix (-1: the one before, +1: the one after, 0: none)
// and the owner's numerator (the other tile's is 2v - num).
__device__ __forceinline__ void axis_term(const Axis& a, int i, int j, int& other, int& num) {
  other = 0;
  num = 2 * a.v;
  if (a.v > 0 && i > 0 && j < a.clip + a.rem) {
    other = -1;
    num = 2 * (j + a.clip) + 1;
  } else if (a.v > 0 && i < a.n - 1 && j >= a.h - a.clip) {
    other = 1;
    num = 2 * a.v - (2 * (j - (a.h - a.clip)) + 1);
  }
}

// What the plain pass writes for pixel (y, x) of tile (tr, tc) of `plane`.
template <typename T, int MODE>
__device__ __forceinline__ T tile_value(const StitchSrc<T>& s, int plane, int tr, int tc, int y, int x,
                                        const GroupMax& g) {
  const int64_t tile_elems = (int64_t)s.ty * s.tx, pix = (int64_t)y * s.tx + x;
  const T px = s.tiles[(((int64_t)plane * s.n_tr + tr) * s.n_tc + tc) * tile_elems + pix];
  if (MODE == BL_COPY) return px;
  if (MODE == BL_SHADE) {
    const int64_t f = (int64_t)(plane / s.planes_per_group) * tile_elems + pix;
    return ShadeOp<T>::apply(px, ((const float*)s.d_dark)[f], ((const float*)s.d_flat)[f]);
  }
  const double dk = s.d_dark ? mg_load_f64(s.d_dark, s.dark_dt, pix) : s.dark;
  const double fl = s.d_flat ? mg_load_f64(s.d_flat, s.flat_dt, pix) : s.flat;
  double t = (double)px - dk;
  t = t < 0.0 ? 0.0 : t;
  return correct_pixel<T>(t, fl, IsIntegral<T>::value ? refined_rcp(fl) : 0.0, g.m1, g.m2, g.kk, g.fast_ok);
}

// The mix of the owner's value c00 with the x neighbour's c01, the y neighbour's c10 and the diagonal tile's c11
// (nx, ny: the owner's numerators).
template <typename T>
__device__ __forceinline__ T mix_tiles(T c00, T c01, T c10, T c11, bool has_x, bool has_y, int nx, int ny, int v) {
  if (IsIntegral<T>::value) {
    const uint64_t two_v = 2 * (uint64_t)v, D = two_v * two_v, nx1 = two_v - nx, ny1 = two_v - ny;
    uint64_t acc = (uint64_t)ny * nx * (uint64_t)c00;
    if (has_x) acc += (uint64_t)ny * nx1 * (uint64_t)c01;
    if (has_y) acc += ny1 * nx * (uint64_t)c10;
    if (has_x && has_y) acc += ny1 * nx1 * (uint64_t)c11;
    return (T)((acc + D / 2) / D);
  }
  const double d = 2.0 * (double)v;
  double a0 = (double)c00, a1 = (double)c10;
  if (has_x) {
    const double w0 = (double)nx / d, w1 = (double)(2 * v - nx) / d;
    a0 = (double)c00 * w0 + (double)c01 * w1;
    a1 = (double)c10 * w0 + (double)c11 * w1;
  }
  if (has_y) a0 = a0 * ((double)ny / d) + a1 * ((double)(2 * v - ny) / d);
  return cast_trunc<T>(a0);
}

}  // namespace
