// Stitch with linear overlap blending ("stitch: linear overlap blending"): the crop / concat of
// mg_flatfield.hip with every inner seam feathered -- inside the band of `overlap` pixels around a seam a pixel is the
// linear mix of the two tiles that cover it, of the four where a row band and a column band cross.  One pass: the
// pending correction (flat-field or shading, the per-pixel code of mg_flatcorr.h / mg_shadeop.h), the crop / concat,
// the mix and the per-plane min / max of the BLENDED values.
//
// Per axis (tile length t, overlap v, c = v / 2, r = v % 2, h = t - v, n tiles; canvas o, owner i = o / h,
// j = o - i h, local p = j + c):
//   v > 0, i > 0,     j < c + r : k = j + c:        tile i at p with numerator 2k + 1, tile i - 1 at p + h with 2v - (2k + 1)
//   v > 0, i < n - 1, j >= h - c: k = j - (h - c):  tile i at p with 2v - (2k + 1),    tile i + 1 at p - h with 2k + 1
//   else                        : tile i alone, numerator 2v.
// The two cases exclude each other while 2v <= t (the entries refuse anything else).
// Integer pixels: out = (sum ny nx value + D / 2) / D, D = (2v)^2, in 64-bit integers.  Float pixels, in float64:
// a = c0 (nx0 / 2v) + c1 (nx1 / 2v) along x for each contributing row, then the rows the same way along y, then the
// cast; a term without a second tile is not formed.
//
// The kernel is the generic one with BLEND on, k_stitch<T, MODE, true, false> (mg_stitch_kernel.h).
//
// Roofline: HBM, as the plain pass.  A chunk of N pixels that touches no band is the plain pass's chunk: one 16-byte
// load per plane, the dark / flat operands loaded once for the PLANES_PER_BLOCK planes of the workgroup.  A row band is
// a whole output row (workgroup-uniform); a column band is a range of lanes: those lanes go on, pixel by pixel, to
// the second (or the three other) tiles and their operands while the rest of the wave waits for them.
#include <math.h>

#include "mg_stitch_kernel.h"

namespace {

inline bool blend_shape_ok(int n_tr, int n_tc, int ty, int tx, int overlap) {
  // 2 overlap <= tile: a pixel lies in at most one band per axis
  return n_tr > 0 && n_tc > 0 && ty > 0 && tx > 0 && overlap >= 0 && 2 * (int64_t)overlap <= ty && 2 * (int64_t)overlap <= tx;
}

}  // namespace

extern "C" int mg_flatfield_apply_stitch_blend(const void* d_tiles, int dtype, int64_t n_planes, int n_tile_rows,
                                               int n_tile_cols, int ty, int tx, int overlap, int apply_flatfield,
                                               int planes_per_group, double dark, const void* d_dark, int dark_dtype,
                                               double flat, const void* d_flat, int flat_dtype, const double* d_max2,
                                               void* d_image, double* d_minmax, void* stream) {
  if (!blend_shape_ok(n_tile_rows, n_tile_cols, ty, tx, overlap)) return MG_EINVAL;
  hipStream_t s = mg_stream(stream);
  return flatfield_stitch_entry(
      d_tiles, dtype, n_planes, n_tile_rows, n_tile_cols, ty, tx, apply_flatfield, planes_per_group, dark, d_dark, dark_dtype,
      flat, d_flat, flat_dtype, d_max2, d_image, [&](const auto& src, auto mode) {
        return launch_stitch<decltype(mode)::value, true, false>(src, n_planes, overlap, PlaneSel{}, d_image, d_minmax, s);
      });
}

extern "C" int mg_shading_apply_stitch_blend(const void* d_tiles, int dtype, int n_fields, int64_t planes_per_field,
                                             int n_tile_rows, int n_tile_cols, int ty, int tx, int overlap,
                                             const float* d_flat, const float* d_dark, void* d_image, double* d_minmax,
                                             void* stream) {
  if (!blend_shape_ok(n_tile_rows, n_tile_cols, ty, tx, overlap)) return MG_EINVAL;
  hipStream_t s = mg_stream(stream);
  return shading_stitch_entry(d_tiles, dtype, n_fields, planes_per_field, n_tile_rows, n_tile_cols, ty, tx, d_flat, d_dark,
                              d_image, [] { return (int)MG_OK; }, [&](const auto& src, int64_t n_planes) {
                                return launch_stitch<BL_SHADE, true, false>(src, n_planes, overlap, PlaneSel{}, d_image,
                                                                            d_minmax, s);
                              });
}
