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
// Roofline: HBM, as the plain pass.  A chunk of N pixels that touches no band is the plain pass's chunk: one 16-byte
// load per plane, the dark / flat operands loaded once for the PLANES_PER_BLOCK planes of the workgroup.  A row band is
// a whole output row (workgroup-uniform); a column band is a range of lanes: those lanes go on, pixel by pixel, to
// the second (or the three other) tiles and their operands while the rest of the wave waits for them.
#include <math.h>

#include "mg_blendop.h"
#include "mg_common.h"
#include "mg_flatcorr.h"
#include "mg_shadeop.h"
#include "mg_stitch.h"

namespace {

// Block = 256 lanes x N pixels of `rows_per_block` output rows, for PLANES_PER_BLOCK consecutive planes, as
// k_apply_stitch (mg_flatfield.hip); the chunk of a lane is first made as there, then its band pixels are mixed.
template <typename T, int MODE>
__global__ __launch_bounds__(256) void k_blend_stitch(BlendSrc<T> s, int n_planes, int v, int hy, int hx,
                                                       T* __restrict__ image, double* __restrict__ d_minmax,
                                                       int rows_per_block) {
  constexpr int N = VecOf<T>::N;
  constexpr int PB = PLANES_PER_BLOCK;
  const int clip = v / 2, rem = v % 2, n_tr = s.n_tr, n_tc = s.n_tc, tx = s.tx;
  const Axis ay{v, clip, rem, hy, n_tr}, ax{v, clip, rem, hx, n_tc};
  const int plane0 = blockIdx.z * PB;
  const int np = min(PB, n_planes - plane0);
  const int h_out = n_tr * hy, w_out = n_tc * hx;
  const int ox0 = (blockIdx.x * blockDim.x + threadIdx.x) * N;
  double m1[PB], m2[PB], kk[PB];
  bool fast_ok[PB];
#pragma unroll
  for (int b = 0; b < PB; ++b) {
    m1[b] = 0.0, m2[b] = 1.0, kk[b] = 1.0, fast_ok[b] = false;
    if (MODE == BL_FLAT && b < np) {
      const int group = (plane0 + b) / s.planes_per_group;
      m1[b] = s.d_max2[2 * group];
      m2[b] = s.d_max2[2 * group + 1];
      fast_ok[b] = group_quotient(m1[b], m2[b], kk[b]);
    }
  }
  double vmin[PB], vmax[PB];
  uint32_t imin[PB], imax[PB];  // integer outputs: min/max in integer registers
#pragma unroll
  for (int b = 0; b < PB; ++b) vmin[b] = INFINITY, vmax[b] = -INFINITY, imin[b] = 0xFFFFFFFFu, imax[b] = 0u;
  const int64_t tile_elems = (int64_t)s.ty * tx;
  if (ox0 < w_out) {
    const int tc0 = ox0 / hx;
    const int x0 = ox0 - tc0 * hx + clip;
    const bool one_tile = (ox0 + N <= w_out) && (x0 - clip + N <= hx);
    const int cnt = one_tile ? N : min(N, w_out - ox0);
    bool col_band = false;  // a pixel of this chunk lies in a column band
#pragma unroll
    for (int j = 0; j < N; ++j) {
      const int ox = ox0 + min(j, cnt - 1), tc = ox / hx;
      int other, num;
      axis_term(ax, tc, ox - tc * hx, other, num);
      col_band |= other != 0;
    }
    for (int yg = blockIdx.y; yg * rows_per_block < h_out; yg += gridDim.y) {  // (as in k_apply_stitch)
      const int row_end = min((yg + 1) * rows_per_block, h_out);
      for (int oy = yg * rows_per_block; oy < row_end; ++oy) {
        const int tr = oy / hy;
        const int y = oy - tr * hy + clip;
        int oth_y, ny;  // (the same in every lane: a row band is a whole row)
        axis_term(ay, tr, y - clip, oth_y, ny);
        int64_t pix[N], toff[N];  // pixel index inside the tile, element offset of the tile in a plane
#pragma unroll
        for (int j = 0; j < N; ++j) {
          const int ox = ox0 + (one_tile ? j : min(j, cnt - 1));
          const int tc = one_tile ? tc0 : ox / hx;
          const int xx = one_tile ? x0 + j : ox - tc * hx + clip;
          pix[j] = (int64_t)y * tx + xx;
          toff[j] = ((int64_t)tr * n_tc + tc) * tile_elems;
        }
        double dk[N], fl[N], rr[N];
        // the operands of the chunk, shared by the planes that use the same fields (BL_FLAT: all of them)
        auto load_operands = [&](const void* dptr, const void* fptr) {
          if (one_tile) {
            load_field<N>(dptr, s.dark_dt, pix[0], s.dark, dk);
            load_field<N>(fptr, s.flat_dt, pix[0], s.flat, fl);
          } else {
#pragma unroll
            for (int j = 0; j < N; ++j) {
              dk[j] = dptr ? mg_load_f64(dptr, s.dark_dt, pix[j]) : s.dark;
              fl[j] = fptr ? mg_load_f64(fptr, s.flat_dt, pix[j]) : s.flat;
            }
          }
#pragma unroll
          for (int j = 0; j < N; ++j) rr[j] = (MODE == BL_FLAT && IsIntegral<T>::value) ? refined_rcp(fl[j]) : 0.0;
        };
        if (MODE == BL_FLAT) load_operands(s.d_dark, s.d_flat);
        int field_loaded = -1;
#pragma unroll
        for (int b = 0; b < PB; ++b) {
          if (b >= np) break;
          const int plane = plane0 + b;
          if (MODE == BL_SHADE) {
            const int field = plane / s.planes_per_group;
            if (field != field_loaded) {  // (uniform)
              field_loaded = field;
              load_operands((const float*)s.d_dark + (int64_t)field * tile_elems,
                            (const float*)s.d_flat + (int64_t)field * tile_elems);
            }
          }
          const int64_t plane_base = (int64_t)plane * n_tr * n_tc * tile_elems;
          T x[N], o[N];
          if (one_tile) {
            load_vec<T, N>(s.tiles + plane_base + toff[0] + pix[0], x);
          } else {
#pragma unroll
            for (int j = 0; j < N; ++j) x[j] = s.tiles[plane_base + toff[j] + pix[j]];
          }
#pragma unroll
          for (int j = 0; j < N; ++j) {
            if (MODE == BL_FLAT) {
              double t = (double)x[j] - dk[j];
              t = t < 0.0 ? 0.0 : t;
              o[j] = correct_pixel<T>(t, fl[j], rr[j], m1[b], m2[b], kk[b], fast_ok[b]);
            } else if (MODE == BL_SHADE) {
              o[j] = ShadeOp<T>::apply(x[j], (float)dk[j], (float)fl[j]);
            } else {
              o[j] = x[j];
            }
          }
          if (oth_y != 0 || col_band) {
            // band pixels one by one (j is the same in every lane: o[j] is picked with selects, not indexed)
#pragma unroll 1
            for (int j = 0; j < cnt; ++j) {
              const int ox = ox0 + j, tc = ox / hx, xx = ox - tc * hx + clip;
              int oth_x, nx;
              axis_term(ax, tc, xx - clip, oth_x, nx);
              if (oth_x == 0 && oth_y == 0) continue;
              T c00 = o[0], c01 = (T)0, c10 = (T)0, c11 = (T)0;
#pragma unroll
              for (int jj = 1; jj < N; ++jj) c00 = jj == j ? o[jj] : c00;
              const int tr1 = tr + oth_y, y1 = y - oth_y * hy, tc1 = tc + oth_x, x1 = xx - oth_x * hx;
#pragma unroll 1
              for (int q = 1; q < 4; ++q) {  // 1: the x neighbour, 2: the y neighbour, 3: the diagonal tile
                const bool uy = (q & 2) != 0, ux = (q & 1) != 0;
                if ((uy && oth_y == 0) || (ux && oth_x == 0)) continue;
                const T c = tile_value<T, MODE>(s, plane, uy ? tr1 : tr, ux ? tc1 : tc, uy ? y1 : y, ux ? x1 : xx, m1[b],
                                                m2[b], kk[b], fast_ok[b]);
                if (q == 1) c01 = c;
                else if (q == 2) c10 = c;
                else c11 = c;
              }
              const T mixed = mix_tiles<T>(c00, c01, c10, c11, oth_x != 0, oth_y != 0, nx, ny, v);
#pragma unroll
              for (int jj = 0; jj < N; ++jj) o[jj] = jj == j ? mixed : o[jj];
            }
          }
          if (d_minmax) {
#pragma unroll
            for (int j = 0; j < N; ++j) {
              if (j >= cnt) break;
              if (IsIntegral<T>::value) {
                imin[b] = min(imin[b], (uint32_t)o[j]);
                imax[b] = max(imax[b], (uint32_t)o[j]);
              } else {
                const double ov = (double)o[j];
                vmin[b] = mg_nanmin(vmin[b], ov);
                vmax[b] = mg_nanmax(vmax[b], ov);
              }
            }
          }
          T* dst = image + ((int64_t)plane * h_out + oy) * w_out + ox0;
          if (cnt == N) {
            store_vec<T, N>(dst, o);
          } else {
            for (int j = 0; j < cnt; ++j) dst[j] = o[j];
          }
        }
      }
    }
  }
  if (d_minmax) mg_block_minmax<PB>(vmin, vmax, imin, imax, np, d_minmax, plane0);
}

template <typename T, int MODE>
int launch_blend(const BlendSrc<T>& src, int64_t n_planes, int overlap, void* d_image, double* d_minmax, hipStream_t s) {
  const auto [clip, hy, hx, h_out, w_out] = mg_stitch_geom(src.ty, src.tx, overlap, src.n_tr, src.n_tc);
  (void)clip;
  if (n_planes == 0 || h_out == 0 || w_out == 0) return MG_OK;
  if (n_planes > 0x7FFFFFF0) return MG_EINVAL;
  int rows;
  const dim3 grid = stitch_grid<VecOf<T>::N>(h_out, w_out, n_planes, rows);
  if (grid.y > 65535 || grid.z > 65535) return MG_EINVAL;
  hipLaunchKernelGGL((k_blend_stitch<T, MODE>), grid, dim3(256), 0, s, src, (int)n_planes, overlap, hy, hx, (T*)d_image,
                     d_minmax, rows);
  MG_CHECK_LAUNCH();
  return MG_OK;
}

inline bool field_dtype_ok(const void* p, int dt) { return p == nullptr || dt == MG_F32 || dt == MG_F64; }
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
  if (!d_tiles || !d_image || n_planes < 0 || !blend_shape_ok(n_tile_rows, n_tile_cols, ty, tx, overlap)) return MG_EINVAL;
  // (integer pixels, dark 0, flat 1: the plain pass writes the pixel itself, see mg_flatfield_apply_stitch)
  if (apply_flatfield && mg_flatfield_is_identity(dtype, dark, d_dark, flat, d_flat)) apply_flatfield = 0;
  if (apply_flatfield && (!d_max2 || planes_per_group <= 0)) return MG_EINVAL;
  if (!field_dtype_ok(d_dark, dark_dtype) || !field_dtype_ok(d_flat, flat_dtype)) return MG_EINVAL;
  hipStream_t s = mg_stream(stream);
  return mg_dispatch_pixel(dtype, [&](auto t) {
    using T = decltype(t);
    const BlendSrc<T> src{(const T*)d_tiles, n_tile_rows, n_tile_cols, ty, tx, planes_per_group > 0 ? planes_per_group : 1,
                          dark, d_dark, dark_dtype, flat, d_flat, flat_dtype, d_max2};
    return apply_flatfield ? launch_blend<T, BL_FLAT>(src, n_planes, overlap, d_image, d_minmax, s)
                           : launch_blend<T, BL_COPY>(src, n_planes, overlap, d_image, d_minmax, s);
  });
}

extern "C" int mg_shading_apply_stitch_blend(const void* d_tiles, int dtype, int n_fields, int64_t planes_per_field,
                                             int n_tile_rows, int n_tile_cols, int ty, int tx, int overlap,
                                             const float* d_flat, const float* d_dark, void* d_image, double* d_minmax,
                                             void* stream) {
  if (!d_tiles || !d_image || !d_flat || !d_dark || n_fields < 1 || planes_per_field < 0 || planes_per_field > 0x7FFFFFF0 ||
      !blend_shape_ok(n_tile_rows, n_tile_cols, ty, tx, overlap))
    return MG_EINVAL;
  if (planes_per_field == 0) return MG_OK;
  hipStream_t s = mg_stream(stream);
  return mg_dispatch_pixel(dtype, [&](auto t) {
    using T = decltype(t);
    const BlendSrc<T> src{(const T*)d_tiles, n_tile_rows, n_tile_cols, ty, tx, (int)planes_per_field,
                          0.0, d_dark, MG_F32, 1.0, d_flat, MG_F32, nullptr};
    return launch_blend<T, BL_SHADE>(src, (int64_t)n_fields * planes_per_field, overlap, d_image, d_minmax, s);
  });
}
