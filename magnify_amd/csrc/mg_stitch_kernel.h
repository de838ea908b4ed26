// The generic stitch kernel: crop / concat of the tiles with the pending correction (MODE), optionally the seams
// blended (BLEND, DESIGN.md "stitch: linear overlap blending") and a selection of planes (SUBSET), and the per-plane
// min / max of what was written.  mg_flatfield.hip instantiates the plain forms, mg_blend.hip the blended ones; each
// translation unit only what it launches.
#pragma once
#include "mg_blendop.h"
#include "mg_common.h"
#include "mg_flatcorr.h"
#include "mg_shadeop.h"
#include "mg_stitch.h"

namespace {

// Block = 256 lanes x N pixels of `rows_per_block` output rows, for PLANES_PER_BLOCK consecutive planes: the dark/flat
// operands of a pixel chunk are loaded once and reused across those planes.  BLEND: the chunk of a lane is first made
// as in the plain pass, then its band pixels are mixed.
template <typename T, int MODE, bool BLEND, bool SUBSET>
__global__ __launch_bounds__(256) void k_stitch(StitchSrc<T> s, int n_planes, int v, int hy, int hx,
                                                 T* __restrict__ image, double* __restrict__ d_minmax,
                                                 int rows_per_block, PlaneSel sel) {
  constexpr int N = VecOf<T>::N;
  constexpr int PB = PLANES_PER_BLOCK;
  const int clip = v / 2, rem = v % 2, n_tr = s.n_tr, n_tc = s.n_tc, tx = s.tx;
  const Axis ay{v, clip, rem, hy, n_tr}, ax{v, clip, rem, hx, n_tc};
  const int plane0 = blockIdx.z * PB;  // (SUBSET: n_planes, plane0 count SELECTED planes; pl[b] is the plane itself)
  const int np = min(PB, n_planes - plane0);
  const int h_out = n_tr * hy, w_out = n_tc * hx;
  const int ox0 = (blockIdx.x * blockDim.x + threadIdx.x) * N;
  int pl[PB];
#pragma unroll
  for (int b = 0; b < PB; ++b) pl[b] = (!SUBSET || b < np) ? sel_plane<SUBSET>(plane0 + b, s.planes_per_group, sel) : 0;
  GroupMax gm[PB];
#pragma unroll
  for (int b = 0; b < PB; ++b)
    if (MODE == BL_FLAT && b < np) gm[b] = group_maxima(s.d_max2, pl[b], s.planes_per_group);
  PlaneMinMax<T, PB> mm;
  const int64_t tile_elems = (int64_t)s.ty * tx;
  if (ox0 < w_out) {
    const StitchChunk c = stitch_chunk<N>(ox0, hx, clip, w_out);
    const int cnt = c.cnt;
    bool col_band = false;  // a pixel of this chunk lies in a column band
    if constexpr (BLEND) {
#pragma unroll
      for (int j = 0; j < N; ++j) {
        const int ox = ox0 + min(j, cnt - 1), tc = ox / hx;
        int other, num;
        axis_term(ax, tc, ox - tc * hx, other, num);
        col_band |= other != 0;
      }
    }
    // a workgroup takes the row groups blockIdx.y, blockIdx.y + gridDim.y, ...: one set of min/max atomics per
    // workgroup however short the row groups are
    for (int yg = blockIdx.y; yg * rows_per_block < h_out; yg += gridDim.y) {
      const int row_end = min((yg + 1) * rows_per_block, h_out);
      for (int oy = yg * rows_per_block; oy < row_end; ++oy) {
        const int tr = oy / hy;
        const int y = oy - tr * hy + clip;
        int oth_y = 0, ny = 2 * v;  // (the same in every lane: a row band is a whole row)
        if constexpr (BLEND) axis_term(ay, tr, y - clip, oth_y, ny);
        int64_t pix[N], toff[N];  // pixel index inside the tile, element offset of the tile in a plane
        chunk_row<N>(c, hx, clip, n_tc, tx, tile_elems, tr, y, pix, toff);
        double dk[N], fl[N], rr[N];
        // the operands of the chunk, shared by the planes that use the same fields (BL_FLAT: all of them)
        auto load_operands = [&](const void* dptr, const void* fptr) {
          load_chunk_field<N>(dptr, s.dark_dt, s.dark, c.one_tile, pix, dk);
          load_chunk_field<N>(fptr, s.flat_dt, s.flat, c.one_tile, pix, fl);
          // the refined reciprocal of flat is shared by all planes of the block
#pragma unroll
          for (int j = 0; j < N; ++j) rr[j] = (MODE == BL_FLAT && IsIntegral<T>::value) ? refined_rcp(fl[j]) : 0.0;
        };
        if (MODE == BL_FLAT) load_operands(s.d_dark, s.d_flat);
        int field_loaded = -1;
#pragma unroll
        for (int b = 0; b < PB; ++b) {
          if (b >= np) break;
          const int plane = pl[b];
          if (MODE == BL_SHADE) {
            const int field = plane / s.planes_per_group;
            if (field != field_loaded) {  // (uniform)
              field_loaded = field;
              load_operands((const float*)s.d_dark + (int64_t)field * tile_elems,
                            (const float*)s.d_flat + (int64_t)field * tile_elems);
            }
          }
          T x[N], o[N];
          load_chunk<T, N>(s.tiles + (int64_t)plane * n_tr * n_tc * tile_elems, c.one_tile, pix, toff, x);
#pragma unroll
          for (int j = 0; j < N; ++j) {
            if (MODE == BL_FLAT) {
              double t = (double)x[j] - dk[j];
              t = t < 0.0 ? 0.0 : t;
              o[j] = correct_pixel<T>(t, fl[j], rr[j], gm[b].m1, gm[b].m2, gm[b].kk, gm[b].fast_ok);
            } else if (MODE == BL_SHADE) {
              o[j] = ShadeOp<T>::apply(x[j], (float)dk[j], (float)fl[j]);
            } else {
              o[j] = x[j];
            }
          }
          if constexpr (BLEND) {
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
                  const T cq = tile_value<T, MODE>(s, plane, uy ? tr1 : tr, ux ? tc1 : tc, uy ? y1 : y, ux ? x1 : xx, gm[b]);
                  if (q == 1) c01 = cq;
                  else if (q == 2) c10 = cq;
                  else c11 = cq;
                }
                const T mixed = mix_tiles<T>(c00, c01, c10, c11, oth_x != 0, oth_y != 0, nx, ny, v);
#pragma unroll
                for (int jj = 0; jj < N; ++jj) o[jj] = jj == j ? mixed : o[jj];
              }
            }
          }
          if (d_minmax) mm.add(b, o, cnt);
          store_chunk<T, N>(image + ((int64_t)plane * h_out + oy) * w_out + ox0, o, cnt);
        }
      }
    }
  }
  if (d_minmax) {
    if constexpr (SUBSET) mm.flush(np, d_minmax, SelBase{plane0, s.planes_per_group, sel});
    else mm.flush(np, d_minmax, plane0);
  }
}

// The pass for a source, `n_planes` planes (SUBSET: selected planes) and an overlap: geometry, grid, launch.
template <int MODE, bool BLEND, bool SUBSET, typename T>
int launch_stitch(const StitchSrc<T>& src, int64_t n_planes, int overlap, PlaneSel sel, void* d_image, double* d_minmax,
                  hipStream_t s) {
  const auto [clip, hy, hx, h_out, w_out] = mg_stitch_geom(src.ty, src.tx, overlap, src.n_tr, src.n_tc);
  (void)clip;
  if (n_planes == 0 || h_out == 0 || w_out == 0) return MG_OK;
  if (n_planes > 0x7FFFFFF0) return MG_EINVAL;
  int rows;
  const dim3 grid = stitch_grid<VecOf<T>::N>(h_out, w_out, n_planes, rows);
  if (grid.y > MG_WALK_MAX_Y || grid.z > MG_WALK_MAX_Y) return MG_EINVAL;
  hipLaunchKernelGGL((k_stitch<T, MODE, BLEND, SUBSET>), grid, dim3(256), 0, s, src, (int)n_planes, overlap, hy, hx,
                     (T*)d_image, d_minmax, rows, sel);
  MG_CHECK_LAUNCH();
  return MG_OK;
}

}  // namespace
