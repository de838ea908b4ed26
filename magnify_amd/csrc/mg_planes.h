// What the plane filters share (mg_depth.hip, mg_despeckle.hip, mg_background.hip; DESIGN.md, "Plane filters: what they
// share"): the host check of a block of planes, the grid "workgroups walk the items of a plane, blockIdx.y walks the
// planes" with the device loops that go with it, and the fill of a tile with its halo into LDS.
#pragma once
#include <algorithm>
#include <initializer_list>

#include "mg_common.h"

// ---- the host check ---------------------------------------------------------------------------------------------------

// A contiguous block (n, h, w) of `dtype` (for a depth stack n counts the stacks; z is the entry's own rule) and the
// pointers into blocks of that type.  MG_PLANES_REFUSED: a dtype other than u8 / u16 / f32 / f64; n, h or w below 0;
// h above 2^30 or w above 2^20 (a tile's fill reads with 32-bit byte offsets from the tile's first pixel, and n h w
// keeps well inside 63 bits); a pointer of `pixels` that is not null and not aligned to the element size -- null is
// the entry's own rule, as are all its other arguments.  MG_PLANES_EMPTY: none of that, and n, h or w is 0.  An
// entry returns MG_EINVAL for REFUSED or a broken rule of its own, THEN MG_OK for EMPTY, nothing launched either way.
enum MgPlanes { MG_PLANES_REFUSED, MG_PLANES_EMPTY, MG_PLANES_RUN };
static inline MgPlanes mg_planes_check(int dtype, int64_t n, int h, int w, std::initializer_list<const void*> pixels) {
  if (dtype != MG_U8 && dtype != MG_U16 && dtype != MG_F32 && dtype != MG_F64) return MG_PLANES_REFUSED;
  if (n < 0 || h < 0 || w < 0 || h > (1 << 30) || w > (1 << 20)) return MG_PLANES_REFUSED;
  for (const void* p : pixels)
    if (reinterpret_cast<uintptr_t>(p) % mg_elem_size(dtype)) return MG_PLANES_REFUSED;
  return n == 0 || h == 0 || w == 0 ? MG_PLANES_EMPTY : MG_PLANES_RUN;
}

// ---- the grid and its walk --------------------------------------------------------------------------------------------

// Grid of a kernel whose workgroups walk the `items` (tiles, or blocks of lanes; at least 1) of a plane along x and the
// n planes along y: y = min(n, MG_WALK_MAX_Y); x = the items, cut to `per_plane` and to x * y <= `budget` workgroups in all (0:
// no such limit), and never below 1.  Neither count is bounded by the grid: the kernel strides over both, with
// MG_FOR_BLOCK_PLANES and MG_FOR_BLOCK_ITEMS (or a loop of its own over items that are not dealt by the workgroup).
static inline dim3 mg_plane_grid(int64_t items, int64_t n, int64_t budget = 0, int64_t per_plane = 0) {
  const int64_t gy = std::min<int64_t>(n, MG_WALK_MAX_Y);
  int64_t gx = items;
  if (per_plane) gx = std::min(gx, per_plane);
  if (budget) gx = std::min(gx, budget / gy);
  return dim3((unsigned)std::max<int64_t>(gx, 1), (unsigned)gy);
}
// The loop heads: the planes of this workgroup's blockIdx.y, and the items (below 2^31) of a plane of its blockIdx.x.
#define MG_FOR_BLOCK_PLANES(plane, n) for (int64_t plane = blockIdx.y; plane < (n); plane += gridDim.y)
#define MG_FOR_BLOCK_ITEMS(item, items) for (int item = blockIdx.x; item < (items); item += gridDim.x)
// Item `tile` as a tile of a plane that is tiles_x tiles wide, row-major.
struct MgTile {
  int y, x;  // the tile's row and column
};
__device__ __forceinline__ MgTile mg_tile(int tile, int tiles_x) {
  const int tyi = tile / tiles_x;
  return {tyi, tile - tyi * tiles_x};
}

// ---- the tile fill ----------------------------------------------------------------------------------------------------

// The side of a padded tile that is known when the kernel is compiled (one that is not: a struct with `n` and `row`).
template <int N>
struct MgSide {
  static constexpr int n = N;
  __device__ __forceinline__ int row(int i) const { return i / N; }  // of element i, row-major
};

// side.n x side.n pixels of `plane` (h x w) into s_px, row-major: the tile whose first output pixel is (y0, x0) with
// `halo` more pixels on every side, coordinates clamped into the plane -- the reader of the tile has no edge cases
// and never sees another plane.  Workgroups of 256 threads, all of which call.  A thread issues NLOAD loads before its
// first store, so a wave has NLOAD cache lines in flight (one load at a time leaves the kernel waiting on memory
// latency); a tile of more than 256 NLOAD pixels takes several such rounds.  The loads are relative to the tile's
// first pixel, with 32-bit byte offsets: at most (side.n - 1) (w + 1) pixels, side.n <= 68 and w <= 2^20
// (mg_planes_check).  `wait` (uniform): somebody may still be reading s_px -- the barrier for that stands behind the
// first round's loads, where it costs no latency.  Returns behind the barrier after the last store.
template <int NLOAD, class T, class Side>
__device__ __forceinline__ void mg_fill_tile(T* s_px, const T* plane, int h, int w, int y0, int x0,
                                             int halo, Side side, bool wait) {
  const int t = threadIdx.x, total = side.n * side.n;
  const int gy0 = max(y0 - halo, 0), gx0 = max(x0 - halo, 0);
  const char* first = reinterpret_cast<const char*>(plane + (int64_t)gy0 * w + gx0);
  for (int base = 0; base < total; base += 256 * NLOAD) {
    T staged[NLOAD];
#pragma unroll
    for (int j = 0; j < NLOAD; ++j) {  // (past the tile: its last pixel again)
      const int i = min(base + t + 256 * j, total - 1), yy = side.row(i), xx = i - yy * side.n;
      const int gy = min(max(y0 - halo + yy, 0), h - 1), gx = min(max(x0 - halo + xx, 0), w - 1);
      const uint32_t off = ((uint32_t)(gy - gy0) * (uint32_t)w + (uint32_t)(gx - gx0)) * (uint32_t)sizeof(T);
      staged[j] = *reinterpret_cast<const T*>(first + off);
    }
    if (wait && base == 0) __syncthreads();
#pragma unroll
    for (int j = 0; j < NLOAD; ++j)
      if (base + t + 256 * j < total) s_px[base + t + 256 * j] = staged[j];
  }
  __syncthreads();
}
