// Skew: the projection profiles of a plane along every angle of a table (include/magnify_hip.h, "Skew"; DESIGN.md §34;
// tests/skew_ref.py).  Integers only behind the quantisation of a float pixel: every sum is exact in any order.
//
// Grid and walk: mg_plane_grid over the MG_SKEW_TILE x MG_SKEW_TILE tiles of the one plane.  A workgroup of 256 threads
// quantises a tile into LDS -- a pixel that takes part as q | 1 << SK_CNT_SHIFT, its sum and its count in one word, any
// other as 0 -- and drops the tile when nothing of it takes part.  Thread t then owns two RUNS of SK_RUN consecutive
// pixels, in registers for the whole angle table: a piece of row t % 64 for the row profile and a piece of column
// t % 64 for the column profile.  Along a row the row bin moves by sin(angle) per pixel and along a column the column
// bin does, so a run stays in one bin for 1 / sin pixels: the thread adds the words up in a register and goes to LDS
// when the bin changes -- about 1 + 16 sin times per run, not 16.  (Across the run the other profile's bin moves by cos
// per pixel: that is why each profile has runs of its own direction.)  The column profile is the row profile of the
// transposed plane at the opposite angle, so both are one walk.  A wave holds the same piece of 64 neighbouring lines:
// 2 C is 65536 less a little, so their bins change at nearly the same steps -- the branch around the LDS atomic is
// skipped by the whole wave at most steps -- and they change into 64 different bins.
// Inside a tile the index is 32-bit: (v C - u S) = the tile's corner value (int64, once per angle) + a difference below
// 2^23, and bin = ((corner & 0xFFFF) + difference) >> 16 + (corner >> 16).
// LDS histograms: SK_GROUP angles at a time, SK_BINS bins per angle and axis from the tile's lowest bin on (a tile
// spans at most 63 * (|C| + |S|) / 32768 + 2 <= 92 bins), one 64-bit word per bin: the count above the 32-bit sum
// (64 * 64 * 65535 < 2^32).  Non-empty bins go to the profiles as one 64-bit and one 32-bit integer atomic each.
#include "mg_planes.h"

namespace {

constexpr int SK_T = MG_SKEW_TILE, SK_RUN = 16, SK_SEGS = SK_T / SK_RUN, SK_PITCH = SK_T + 1;
constexpr int SK_GROUP = 8, SK_BINS = 96;
constexpr int SK_CNT_SHIFT = 24;  // a run's word: the count above SK_CNT_SHIFT bits of sum
constexpr uint32_t SK_SUM_MASK = (1u << SK_CNT_SHIFT) - 1u;
static_assert(SK_T == 64 && SK_T * SK_SEGS == 256 && SK_T * SK_T == 256 * SK_RUN, "a thread owns one run of each direction");
static_assert(SK_RUN * 65535u <= SK_SUM_MASK && SK_RUN < (1 << (32 - SK_CNT_SHIFT)), "a run's sum and count fit their fields");
static_assert((uint64_t)SK_T * SK_T * 65535u < (1ull << 32), "a tile's partial sum fits 32 bits");
static_assert((SK_T - 1) * 46341ll / 32768 + 3 <= SK_BINS, "a tile's bins fit the histogram (|C| + |S| <= 46341)");
static_assert(2 * (SK_T - 1) * 46341ll + 65535 < (1ll << 31), "the index inside a tile is 32-bit");
static_assert(2 * SK_GROUP <= 256 && 2 * MG_SKEW_MAX_ANGLES <= 256, "one thread per table entry");

template <class T>
struct SkewArgs {
  const T* plane;
  int h, w;
  int64_t row_stride;
  double lo, scale;
  const int32_t* cs;
  int n_angles, nb, tiles_x, tiles;
  unsigned long long* sums;
  uint32_t* counts;
};

// A pixel's word: q | 1 << SK_CNT_SHIFT, or 0 for a NaN
template <class T>
__device__ __forceinline__ uint32_t sk_word(T p, double lo, double scale) {
  if constexpr (std::is_integral<T>::value) {
    return (uint32_t)p | (1u << SK_CNT_SHIFT);
  } else {
    if (p != p) return 0u;
    const double t = ((double)p - lo) * scale;
    return (t < 0.0 ? 0u : t > 65535.0 ? 65535u : t == t ? (uint32_t)floor(t) : 0u) | (1u << SK_CNT_SHIFT);
  }
}

// Of one angle and axis, for the tile whose first pixel is (v0, u0): v C - u S over the tile = corner + a difference.
struct SkewAxis {
  int frac;    // corner & 0xFFFF
  int shift;   // (corner >> 16) - lowest: what turns (frac + difference) >> 16 into an index of the tile's histogram
  int lowest;  // the lowest (v C - u S) >> 16 of the tile: that of one of its corners
};
__device__ __forceinline__ SkewAxis sk_axis(int v0, int u0, int c, int s) {
  const int64_t dv = 2 * (SK_T - 1) * (int64_t)c, du = -2 * (SK_T - 1) * (int64_t)s;
  const int64_t corner = (int64_t)v0 * c - (int64_t)u0 * s;
  const int lowest = (int)((corner + min(dv, (int64_t)0) + min(du, (int64_t)0)) >> 16);
  return {(int)(corner & 0xFFFF), (int)(corner >> 16) - lowest, lowest};
}

__device__ __forceinline__ void sk_add(unsigned long long* s_hist, int bin, uint32_t word) {
  if ((unsigned)bin < (unsigned)SK_BINS)  // (always, with a table of 32768 (cos, sin))
    atomicAdd(&s_hist[bin], ((unsigned long long)(word >> SK_CNT_SHIFT) << 32) | (word & SK_SUM_MASK));
}

// One run: pixel i has x + i step in the place of frac + difference.
__device__ __forceinline__ void sk_walk(const uint32_t (&run)[SK_RUN], int x, int step, int shift,
                                        unsigned long long* s_hist) {
  int cur = x >> 16;
  uint32_t word = 0;
#pragma unroll
  for (int i = 0; i < SK_RUN; ++i, x += step) {
    const int bin = x >> 16;
    if (bin != cur) {
      sk_add(s_hist, cur + shift, word);
      word = 0;
      cur = bin;
    }
    word += run[i];
  }
  if (word) sk_add(s_hist, cur + shift, word);
}

template <class T>
__global__ __launch_bounds__(256) void k_skew_profiles(const SkewArgs<T> a) {
  __shared__ uint32_t s_tile[SK_T * SK_PITCH];
  __shared__ unsigned long long s_hist[SK_GROUP * 2 * SK_BINS];
  __shared__ SkewAxis s_axis[SK_GROUP * 2];
  __shared__ int s_cs[2 * MG_SKEW_MAX_ANGLES];
  const int t = threadIdx.x, line = t % SK_T, seg = t / SK_T;
  const int64_t radius = (int64_t)min(a.h, a.w) - 1, r2 = radius * radius;
  if (t < 2 * a.n_angles) s_cs[t] = a.cs[t];  // (read behind the barriers of the first tile that takes part)

  MG_FOR_BLOCK_ITEMS(item, a.tiles) {
    const MgTile tile = mg_tile(item, a.tiles_x);
    const int y0 = tile.y * SK_T, x0 = tile.x * SK_T;
    int any = 0;
#pragma unroll 4
    for (int j = 0; j < SK_RUN; ++j) {
      const int i = t + 256 * j, r = i / SK_T, c = i % SK_T, y = y0 + r, x = x0 + c;
      uint32_t word = 0u;
      if (y < a.h && x < a.w) {
        const int64_t dy = 2 * y - (a.h - 1), dx = 2 * x - (a.w - 1);
        if (dy * dy + dx * dx <= r2) word = sk_word(a.plane[(int64_t)y * a.row_stride + x], a.lo, a.scale);
      }
      s_tile[r * SK_PITCH + c] = word;
      any |= word != 0u;
    }
    if (!__syncthreads_or(any)) continue;  // (uniform; nobody reads this tile, so the next fill needs no barrier)

    uint32_t row_run[SK_RUN], col_run[SK_RUN];
#pragma unroll
    for (int i = 0; i < SK_RUN; ++i) {
      row_run[i] = s_tile[line * SK_PITCH + seg * SK_RUN + i];
      col_run[i] = s_tile[(seg * SK_RUN + i) * SK_PITCH + line];
    }
    const int dy0 = 2 * y0 - (a.h - 1), dx0 = 2 * x0 - (a.w - 1);  // the tile's first pixel

    for (int g0 = 0; g0 < a.n_angles; g0 += SK_GROUP) {
      const int ng = min(SK_GROUP, a.n_angles - g0);
      for (int e = t; e < ng * 2 * SK_BINS; e += 256) s_hist[e] = 0ull;
      if (t < 2 * ng) {  // the row profile: v = dy, u = dx; the column profile: v = dx, u = dy, S negated
        const int c = s_cs[2 * (g0 + t / 2)], s = s_cs[2 * (g0 + t / 2) + 1];
        s_axis[t] = (t & 1) ? sk_axis(dx0, dy0, c, -s) : sk_axis(dy0, dx0, c, s);
      }
      __syncthreads();
      for (int g = 0; g < ng; ++g) {
        const int c = s_cs[2 * (g0 + g)], s = s_cs[2 * (g0 + g) + 1];
        const int along = 2 * line * c, across = 2 * seg * SK_RUN * s;  // the run's first pixel from the tile's
        const SkewAxis rows = s_axis[2 * g], cols = s_axis[2 * g + 1];
        sk_walk(row_run, rows.frac + along - across, -2 * s, rows.shift, s_hist + 2 * g * SK_BINS);
        sk_walk(col_run, cols.frac + along + across, 2 * s, cols.shift, s_hist + (2 * g + 1) * SK_BINS);
      }
      __syncthreads();
      for (int e = t; e < ng * 2 * SK_BINS; e += 256) {
        const unsigned long long v = s_hist[e];
        const uint32_t cnt = (uint32_t)(v >> 32);
        if (!cnt) continue;
        const int ga = e / SK_BINS, k = s_axis[ga].lowest + (e - ga * SK_BINS) + a.nb / 2;  // ga: 2 * angle of the group + axis
        if ((unsigned)k >= (unsigned)a.nb) continue;  // (never, with a table of 32768 (cos, sin))
        const int64_t at = ((int64_t)g0 * 2 + ga) * a.nb + k;
        atomicAdd(&a.sums[at], v & 0xFFFFFFFFull);
        atomicAdd(&a.counts[at], cnt);
      }
      __syncthreads();  // (the next group clears the histograms, the next tile overwrites s_tile)
    }
  }
}

}  // namespace

extern "C" int mg_skew_profiles(const void* d_plane, int dtype, int h, int w, int64_t row_stride, double lo, double scale,
                                const int32_t* d_cs, int n_angles, uint64_t* d_sums, uint32_t* d_counts, void* stream) {
  if (mg_planes_check(dtype, 1, h, w, {d_plane}) == MG_PLANES_REFUSED || !d_plane || !d_cs || !d_sums || !d_counts)
    return MG_EINVAL;
  if (reinterpret_cast<uintptr_t>(d_cs) % 4 || reinterpret_cast<uintptr_t>(d_sums) % 8 ||
      reinterpret_cast<uintptr_t>(d_counts) % 4)
    return MG_EINVAL;
  if (h < 8 || w < 8 || h > MG_SKEW_MAX_SIDE || w > MG_SKEW_MAX_SIDE || row_stride < w) return MG_EINVAL;
  if (n_angles < 1 || n_angles > MG_SKEW_MAX_ANGLES || !isfinite(lo) || !isfinite(scale)) return MG_EINVAL;
  const int tiles_x = (w + SK_T - 1) / SK_T, tiles = tiles_x * ((h + SK_T - 1) / SK_T);  // (at most 512 * 512)
  hipStream_t s = mg_stream(stream);
  return mg_dispatch_pixel(dtype, [&](auto t) {
    using T = decltype(t);
    const SkewArgs<T> args{(const T*)d_plane, h, w, row_stride, lo, scale, d_cs, n_angles, std::min(h, w) + 2, tiles_x, tiles,
                           reinterpret_cast<unsigned long long*>(d_sums), d_counts};
    // about eight workgroups per CU in all; each walks its share of the tiles
    hipLaunchKernelGGL(k_skew_profiles<T>, mg_plane_grid(tiles, 1, MG_SKEW_WALK), dim3(256), 0, s, args);
    MG_CHECK_LAUNCH();
    return (int)MG_OK;
  });
}
