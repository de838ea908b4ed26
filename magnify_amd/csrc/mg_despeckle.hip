// Hot pixels (the `remove_outliers` component): every pixel of a contiguous block (N, H, W) is compared with the median
// of its (2k + 1)^2 window (edge-replicated) and replaced by it where it stands out -- or where a defect map says so
// (mg_despeckle_planes); the same test counted over the planes of one sensor gives the votes a defect map is made from
// (mg_outlier_votes).  Oracle: tests/despeckle_ref.py.
#include "mg_common.h"
#include "mg_mediannet.h"
#include "mg_planes.h"
#include "mg_select.h"

namespace {

constexpr int DS = MG_DESPECKLE_TILE, DS_ROWS = DS * DS / 256;  // a thread's outputs: column t % DS, DS_ROWS rows
static_assert(DS == 64 && DS_ROWS == 16, "a wave owns one row of the tile at a time: 64 lanes along x");

// The sort key of a pixel: median_key's, with every NaN moved behind +inf (numpy.sort's order), whatever its sign.
template <class T>
__device__ __forceinline__ typename median_key<T>::type despeckle_key(T v) {
  typename median_key<T>::type key;
  if (!median_key<T>::key(v, &key)) key = ~(typename median_key<T>::type)0;
  return key;
}

// The keys of a thread's window as it walks down a column: push() takes in the next window row (WIN pixels in LDS) and
// forgets the top one, median() is the middle key of the WIN x WIN held.  3 x 3: every row is kept sorted, so a pixel
// costs one sort of three and four 3-input picks; 5 x 5: the keys as they are, forgetful selection.
template <class T, int WIN>
struct DespeckleWindow {
  using Key = typename median_key<T>::type;
  Key keys[WIN * WIN] = {};  // rows top to bottom
  __device__ __forceinline__ void push(const T* row) {
#pragma unroll
    for (int i = 0; i < (WIN - 1) * WIN; ++i) keys[i] = keys[i + WIN];
#pragma unroll
    for (int i = 0; i < WIN; ++i) keys[(WIN - 1) * WIN + i] = despeckle_key<T>(row[i]);
  }
  __device__ __forceinline__ Key median() const { return mg_net_median<Key, WIN * WIN>(keys); }
};
template <class T>
struct DespeckleWindow<T, 3> {
  using Key = typename median_key<T>::type;
  Key lo[3] = {}, mid[3] = {}, hi[3] = {};
  __device__ __forceinline__ void push(const T* row) {
#pragma unroll
    for (int j = 0; j < 2; ++j) lo[j] = lo[j + 1], mid[j] = mid[j + 1], hi[j] = hi[j + 1];
    lo[2] = despeckle_key<T>(row[0]), mid[2] = despeckle_key<T>(row[1]), hi[2] = despeckle_key<T>(row[2]);
    mg_net_sort3(lo[2], mid[2], hi[2]);
  }
  __device__ __forceinline__ Key median() const { return mg_net_median9_rows(lo, mid, hi); }
};

// "Window median + condition", shared by both kernels: the window's median as a pixel (one of the window's values; the
// all-ones key of a NaN comes back as a NaN) and whether the pixel is to be replaced by it.
template <class T, int WIN>
__device__ __forceinline__ bool despeckle_test(const DespeckleWindow<T, WIN>& window, T px, int which, double threshold,
                                               const uint8_t* defect, T* med) {
  *med = (T)median_key<T>::value(window.median());
  if (defect) return *defect != 0;
  const double d = (double)px - (double)*med;  // NaN fails every comparison below: the pixel stays
  return which == MG_OUTLIER_ALL || (which != MG_OUTLIER_DARK && d > threshold) ||
         (which != MG_OUTLIER_BRIGHT && -d > threshold);
}

// Grid and walk: mg_plane_grid.  LDS: the tile with its halo of K, PH x PH pixels of T, filled by mg_fill_tile with all
// of a thread's loads in flight at once.  Thread t owns column t % DS and rows DS_ROWS * (t / DS) ..: it walks down with
// the window's keys in registers, one new window row per pixel.  VOTES: nothing is written but an int32 atomic per
// pixel that passes; otherwise d_dst gets every pixel and d_counts (if any) one 64-bit atomic per workgroup and plane,
// after the workgroup's last tile of the plane: the counter of a plane is one address, and an atomic per tile on it
// took longer than all the rest of the kernel.
template <class T, int K, bool VOTES>
__global__ __launch_bounds__(256) void k_despeckle(const T* __restrict__ src, T* __restrict__ dst, int64_t n, int h, int w,
                                                   int tiles_x, int n_tiles, int which, double threshold,
                                                   const uint8_t* __restrict__ defects, unsigned long long* __restrict__ counts,
                                                   int32_t* __restrict__ votes) {
  constexpr int WIN = 2 * K + 1, PH = DS + 2 * K, NLOAD = (PH * PH + 255) / 256;
  __shared__ T s_px[PH * PH];
  const int t = threadIdx.x, ox = t % DS, oy0 = DS_ROWS * (t / DS);
  const int64_t plane = (int64_t)h * w;
  bool fresh = true;  // (uniform) nobody has read the tile in LDS yet
  MG_FOR_BLOCK_PLANES(pi, n) {
    int replaced = 0;
    MG_FOR_BLOCK_ITEMS(tile, n_tiles) {
      const MgTile at = mg_tile(tile, tiles_x);
      const int y0 = at.y * DS, x0 = at.x * DS;
      const int x = x0 + ox, rows = min(DS_ROWS, h - (y0 + oy0));  // (rows <= 0: the thread has no pixel)
      mg_fill_tile<NLOAD>(s_px, src + pi * plane, h, w, y0, x0, K, MgSide<PH>{}, !fresh);
      fresh = false;
      if (x < w) {
        DespeckleWindow<T, WIN> window;
        const T* col = s_px + oy0 * PH + ox;
#pragma unroll
        for (int j = 0; j < WIN - 1; ++j) window.push(col + j * PH);
#pragma unroll 4
        for (int r = 0; r < rows; ++r) {
          const T* c = col + r * PH;
          window.push(c + (WIN - 1) * PH);
          const T px = c[K * PH + K];
          const int64_t o = (int64_t)(y0 + oy0 + r) * w + x;
          T med;
          const bool hit = despeckle_test<T, WIN>(window, px, which, threshold, defects ? defects + o : nullptr, &med);
          if constexpr (VOTES) {
            if (hit) atomicAdd(votes + o, 1);
          } else {
            dst[pi * plane + o] = hit ? med : px;
            replaced += hit;
          }
        }
      }
    }
    if constexpr (!VOTES) {
      if (counts) {  // (uniform: every thread takes part in the fold)
        const int total = mg_block_fold(replaced, [](int a, int b) { return a + b; });
        if (t == 0 && total) atomicAdd(counts + pi, (unsigned long long)total);
      }
    }
  }
}

template <class T, int K, bool VOTES>
int launch_despeckle(const void* d_src, void* d_dst, int64_t n, int h, int w, int which, double threshold,
                     const uint8_t* d_defects, int64_t* d_counts, int32_t* d_votes, hipStream_t s) {
  const int64_t tiles_x = ((int64_t)w + DS - 1) / DS, tiles_y = ((int64_t)h + DS - 1) / DS;
  if (tiles_x * tiles_y > 0x7FFFFFFF) return MG_EINVAL;
  if (VOTES) {
    if (mg_zero_async(d_votes, (size_t)h * (size_t)w * 4, s) != hipSuccess) return MG_ELAUNCH;
  } else if (d_counts) {
    if (mg_zero_async(d_counts, (size_t)n * 8, s) != hipSuccess) return MG_ELAUNCH;
  }
  static_assert(sizeof(double) * (DS + 2 * MG_DESPECKLE_MAX_K) * (DS + 2 * MG_DESPECKLE_MAX_K) <= 40 * 1024,
                "the largest tile (float64, k = 2) leaves room for four workgroups on a CU");
  static_assert(MG_FOLD_WAVES * MG_WAVE == 256, "mg_block_fold folds workgroups of 256 threads");
  // about eight workgroups per CU in all; each walks its share of a plane's tiles and adds to the plane's counter once
  hipLaunchKernelGGL((k_despeckle<T, K, VOTES>), mg_plane_grid(tiles_x * tiles_y, n, MG_DESPECKLE_WALK), dim3(256), 0, s, (const T*)d_src,
                     (T*)d_dst, n, h, w, (int)tiles_x, (int)(tiles_x * tiles_y), which, threshold, d_defects,
                     reinterpret_cast<unsigned long long*>(d_counts), d_votes);
  MG_CHECK_LAUNCH();
  return MG_OK;
}

template <bool VOTES>
int despeckle_entry(const void* d_src, void* d_dst, int dtype, int64_t n, int h, int w, int k, int which, double threshold,
                    const uint8_t* d_defects, int64_t* d_counts, int32_t* d_votes, void* stream) {
  const MgPlanes block = mg_planes_check(dtype, n, h, w, {d_src, d_dst});
  if (block == MG_PLANES_REFUSED || !d_src) return MG_EINVAL;
  if (k < 1 || k > MG_DESPECKLE_MAX_K || which < MG_OUTLIER_BRIGHT || which > MG_OUTLIER_ALL) return MG_EINVAL;
  if (!d_defects && which != MG_OUTLIER_ALL && !(threshold >= 0.0)) return MG_EINVAL;
  if (block == MG_PLANES_EMPTY) return MG_OK;
  hipStream_t s = mg_stream(stream);
  return mg_dispatch_pixel(dtype, [&](auto t) {
    using T = decltype(t);
    return k == 1 ? launch_despeckle<T, 1, VOTES>(d_src, d_dst, n, h, w, which, threshold, d_defects, d_counts, d_votes, s)
                  : launch_despeckle<T, 2, VOTES>(d_src, d_dst, n, h, w, which, threshold, d_defects, d_counts, d_votes, s);
  });
}

}  // namespace

extern "C" int mg_despeckle_planes(const void* d_src, void* d_dst, int dtype, int64_t n, int h, int w, int k, int which,
                                   double threshold, const uint8_t* d_defects, int64_t* d_counts, void* stream) {
  if (!d_dst || d_src == d_dst || reinterpret_cast<uintptr_t>(d_counts) % 8) return MG_EINVAL;
  return despeckle_entry<false>(d_src, d_dst, dtype, n, h, w, k, which, threshold, d_defects, d_counts, nullptr, stream);
}

extern "C" int mg_outlier_votes(const void* d_src, int dtype, int64_t n, int h, int w, int k, int which, double threshold,
                                int32_t* d_votes, void* stream) {
  if (!d_votes || reinterpret_cast<uintptr_t>(d_votes) % 4 || which == MG_OUTLIER_ALL || n > 0x7FFFFFFF) return MG_EINVAL;
  return despeckle_entry<true>(d_src, nullptr, dtype, n, h, w, k, which, threshold, nullptr, nullptr, d_votes, stream);
}
