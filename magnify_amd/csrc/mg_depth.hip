// Depth stacks (the `project_depth` component): a contiguous block (N, Z, H, W) of focal series is folded to (N, H, W)
// -- maximum, mean or one chosen slice (mg_depth_project), the per-slice focus totals that choose the sharpest slice
// (mg_depth_focus_totals), and the per-pixel pick of the sharpest slice (mg_depth_fuse, "extended depth of field").
// The focus measure is the modified Laplacian ML = |2c - l - r| + |2c - u - d| with edge-clamped neighbours.
// Oracle: tests/depth_ref.py, the same integer / float64 operations in the same order.
#include "mg_planes.h"

namespace {

// ---- mg_depth_project ------------------------------------------------------------------------------------------------

template <class T>
struct DepthPx {  // pixels per lane: one dword of u8 / u16 pixels
  static constexpr int N = sizeof(T) < 4 ? 4 / (int)sizeof(T) : 1;
};
// The PX pixels of a lane in one load (a slice starts anywhere in a dword: the load may sit at any alignment).
template <class T>
struct __attribute__((packed)) DepthWord {
  T v[DepthPx<T>::N];
};
template <class T>
__device__ __forceinline__ DepthWord<T> depth_load(const T* p) {
  if constexpr (DepthPx<T>::N == 1) {
    DepthWord<T> q;
    q.v[0] = *p;
    return q;
  } else {
    return *reinterpret_cast<const DepthWord<T>*>(p);
  }
}

// The running value of one output pixel over z: max (NaN propagates, the first of equal values stays), the exact
// integer sum, or the float64 sum in slice order.
template <class T, int METHOD>
struct DepthFold {
  using A = std::conditional_t<METHOD == MG_DEPTH_MEAN, std::conditional_t<std::is_integral<T>::value, uint64_t, double>, T>;
  static __device__ __forceinline__ A first(T v) {
    if constexpr (METHOD == MG_DEPTH_MEAN && !std::is_integral<T>::value) return 0.0 + (double)v;
    return (A)v;
  }
  static __device__ __forceinline__ A next(A a, T v) {
    if constexpr (METHOD == MG_DEPTH_MEAN) {
      return a + (A)v;
    } else if constexpr (std::is_integral<T>::value) {
      return v > a ? v : a;
    } else {
      return (a != a) ? a : (v != v) ? v : (v > a ? v : a);
    }
  }
  static __device__ __forceinline__ T last(A a, int z) {
    if constexpr (METHOD != MG_DEPTH_MEAN) {
      return a;
    } else if constexpr (std::is_integral<T>::value) {
      return (T)rint((double)a / (double)z);  // half to even; a mean never leaves the dtype's range
    } else {
      return (T)(a / (double)z);
    }
  }
};

// Grid: mg_plane_grid, the items of a plane being blocks of 256 lanes (the lanes stride over the plane themselves).  The
// planes of a stack are contiguous, so a plane is one run of h * w pixels: every lane owns the PX pixels of one ALIGNED dword of
// the output (a plane of odd size starts anywhere in a dword: lane j of a plane whose first pixel is the s-th of its
// dword covers pixels PX * j - s .. PX * j - s + PX - 1); the first and last lane of a plane take their pixels one
// by one, every other lane reads one (unaligned) dword per slice and stores one aligned dword.  METHOD PICK reads
// slice pick[stack] only (clamped into [0, z): the caller has checked it).
template <class T, int METHOD>
__global__ __launch_bounds__(256) void k_depth_project(const T* __restrict__ src, T* __restrict__ dst, int64_t n_stacks,
                                                       int z, int64_t plane, const int32_t* __restrict__ pick,
                                                       int64_t lanes) {
  constexpr int PX = DepthPx<T>::N;
  using F = DepthFold<T, METHOD>;
  const int64_t base_px = (int64_t)((reinterpret_cast<uintptr_t>(dst) / sizeof(T)) % PX);
  MG_FOR_BLOCK_PLANES(stack, n_stacks) {
    const T* ps = src + stack * z * plane;
    T* pd = dst + stack * plane;
    int z0 = 0, z1 = z;
    if (METHOD == MG_DEPTH_PICK) {
      z0 = min(max(pick[stack], 0), z - 1);
      z1 = z0 + 1;
    }
    const int s = PX == 1 ? 0 : (int)((base_px + stack * plane) % PX);
    for (int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; j < lanes; j += (int64_t)gridDim.x * blockDim.x) {
      const int64_t xs = j * PX - s;
      if (xs >= plane) break;
      if (xs >= 0 && xs + PX <= plane) {
        const T* p = ps + xs + (int64_t)z0 * plane;
        DepthWord<T> q = depth_load(p);
        typename F::A a[PX];
#pragma unroll
        for (int e = 0; e < PX; ++e) a[e] = F::first(q.v[e]);
#pragma unroll 4
        for (int zi = z0 + 1; zi < z1; ++zi) {
          p += plane;
          q = depth_load(p);
#pragma unroll
          for (int e = 0; e < PX; ++e) a[e] = F::next(a[e], q.v[e]);
        }
        if constexpr (PX > 1) {
          uint32_t word = 0;
#pragma unroll
          for (int e = 0; e < PX; ++e) word |= (uint32_t)F::last(a[e], z) << (8 * (int)sizeof(T) * e);
          *reinterpret_cast<uint32_t*>(pd + xs) = word;
        } else {
          pd[xs] = F::last(a[0], z);
        }
      } else {
        for (int e = 0; e < PX; ++e) {
          const int64_t x = xs + e;
          if (x < 0 || x >= plane) continue;
          const T* p = ps + x + (int64_t)z0 * plane;
          typename F::A a = F::first(*p);
          for (int zi = z0 + 1; zi < z1; ++zi) {
            p += plane;
            a = F::next(a, *p);
          }
          pd[x] = F::last(a, z);
        }
      }
    }
  }
}

template <class T, int METHOD>
int launch_project(const void* d_src, void* d_dst, int64_t n, int z, int h, int w, const int32_t* d_pick, hipStream_t s) {
  constexpr int PX = DepthPx<T>::N;
  const int64_t plane = (int64_t)h * w;
  // lanes per plane: one more than the plane's dwords when a plane can start inside a dword
  const int64_t lanes = (plane + PX - 1) / PX + (PX > 1 ? 1 : 0);
  // 16 workgroups per CU in all when there is that much work; each walks its share of the plane
  hipLaunchKernelGGL((k_depth_project<T, METHOD>), mg_plane_grid((lanes + 255) / 256, n, MG_DEPTH_PROJECT_WALK), dim3(256), 0, s,
                     (const T*)d_src, (T*)d_dst, n, z, plane, d_pick, lanes);
  MG_CHECK_LAUNCH();
  return MG_OK;
}

// ---- the modified Laplacian -------------------------------------------------------------------------------------------

template <class T>
using DepthM = std::conditional_t<std::is_integral<T>::value, uint32_t, double>;

template <class T>
__device__ __forceinline__ DepthM<T> depth_ml(T c, T l, T r, T u, T d) {
#pragma clang fp contract(off)
  if constexpr (std::is_integral<T>::value) {
    const int c2 = 2 * (int)c;
    return (uint32_t)abs(c2 - (int)l - (int)r) + (uint32_t)abs(c2 - (int)u - (int)d);
  } else {
    const double c2 = 2.0 * (double)c;
    return fabs((c2 - (double)l) - (double)r) + fabs((c2 - (double)u) - (double)d);
  }
}

// ---- mg_depth_focus_totals -------------------------------------------------------------------------------------------

// A workgroup step covers 256 columns x FT_ROWS rows of one slice; a thread walks down its column with the pixel above,
// the pixel and the pixel below in registers (one new centre load per row, the two horizontal neighbours are the
// neighbouring lanes' lines).
constexpr int FT_ROWS = 16;

template <class T>
__global__ __launch_bounds__(256) void k_depth_focus_totals(const T* __restrict__ src, int64_t n_slices, int h, int w,
                                                            int tiles_x, int tiles_y, void* __restrict__ totals) {
  using A = mg_acc_t<T>;
  const int n_tiles = tiles_x * tiles_y;
  MG_FOR_BLOCK_PLANES(slice, n_slices) {
    const T* p = src + slice * ((int64_t)h * w);
    A acc = 0;
    MG_FOR_BLOCK_ITEMS(tile, n_tiles) {
      const MgTile at = mg_tile(tile, tiles_x);
      const int x = at.x * 256 + (int)threadIdx.x;
      if (x >= w) continue;
      const int y0 = at.y * FT_ROWS, y1 = min(y0 + FT_ROWS, h);
      const int xl = max(x - 1, 0), xr = min(x + 1, w - 1);
      T u = p[(int64_t)max(y0 - 1, 0) * w + x], c = p[(int64_t)y0 * w + x];
      for (int y = y0; y < y1; ++y) {
        const T* row = p + (int64_t)y * w;
        const T d = p[(int64_t)min(y + 1, h - 1) * w + x];
        acc += (A)depth_ml<T>(c, row[xl], row[xr], u, d);
        u = c;
        c = d;
      }
    }
    const A total = mg_block_fold(acc, [](A a, A b) { return a + b; });
    if (threadIdx.x == 0) {
      if constexpr (std::is_integral<T>::value) {
        atomicAdd(reinterpret_cast<unsigned long long*>(totals) + slice, (unsigned long long)total);
      } else {
        atomicAdd(reinterpret_cast<double*>(totals) + slice, total);
      }
    }
  }
}

template <class T>
int launch_focus_totals(const void* d_src, int64_t n, int z, int h, int w, void* d_totals, hipStream_t s) {
  const int64_t n_slices = n * z;
  if (mg_zero_async(d_totals, (size_t)n_slices * 8, s) != hipSuccess) return MG_ELAUNCH;
  const int64_t tiles_x = ((int64_t)w + 255) / 256, tiles_y = ((int64_t)h + FT_ROWS - 1) / FT_ROWS;
  if (tiles_x * tiles_y > 0x7FFFFFFF) return MG_EINVAL;
  static_assert(MG_FOLD_WAVES * MG_WAVE == 256, "mg_block_fold folds workgroups of 256 threads");
  // one atomic per workgroup and slice: at most MG_DEPTH_FOCUS_WALK_PER_SLICE workgroups share a slice
  hipLaunchKernelGGL((k_depth_focus_totals<T>), mg_plane_grid(tiles_x * tiles_y, n_slices, MG_DEPTH_FOCUS_WALK, MG_DEPTH_FOCUS_WALK_PER_SLICE), dim3(256), 0, s,
                     (const T*)d_src, n_slices, h, w, (int)tiles_x, (int)tiles_y, d_totals);
  MG_CHECK_LAUNCH();
  return MG_OK;
}

// ---- mg_depth_fuse ---------------------------------------------------------------------------------------------------

// One workgroup owns an output tile of DF x DF pixels of one stack and loops over z (mg_plane_grid with no budget: a
// workgroup per tile).  LDS, sized by the launch for the window half-width k: region A holds the slice's tile with a
// halo of k + 1 (PH x PH pixels, mg_fill_tile with DF_NLOAD loads of a thread in flight), region B
// its ML (MH x MH, MH = DF + 2k, zero outside the plane).  The row sums (MH rows x DF columns) then take region A's
// place -- every thread has its own four pixels in registers by then -- and the column sums of those are the
// measures.  Lanes run along x in every pass: 32 consecutive words per half wave, no bank conflict.  A thread owns
// four consecutive rows of one column: their windows overlap, so the column pass reads 2k + 4 row sums, not 4 (2k + 1),
// and still adds every measure's terms top to bottom.
constexpr int DF = MG_DEPTH_TILE, DF_PER_THREAD = DF * DF / 256;
static_assert(DF == 32 && DF_PER_THREAD == 4, "a thread's outputs: column t & 31, rows 4 (t >> 5) + i");

// i / d for 0 <= i < 4096 and 32 <= d <= 64 without the division: (i * ceil(2^20 / d)) >> 20 (the error of the
// reciprocal, below i / 2^20 < 1 / 256, never reaches the next integer; tests/test_cpu_depth.py checks every i and d).
__device__ __forceinline__ int depth_div(int i, uint32_t inv) { return (int)(((uint32_t)i * inv) >> 20); }
static_assert((DF + 2 * MG_DEPTH_MAX_K + 2) * (DF + 2 * MG_DEPTH_MAX_K + 2) <= 4096 && DF + 2 * MG_DEPTH_MAX_K + 2 <= 64,
              "depth_div's range");
struct DepthSide {  // the side of a padded tile, known at the launch (mg_fill_tile)
  int n;
  uint32_t inv;
  __device__ __forceinline__ int row(int i) const { return depth_div(i, inv); }
};
constexpr int DF_NLOAD = 8;  // DESIGN.md, "Plane filters: what they share", has the measurements

template <class T>
static inline size_t depth_fuse_lds(int k, size_t* region_a) {
  const size_t ph = DF + 2 * k + 2, mh = DF + 2 * k;
  const size_t a = std::max(ph * ph * sizeof(T), mh * DF * sizeof(DepthM<T>));
  *region_a = (a + 7) / 8 * 8;
  return *region_a + mh * mh * sizeof(DepthM<T>);
}

template <class T>
__global__ __launch_bounds__(256) void k_depth_fuse(const T* __restrict__ src, T* __restrict__ dst, uint8_t* __restrict__ index,
                                                    int64_t n_stacks, int z, int h, int w, int k, int tiles_x,
                                                    uint32_t region_a) {
  using M = DepthM<T>;
  extern __shared__ __attribute__((aligned(8))) unsigned char s_depth[];
  T* s_px = reinterpret_cast<T*>(s_depth);
  M* s_rs = reinterpret_cast<M*>(s_depth);
  M* s_ml = reinterpret_cast<M*>(s_depth + region_a);
  const int ph = DF + 2 * k + 2, mh = DF + 2 * k, win = 2 * k + 1;
  const uint32_t inv_ph = ((1u << 20) + ph - 1) / ph, inv_mh = ((1u << 20) + mh - 1) / mh;
  const int t = threadIdx.x, ox = t & (DF - 1), oy0 = DF_PER_THREAD * (t / DF);
  const int y0 = mg_tile(blockIdx.x, tiles_x).y * DF, x0 = mg_tile(blockIdx.x, tiles_x).x * DF;
  const int64_t plane = (int64_t)h * w;
  MG_FOR_BLOCK_PLANES(stack, n_stacks) {
    M best[DF_PER_THREAD];
    T best_px[DF_PER_THREAD];
    int best_z[DF_PER_THREAD];
    for (int zi = 0; zi < z; ++zi) {
      const T* p = src + (stack * z + zi) * plane;
      mg_fill_tile<DF_NLOAD>(s_px, p, h, w, y0, x0, k + 1, DepthSide{ph, inv_ph}, false);  // (the loop ends in a barrier)
      for (int i = t; i < mh * mh; i += 256) {
        const int my = depth_div(i, inv_mh), mx = i - my * mh;
        const int gy = y0 - k + my, gx = x0 - k + mx;
        M ml = 0;
        if (gy >= 0 && gy < h && gx >= 0 && gx < w) {
          const T* c = s_px + (my + 1) * ph + mx + 1;
          ml = depth_ml<T>(c[0], c[-1], c[1], c[-ph], c[ph]);
        }
        s_ml[i] = ml;
      }
      T px[DF_PER_THREAD];
#pragma unroll
      for (int i = 0; i < DF_PER_THREAD; ++i) px[i] = s_px[(oy0 + i + k + 1) * ph + ox + k + 1];
      __syncthreads();
      // per row the 2k + 1 columns left to right ...
      for (int i = t; i < mh * DF; i += 256) {
        const M* m = s_ml + (i / DF) * mh + (i & (DF - 1));
        M acc = 0;
        for (int j = 0; j < win; ++j) acc += m[j];
        s_rs[i] = acc;
      }
      __syncthreads();
      // ... then the 2k + 1 row sums top to bottom: row sum m of the thread's rows is term m - i of output i
      M sum[DF_PER_THREAD];
#pragma unroll
      for (int i = 0; i < DF_PER_THREAD; ++i) sum[i] = 0;
      const M* r = s_rs + oy0 * DF + ox;
      for (int m = 0; m < win + DF_PER_THREAD - 1; ++m) {
        const M v = r[m * DF];
#pragma unroll
        for (int i = 0; i < DF_PER_THREAD; ++i)
          if (m >= i && m - i < win) sum[i] += v;
      }
#pragma unroll
      for (int i = 0; i < DF_PER_THREAD; ++i) {
        M acc = sum[i];
        const bool take = zi == 0 || acc > best[i];
        if constexpr (!std::is_integral<T>::value) {
          if (zi == 0) acc = acc == acc ? acc : -INFINITY;  // a NaN measure never wins, not even as the first
        }
        if (take) best[i] = acc, best_px[i] = px[i], best_z[i] = zi;
      }
      __syncthreads();  // region A is free for the next slice
    }
#pragma unroll
    for (int i = 0; i < DF_PER_THREAD; ++i) {
      const int y = y0 + oy0 + i, x = x0 + ox;
      if (y < h && x < w) {
        const int64_t o = stack * plane + (int64_t)y * w + x;
        dst[o] = best_px[i];
        if (index) index[o] = (uint8_t)best_z[i];
      }
    }
  }
}

template <class T>
int launch_fuse(const void* d_src, void* d_dst, uint8_t* d_index, int64_t n, int z, int h, int w, int k, hipStream_t s) {
  const int64_t tiles_x = ((int64_t)w + DF - 1) / DF, tiles_y = ((int64_t)h + DF - 1) / DF;
  if (tiles_x * tiles_y > 0x7FFFFFFF) return MG_EINVAL;
  size_t region_a;
  const size_t lds = depth_fuse_lds<T>(k, &region_a);
  static_assert(sizeof(double) * ((DF + 2 * MG_DEPTH_MAX_K + 2) * (DF + 2 * MG_DEPTH_MAX_K + 2) +
                                  (DF + 2 * MG_DEPTH_MAX_K) * (DF + 2 * MG_DEPTH_MAX_K)) <= 65536,
                "the largest window of float64 pixels fits the 64 KiB a workgroup may ask for");
  hipLaunchKernelGGL((k_depth_fuse<T>), mg_plane_grid(tiles_x * tiles_y, n), dim3(256), lds, s, (const T*)d_src, (T*)d_dst,
                     d_index, n, z, h, w, k, (int)tiles_x, (uint32_t)region_a);
  MG_CHECK_LAUNCH();
  return MG_OK;
}

}  // namespace

extern "C" int mg_depth_project(const void* d_src, void* d_dst, int dtype, int64_t n, int z, int h, int w, int method,
                                const int32_t* d_pick, void* stream) {
  const MgPlanes block = mg_planes_check(dtype, n, h, w, {d_src, d_dst});
  if (block == MG_PLANES_REFUSED || z < 1 || !d_src || !d_dst || d_src == d_dst) return MG_EINVAL;
  if (method != MG_DEPTH_MAX && method != MG_DEPTH_MEAN && method != MG_DEPTH_PICK) return MG_EINVAL;
  if (method == MG_DEPTH_PICK && !d_pick) return MG_EINVAL;
  if (block == MG_PLANES_EMPTY) return MG_OK;
  hipStream_t s = mg_stream(stream);
  return mg_dispatch_pixel(dtype, [&](auto t) {
    using T = decltype(t);
    switch (method) {
      case MG_DEPTH_MAX: return launch_project<T, MG_DEPTH_MAX>(d_src, d_dst, n, z, h, w, d_pick, s);
      case MG_DEPTH_MEAN: return launch_project<T, MG_DEPTH_MEAN>(d_src, d_dst, n, z, h, w, d_pick, s);
      default: return launch_project<T, MG_DEPTH_PICK>(d_src, d_dst, n, z, h, w, d_pick, s);
    }
  });
}

extern "C" int mg_depth_focus_totals(const void* d_src, int dtype, int64_t n, int z, int h, int w, void* d_totals,
                                     void* stream) {
  const MgPlanes block = mg_planes_check(dtype, n, h, w, {d_src});
  if (block == MG_PLANES_REFUSED || z < 1 || !d_src || !d_totals || reinterpret_cast<uintptr_t>(d_totals) % 8) return MG_EINVAL;
  if (block == MG_PLANES_EMPTY) return MG_OK;
  hipStream_t s = mg_stream(stream);
  return mg_dispatch_pixel(dtype, [&](auto t) {
    return launch_focus_totals<decltype(t)>(d_src, n, z, h, w, d_totals, s);
  });
}

extern "C" int mg_depth_fuse(const void* d_src, int dtype, int64_t n, int z, int h, int w, int k, void* d_dst,
                             uint8_t* d_index, void* stream) {
  const MgPlanes block = mg_planes_check(dtype, n, h, w, {d_src, d_dst});
  if (block == MG_PLANES_REFUSED || z < 1 || !d_src || !d_dst || d_src == d_dst) return MG_EINVAL;
  if (z > MG_DEPTH_MAX_Z || k < 1 || k > MG_DEPTH_MAX_K) return MG_EINVAL;
  if (block == MG_PLANES_EMPTY) return MG_OK;
  hipStream_t s = mg_stream(stream);
  return mg_dispatch_pixel(dtype, [&](auto t) {
    return launch_fuse<decltype(t)>(d_src, d_dst, d_index, n, z, h, w, k, s);
  });
}
