// Bilinear 2 x 2 affine resampling of image planes (the `rotate` component): output pixel (oy, ox) samples the input at
// matrix @ (oy, ox) + offset, with the semantics of scipy.ndimage.affine_transform(order=1, mode="constant", cval=0).
// Oracle: tests/rotate_ref.py, the same float64 operations in the same order.
#include <algorithm>

#include "mg_common.h"

namespace {

// Output tile of one workgroup step: RT_LY x RT_STEPS rows of RT_LX lanes, PX pixels (one dword; a float64: two) per
// lane.  At any angle the source footprint of a tile is a square of about its diagonal -- a row strip at 45 degrees
// would touch a source line per pixel.
constexpr int RT_LX = 32, RT_LY = 8, RT_STEPS = 4, RT_ROWS = RT_LY * RT_STEPS;

template <class T>
struct RotPx {  // pixels per lane: one dword of u8 / u16 pixels
  static constexpr int N = sizeof(T) < 4 ? 4 / (int)sizeof(T) : 1;
};

// Two horizontal neighbours with one load (u8 / u16: the pair is at most a dword; it may sit at any alignment).
template <class T>
struct __attribute__((packed)) RotPair {
  T a, b;
};

struct RotArgs {
  double m[4], off[2];
};

// The value of output pixel (oy, ox) in float64.  Called for 0 <= oy < h only; ox may be any int (a lane's pixels
// outside [0, w) are computed from in-range reads -- or none -- and never stored).
template <class T>
__device__ __forceinline__ double rot_sample(const T* __restrict__ src, int h, int w, const RotArgs& a, int oy, int ox) {
#pragma clang fp contract(off)
  const double cy = (a.off[0] + (double)oy * a.m[0]) + (double)ox * a.m[1];
  const double cx = (a.off[1] + (double)oy * a.m[2]) + (double)ox * a.m[3];
  // (written so that a NaN coordinate is outside as well)
  if (!(cy >= 0.0 && cy <= (double)(h - 1) && cx >= 0.0 && cx <= (double)(w - 1))) return 0.0;
  const double fy = floor(cy), fx = floor(cx);
  const double ty = cy - fy, tx = cx - fx;
  const int y0 = (int)fy, x0 = (int)fx;  // in [0, h - 1] x [0, w - 1]
  const int y1 = min(y0 + 1, h - 1);
  const T* r0 = src + (int64_t)y0 * w;
  const T* r1 = src + (int64_t)y1 * w;
  double p00, p01, p10, p11;
  if (sizeof(T) < 4 && w >= 2) {
    // columns xa, xa + 1 with xa = min(x0, w - 2): in the last column both neighbours are the pair's second pixel
    const int xa = min(x0, w - 2);
    const RotPair<T> q0 = *reinterpret_cast<const RotPair<T>*>(r0 + xa);
    const RotPair<T> q1 = *reinterpret_cast<const RotPair<T>*>(r1 + xa);
    const bool last = x0 != xa;
    p00 = (double)(last ? q0.b : q0.a), p01 = (double)q0.b;
    p10 = (double)(last ? q1.b : q1.a), p11 = (double)q1.b;
  } else {
    const int x1 = min(x0 + 1, w - 1);
    p00 = (double)r0[x0], p01 = (double)r0[x1];
    p10 = (double)r1[x0], p11 = (double)r1[x1];
  }
  const double uy = 1.0 - ty, ux = 1.0 - tx;
  double v = (p00 * uy) * ux;
  v = v + (p01 * uy) * tx;
  v = v + (p10 * ty) * ux;
  v = v + (p11 * ty) * tx;
  return v;
}

template <class T>
__device__ __forceinline__ T rot_convert(double v) {
  if constexpr (std::is_integral<T>::value) {
    // floor(v + 0.5); v is a convex combination of pixels up to rounding, so the clamp only guards the cast
    const double r = floor(v + 0.5);
    constexpr double top = (double)(T)~(T)0;
    return (T)(r < 0.0 ? 0.0 : r > top ? top : r);
  } else {
    return (T)v;
  }
}

// Grid: x = workgroups that walk the tiles of a plane, y = workgroups that walk the planes.  Every lane owns the PX
// pixels of one ALIGNED dword of the output row: rows of an odd width start anywhere in a dword, so lane j of a row
// whose first pixel is the s-th of its dword covers columns PX * j - s .. PX * j - s + PX - 1; the first and last
// lane of a row store their pixels one by one, everything between is one dword store, 128 contiguous bytes per row of
// lanes.
template <class T>
__global__ __launch_bounds__(256) void k_affine_bilinear(const T* __restrict__ src, T* __restrict__ dst, int64_t n_planes,
                                                         int h, int w, RotArgs a, int tiles_x, int tiles_y,
                                                         double* __restrict__ d_minmax) {
  constexpr int PX = RotPx<T>::N;
  const int lx = threadIdx.x & (RT_LX - 1), ly = threadIdx.x / RT_LX;
  const int n_tiles = tiles_x * tiles_y;  // (the launcher keeps it below 2^31)
  const int64_t plane_elems = (int64_t)h * w;
  // pixel index of dst[0] within its dword (dst is aligned to its element size)
  const int64_t base_px = (int64_t)((reinterpret_cast<uintptr_t>(dst) / sizeof(T)) % PX);
  for (int64_t plane = blockIdx.y; plane < n_planes; plane += gridDim.y) {
    const T* ps = src + plane * plane_elems;
    T* pd = dst + plane * plane_elems;
    double vmin = INFINITY, vmax = -INFINITY;
    uint32_t imin = 0xFFFFFFFFu, imax = 0u;
    for (int tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
      const int tyi = tile / tiles_x, txi = tile - tyi * tiles_x;
#pragma unroll
      for (int st = 0; st < RT_STEPS; ++st) {
        const int oy = tyi * RT_ROWS + st * RT_LY + ly;
        if (oy >= h) continue;
        const int64_t row = plane * plane_elems + (int64_t)oy * w;  // element index of the row's first pixel in dst
        const int s = PX == 1 ? 0 : (int)((base_px + row) % PX);
        const int xs = (txi * RT_LX + lx) * PX - s;
        if (xs >= w) continue;
        T o[PX];
#pragma unroll
        for (int j = 0; j < PX; ++j) {
          const int ox = xs + j;
          o[j] = (ox >= 0 && ox < w) ? rot_convert<T>(rot_sample<T>(ps, h, w, a, oy, ox)) : (T)0;
        }
        T* prow = pd + (int64_t)oy * w;
        if (PX > 1 && (xs < 0 || xs + PX > w)) {
#pragma unroll
          for (int j = 0; j < PX; ++j)
            if (xs + j >= 0 && xs + j < w) prow[xs + j] = o[j];
        } else if constexpr (PX > 1) {
          uint32_t word = 0;
#pragma unroll
          for (int j = 0; j < PX; ++j) word |= (uint32_t)o[j] << (8 * (int)sizeof(T) * j);
          *reinterpret_cast<uint32_t*>(prow + xs) = word;
        } else {
          prow[xs] = o[0];
        }
        if (d_minmax) {
#pragma unroll
          for (int j = 0; j < PX; ++j) {
            if (xs + j < 0 || xs + j >= w) continue;
            if constexpr (std::is_integral<T>::value) {
              imin = min(imin, (uint32_t)o[j]);
              imax = max(imax, (uint32_t)o[j]);
            } else {
              vmin = mg_nanmin(vmin, (double)o[j]);
              vmax = mg_nanmax(vmax, (double)o[j]);
            }
          }
        }
      }
    }
    if (d_minmax) {  // (uniform over the workgroup)
      mg_block_minmax<1>(&vmin, &vmax, &imin, &imax, 1, d_minmax, plane);
      __syncthreads();  // the tail's shared rows are free again before the next plane's fold
    }
  }
}

template <class T>
int launch_affine(const void* d_src, void* d_dst, int64_t n_planes, int h, int w, const RotArgs& a, double* d_minmax,
                  hipStream_t s) {
  constexpr int PX = RotPx<T>::N;
  if ((reinterpret_cast<uintptr_t>(d_src) | reinterpret_cast<uintptr_t>(d_dst)) % sizeof(T)) return MG_EINVAL;
  // lanes per row: one more than the row's dwords when rows can start inside a dword
  const int64_t lanes = ((int64_t)w + PX - 1) / PX + (PX > 1 ? 1 : 0);
  const int64_t tiles_x = (lanes + RT_LX - 1) / RT_LX, tiles_y = ((int64_t)h + RT_ROWS - 1) / RT_ROWS;
  if (tiles_x * tiles_y > 0x7FFFFFFF) return MG_EINVAL;
  // ~MG_ROTATE_WALK workgroups in all walk the tiles (each ends with min/max atomics on its plane's one cache line)
  const unsigned gy = (unsigned)std::min<int64_t>(n_planes, MG_WALK_MAX_Y);
  const unsigned gx = (unsigned)std::max<int64_t>(1, std::min<int64_t>(tiles_x * tiles_y, MG_ROTATE_WALK / gy));
  static_assert(RT_LX * RT_LY == 256, "mg_block_minmax folds workgroups of 256 threads");
  hipLaunchKernelGGL((k_affine_bilinear<T>), dim3(gx, gy), dim3(RT_LX * RT_LY), 0, s, (const T*)d_src, (T*)d_dst, n_planes,
                     h, w, a, (int)tiles_x, (int)tiles_y, d_minmax);
  MG_CHECK_LAUNCH();
  return MG_OK;
}

}  // namespace

extern "C" int mg_affine_bilinear(const void* d_src, void* d_dst, int dtype, int64_t n_planes, int h, int w,
                                  const double* matrix, const double* offset, double* d_minmax, void* stream) {
  if (!d_src || !d_dst || d_src == d_dst || !matrix || !offset || n_planes < 0 || h < 0 || w < 0) return MG_EINVAL;
  if (dtype != MG_U8 && dtype != MG_U16 && dtype != MG_F32 && dtype != MG_F64) return MG_EINVAL;
  RotArgs a;
  for (int i = 0; i < 4; ++i) a.m[i] = matrix[i];
  for (int i = 0; i < 2; ++i) a.off[i] = offset[i];
  for (int i = 0; i < 4; ++i)
    if (!std::isfinite(a.m[i])) return MG_EINVAL;
  if (!std::isfinite(a.off[0]) || !std::isfinite(a.off[1])) return MG_EINVAL;
  if (n_planes == 0 || h == 0 || w == 0) return MG_OK;
  hipStream_t s = mg_stream(stream);
  return mg_dispatch_pixel(dtype, [&](auto t) {
    return launch_affine<decltype(t)>(d_src, d_dst, n_planes, h, w, a, d_minmax, s);
  });
}
