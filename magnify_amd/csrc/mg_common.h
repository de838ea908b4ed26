// Shared device/host helpers for the gfx950 marker-detection kernels.
// Built with -ffp-contract=off: float64 sequences must round exactly like NumPy's.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include <type_traits>

#include "../../include/magnify_hip.h"

#define MG_WAVE 64

// Keyed scoring prefilter (mg_score.hip): super-tiles of MG_SCORE_SUBY x MG_SCORE_SUBX centre tiles (128 x 256
// positions) with their edge window as bytes in LDS (a pixel's orientation bin | its right neighbour's << 4), row
// stride 308 B = 77 dwords (odd: rows rotate through the banks); radii up to MG_SCORE_MAX_R (window 180 x 308),
// perimeters up to 2 * MG_SCORE_MAX_PAIRS points.
#define MG_SCORE_TILE 64
#define MG_SCORE_SUBY 2
#define MG_SCORE_SUBX 4
#define MG_SCORE_MAX_R 26
#define MG_SCORE_MAX_PAIRS 80
#define MG_SCORE_WSTRIDE (MG_SCORE_TILE * MG_SCORE_SUBX + 2 * MG_SCORE_MAX_R)

// The 32-bit circle key of the keyed path: tile << 17 | radius layer << 12 | row << 6 | col, where (row, col) is the
// position of the centre in its 64 x 64 tile of the grid padded by max_r on every side and layer = r - min_r.
// Ascending keys = the build's canonical (tile, r, row, col) order; the low 17 bits are the circle's bit index in the
// tile's de-duplication layers.  15 + 5 + 12 bits: mg_key_layout refuses what does not fit.
constexpr int MG_KEY_ROW_SHIFT = 6, MG_KEY_LAYER_SHIFT = 12, MG_KEY_TILE_SHIFT = 17;
constexpr uint32_t MG_KEY_POS_MASK = 63u, MG_KEY_LAYER_MASK = 31u;
constexpr uint32_t MG_KEY_CENTRE_MASK = (1u << MG_KEY_LAYER_SHIFT) - 1u, MG_KEY_LOW17_MASK = (1u << MG_KEY_TILE_SHIFT) - 1u;
constexpr uint32_t MG_NO_KEY = 0xFFFFFFFFu;  // candidate rejected by the radius / on-image filter
constexpr int MG_KEY_MAX_TILES = 1 << (32 - MG_KEY_TILE_SHIFT), MG_KEY_MAX_LAYERS = 1 << (MG_KEY_TILE_SHIFT - MG_KEY_LAYER_SHIFT);
__host__ __device__ __forceinline__ uint32_t mg_key_pack(int tile, int layer, int row, int col) {
  return ((uint32_t)tile << MG_KEY_TILE_SHIFT) | ((uint32_t)layer << MG_KEY_LAYER_SHIFT) |
         (uint32_t)((row << MG_KEY_ROW_SHIFT) + col);
}
__host__ __device__ __forceinline__ uint32_t mg_key_from_low17(int tile, uint32_t low17) {
  return ((uint32_t)tile << MG_KEY_TILE_SHIFT) | low17;
}
__host__ __device__ __forceinline__ uint32_t mg_key_tile(uint32_t key) { return key >> MG_KEY_TILE_SHIFT; }
__host__ __device__ __forceinline__ uint32_t mg_key_low17(uint32_t key) { return key & MG_KEY_LOW17_MASK; }
__host__ __device__ __forceinline__ int mg_key_layer(uint32_t key) { return (int)((key >> MG_KEY_LAYER_SHIFT) & MG_KEY_LAYER_MASK); }
__host__ __device__ __forceinline__ int mg_key_row(uint32_t key) { return (int)((key >> MG_KEY_ROW_SHIFT) & MG_KEY_POS_MASK); }
__host__ __device__ __forceinline__ int mg_key_col(uint32_t key) { return (int)(key & MG_KEY_POS_MASK); }
// mg_dedup_layout for a launcher that takes keys: MG_EINVAL also where a tile or a radius layer has no key.
static inline int mg_key_layout(int h, int w, int min_r, int max_r, int* ntr, int* ntc, int* nr) {
  int64_t n_layers, words;
  if (mg_dedup_layout(h, w, min_r, max_r, ntr, ntc, &n_layers, &words) != MG_OK) return MG_EINVAL;
  *nr = max_r - min_r + 1;
  return ((int64_t)*ntr * *ntc >= MG_KEY_MAX_TILES || *nr > MG_KEY_MAX_LAYERS) ? MG_EINVAL : MG_OK;
}

#define MG_CHECK_LAUNCH()                          \
  do {                                             \
    hipError_t e_ = hipGetLastError();             \
    if (e_ != hipSuccess) return MG_ELAUNCH;       \
  } while (0)

static inline hipStream_t mg_stream(void* s) { return reinterpret_cast<hipStream_t>(s); }

// Clearing small counters / bitmaps: a kernel, not hipMemsetAsync.  The calls of this library are captured into
// hipGraphs by the host side (hotpath.CircleFinder), and memset nodes of one captured graph were found to be replayed
// with another graph's parameters once a second graph had been captured (ROCm 7.2: a counter came back as 0x10101034);
// kernel nodes carry their own arguments.
static __global__ void mg_k_zero_words(uint32_t* __restrict__ p, int64_t n_words) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n_words; i += (int64_t)gridDim.x * blockDim.x) p[i] = 0u;
}
static inline hipError_t mg_zero_async(void* p, size_t bytes, hipStream_t s) {  // bytes: a multiple of 4
  const int64_t n = (int64_t)(bytes / 4);
  if (n == 0) return hipSuccess;
  const int blocks = (int)(n < 256 * 1024 ? (n + 255) / 256 : MG_ZERO_WALK);
  hipLaunchKernelGGL(mg_k_zero_words, dim3(blocks), dim3(256), 0, s, reinterpret_cast<uint32_t*>(p), n);
  return hipGetLastError();
}

__host__ __device__ static inline int mg_elem_size(int dtype) {
  return dtype == MG_U8 ? 1 : dtype == MG_U16 ? 2 : dtype == MG_F32 ? 4 : 8;
}

// The pixel-type switch of the C ABI, once: f(T{}) with T the element type of `dtype`; MG_EINVAL for any other code.
template <class F>
static inline int mg_dispatch_pixel(int dtype, F&& f) {
  switch (dtype) {
    case MG_U8: return f(uint8_t{});
    case MG_U16: return f(uint16_t{});
    case MG_F32: return f(float{});
    case MG_F64: return f(double{});
  }
  return MG_EINVAL;
}
// Accumulator of masked sums: exact for integer pixels (below 2^53 in the float64 result), float64 otherwise.
template <class T>
using mg_acc_t = std::conditional_t<std::is_integral<T>::value, long long, double>;

// A byte mask of gathered windows as every window kernel reads it: the L x L bytes of marker g at timepoint t start at
// p + g * stride_m + t * stride_t (a stride of 0: one mask for all markers / timepoints).
struct MgMaskView {
  const uint8_t* p;
  int64_t stride_m, stride_t;
  __device__ __forceinline__ const uint8_t* at(int64_t g, int64_t t) const { return p + g * stride_m + t * stride_t; }
};
static inline bool mg_mask_view_ok(const MgMaskView& v) { return v.p && v.stride_m >= 0 && v.stride_t >= 0; }

// Stitch crop (stitch.py:22-39): every tile keeps rows / columns [clip, clip + hy / hx) -- half the overlap goes on
// each side, the odd pixel on the far one -- and the n_tr x n_tc kept parts are laid side by side.
struct MgStitchGeom {
  int clip, hy, hx, h_out, w_out;
};
static inline MgStitchGeom mg_stitch_geom(int ty, int tx, int overlap, int n_tr, int n_tc) {
  const int clip = overlap / 2, rem = overlap % 2;
  const int hy = ty - 2 * clip - rem, hx = tx - 2 * clip - rem;
  return {clip, hy, hx, n_tr * hy, n_tc * hx};
}

// cv::borderInterpolate(p, n, BORDER_REFLECT_101)
__device__ __forceinline__ int mg_reflect101(int p, int n) {
  if (n == 1) return 0;
  while (p < 0 || p >= n) p = p < 0 ? -p : 2 * n - 2 - p;
  return p;
}

// n (1..32) consecutive bits of a linear (y * w + x) bitmap from bit index bit0 on.  The second word is read only when
// the group reaches into it: for loads that sit behind data-dependent branches anyway (mg_edges.hip has the
// branch-free form for loads that are meant to be in flight together).
__device__ __forceinline__ uint32_t mg_bits_at(const uint32_t* __restrict__ bits, int64_t bit0, int n) {
  const int64_t wi = bit0 >> 5;
  const int sh = (int)(bit0 & 31);
  uint64_t two = bits[wi];
  if (sh + n > 32) two |= (uint64_t)bits[wi + 1] << 32;
  const uint32_t v = (uint32_t)(two >> sh);
  return n >= 32 ? v : (v & ((1u << n) - 1u));
}

// Load element idx of a scalar-or-image operand as float64.
__device__ __forceinline__ double mg_load_f64(const void* p, int dtype, int64_t idx) {
  switch (dtype) {
    case MG_U8: return (double)((const uint8_t*)p)[idx];
    case MG_U16: return (double)((const uint16_t*)p)[idx];
    case MG_F32: return (double)((const float*)p)[idx];
    default: return ((const double*)p)[idx];
  }
}

// i = (a * nb + b) * nc + c of a grid-stride loop, taken apart; row = a * nb + b.  `small` (uniform): the loop's total
// fits 31 bits, so the divisions are 32-bit ones.
struct MgIndex3 {
  int64_t row;
  int a, b, c;
};
__device__ __forceinline__ MgIndex3 mg_split3(int64_t i, bool small, int nb, int nc) {
  if (small) {
    const uint32_t u = (uint32_t)i, r = u / (uint32_t)nc, a = r / (uint32_t)nb;
    return {(int64_t)r, (int)a, (int)(r - a * (uint32_t)nb), (int)(u - r * (uint32_t)nc)};
  }
  const int64_t r = i / nc;
  const int a = (int)(r / nb);
  return {r, a, (int)(r - (int64_t)a * nb), (int)(i - r * nc)};
}

// The NaN every kernel writes where a result has nothing to stand on (an empty selection, a window without a threshold).
constexpr double MG_QNAN = __builtin_nan("");

// NaN-propagating max / min, as np.max / np.min.
__device__ __forceinline__ double mg_nanmax(double a, double b) { return (a != a) ? a : (b != b) ? b : (a > b ? a : b); }
__device__ __forceinline__ double mg_nanmin(double a, double b) { return (a != a) ? a : (b != b) ? b : (a < b ? a : b); }

__device__ __forceinline__ double mg_wave_nanmax(double v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v = mg_nanmax(v, __shfl_xor(v, off));
  return v;
}
__device__ __forceinline__ double mg_wave_nanmin(double v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v = mg_nanmin(v, __shfl_xor(v, off));
  return v;
}

// Look first, with a load that bypasses the (non-coherent) L1: workgroups that finish together would otherwise all
// see the same stale value and all go through the compare-and-swap, one after the other on one cache line.
__device__ __forceinline__ void mg_atomic_nanmax(double* addr, double v) {
  unsigned long long* a = reinterpret_cast<unsigned long long*>(addr);
  unsigned long long old = __hip_atomic_load(a, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  while (true) {
    double cur = __longlong_as_double((long long)old);
    if (cur != cur) return;                // already NaN
    if (v == v && !(v > cur)) return;      // not larger (and not NaN)
    unsigned long long seen = atomicCAS(a, old, (unsigned long long)__double_as_longlong(v));
    if (seen == old) return;
    old = seen;
  }
}
__device__ __forceinline__ void mg_atomic_nanmin(double* addr, double v) {
  unsigned long long* a = reinterpret_cast<unsigned long long*>(addr);
  unsigned long long old = __hip_atomic_load(a, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  while (true) {
    double cur = __longlong_as_double((long long)old);
    if (cur != cur) return;
    if (v == v && !(v < cur)) return;
    unsigned long long seen = atomicCAS(a, old, (unsigned long long)__double_as_longlong(v));
    if (seen == old) return;
    old = seen;
  }
}

// The per-plane min/max tail of the kernels that feed to_uint8 (utils.py:24-26).  Contract: d_minmax is
// double[n_planes][2], pre-initialised by the caller to {+inf, -inf}; every workgroup folds what its threads saw of PB
// consecutive planes from plane0 on (np <= PB of them in use) and publishes it with mg_atomic_nanmin / _nanmax, one
// thread per plane.  A workgroup that saw nothing of a plane -- its running values are still the identity
// (+inf, -inf), or (0xFFFFFFFF, 0) in the integer form -- leaves the plane's slot alone; NaN propagates as in np.min /
// np.max (mg_nanmin / mg_nanmax; once a slot is NaN it stays NaN).  Workgroups of MG_MINMAX_WAVES * 64 = 256 threads:
// every caller is a __launch_bounds__(256) kernel launched with dim3(256).  Called by all threads (it synchronises).
// A thread's running values of a plane are the float64 pair, or, where the kernel kept integer pixels in uint32
// registers and saw one, the integer pair (a kernel instance uses one of the two; the other stays at its identity).
constexpr int MG_MINMAX_WAVES = 4;
template <int PB, class I>
__device__ __forceinline__ void mg_block_minmax_f64(const double* vmin, const double* vmax, int np, double* d_minmax,
                                                    I plane0) {
  __shared__ double s_min[PB][MG_MINMAX_WAVES], s_max[PB][MG_MINMAX_WAVES];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int b = 0; b < PB; ++b) {
    const double a = mg_wave_nanmin(vmin[b]), c = mg_wave_nanmax(vmax[b]);
    if (lane == 0) {
      s_min[b][wave] = a;
      s_max[b][wave] = c;
    }
  }
  __syncthreads();
  if (threadIdx.x < np) {
    const int b = threadIdx.x;
    double a = s_min[b][0], c = s_max[b][0];
    for (int i = 1; i < MG_MINMAX_WAVES; ++i) {
      a = mg_nanmin(a, s_min[b][i]);
      c = mg_nanmax(c, s_max[b][i]);
    }
    if (!(a == INFINITY && c == -INFINITY)) {
      mg_atomic_nanmin(d_minmax + 2 * (plane0 + b), a);
      mg_atomic_nanmax(d_minmax + 2 * (plane0 + b) + 1, c);
    }
  }
}
// (a kernel that keeps both pairs: the integer one, where it saw a pixel, takes the place of the float64 one)
template <int PB, class I>
__device__ __forceinline__ void mg_block_minmax(double* vmin, double* vmax, const uint32_t* imin, const uint32_t* imax,
                                                int np, double* d_minmax, I plane0) {
#pragma unroll
  for (int b = 0; b < PB; ++b)
    if (imin[b] <= imax[b]) vmin[b] = (double)imin[b], vmax[b] = (double)imax[b];
  mg_block_minmax_f64<PB>(vmin, vmax, np, d_minmax, plane0);
}
// The same for integer pixels kept as uint32 (no NaN; the identity is min > max).
template <int PB, class I>
__device__ __forceinline__ void mg_block_minmax_u32(const uint32_t* imin, const uint32_t* imax, int np, double* d_minmax,
                                                    I plane0) {
  static_assert(MG_MINMAX_WAVES == 4, "the fold below is written out for four waves");
  __shared__ uint32_t s_min[PB][MG_MINMAX_WAVES], s_max[PB][MG_MINMAX_WAVES];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int b = 0; b < PB; ++b) {
    uint32_t a = imin[b], c = imax[b];
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
      a = min(a, (uint32_t)__shfl_xor((int)a, off));
      c = max(c, (uint32_t)__shfl_xor((int)c, off));
    }
    if (lane == 0) s_min[b][wave] = a, s_max[b][wave] = c;
  }
  __syncthreads();
  if (threadIdx.x < np) {
    const int b = threadIdx.x;
    const uint32_t a = min(min(s_min[b][0], s_min[b][1]), min(s_min[b][2], s_min[b][3]));
    const uint32_t c = max(max(s_max[b][0], s_max[b][1]), max(s_max[b][2], s_max[b][3]));
    if (a <= c) {
      mg_atomic_nanmin(d_minmax + 2 * (plane0 + b), (double)a);
      mg_atomic_nanmax(d_minmax + 2 * (plane0 + b) + 1, (double)c);
    }
  }
}

// Inclusive prefix sum over the 64 lanes on the VALU's DPP paths: Kogge-Stone inside each row of 16
// (row_shr 1, 2, 4, 8), then the row totals (row_bcast:15 into rows 1 and 3, row_bcast:31 into rows 2, 3).
__device__ __forceinline__ int mg_wave_scan_incl_i32(int v) {
  v += __builtin_amdgcn_update_dpp(0, v, 0x111, 0xF, 0xF, true);
  v += __builtin_amdgcn_update_dpp(0, v, 0x112, 0xF, 0xF, true);
  v += __builtin_amdgcn_update_dpp(0, v, 0x114, 0xF, 0xF, true);
  v += __builtin_amdgcn_update_dpp(0, v, 0x118, 0xF, 0xF, true);
  v += __builtin_amdgcn_update_dpp(0, v, 0x142, 0xA, 0xF, false);
  v += __builtin_amdgcn_update_dpp(0, v, 0x143, 0xC, 0xF, false);
  return v;
}
__device__ __forceinline__ int mg_wave_sum_i32(int v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off);
  return v;
}
__device__ __forceinline__ long long mg_wave_sum_i64(long long v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off);
  return v;
}
__device__ __forceinline__ double mg_wave_sum_f64(double v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off);
  return v;
}

// op folded over the 256 threads of a workgroup: xor-shuffles in the wave, then the four waves' partials as
// op(op(s0, s1), op(s2, s3)).  The same value in every thread; called by all (it synchronises, before and after the
// read of the partials).  The sums of mg_track, mg_register, mg_buttons, mg_roi and mg_flatfield are not callers: they
// add their four partials left to right, and another tree would change a float sum in the last bit.
constexpr int MG_FOLD_WAVES = 4;
template <typename V, class Op>
__device__ __forceinline__ V mg_block_fold(V v, Op op) {
  __shared__ V s_part[MG_FOLD_WAVES];
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v = op(v, __shfl_xor(v, off));
  if ((threadIdx.x & 63) == 0) s_part[threadIdx.x >> 6] = v;
  __syncthreads();
  static_assert(MG_FOLD_WAVES == 4, "the fold below is written out for four waves");
  const V r = op(op(s_part[0], s_part[1]), op(s_part[2], s_part[3]));
  __syncthreads();
  return r;
}

// Exclusive prefix sum over the threads of a block (blockDim.x <= 1024, multiple of 64).
// Returns this thread's exclusive prefix; *total receives the block sum in every thread.
__device__ __forceinline__ int mg_block_exscan(int v, int* total) {
  __shared__ int s_wave[16];
  __shared__ int s_total;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, nw = blockDim.x >> 6;
  int incl = v;
#pragma unroll
  for (int off = 1; off < 64; off <<= 1) {
    const int t = __shfl_up(incl, off);
    if (lane >= off) incl += t;
  }
  if (lane == 63) s_wave[wave] = incl;
  __syncthreads();
  if (wave == 0) {
    const int w = lane < nw ? s_wave[lane] : 0;
    int wi = w;
#pragma unroll
    for (int off = 1; off < 16; off <<= 1) {
      const int t = __shfl_up(wi, off);
      if (lane >= off) wi += t;
    }
    if (lane < nw) s_wave[lane] = wi - w;
    if (lane == nw - 1) s_total = wi;
  }
  __syncthreads();
  const int res = incl - v + s_wave[wave];
  *total = s_total;
  __syncthreads();
  return res;
}

// float32 gradient angle at an edge pixel: Scharr on the blurred image (BORDER_REFLECT_101),
// arctan2(dy, dx) evaluated in float64 and rounded once (utils.py:118-119, 170).
struct __attribute__((packed)) MgUnaligned32 {
  uint32_t v;
};
struct __attribute__((packed)) MgUnaligned64 {
  uint64_t v;
};
__device__ __forceinline__ float mg_edge_angle(const uint8_t* __restrict__ pb, int h, int w, int y, int x) {
  if (y >= 1 && y < h - 1 && x >= 1 && x < w - 2) {
    // interior: one (unaligned) 4-byte load per row covers columns x - 1 .. x + 2
    const uint32_t r0 = reinterpret_cast<const MgUnaligned32*>(pb + (int64_t)(y - 1) * w + x - 1)->v;
    const uint32_t r1 = reinterpret_cast<const MgUnaligned32*>(pb + (int64_t)y * w + x - 1)->v;
    const uint32_t r2 = reinterpret_cast<const MgUnaligned32*>(pb + (int64_t)(y + 1) * w + x - 1)->v;
    const int a = r0 & 0xFF, b = (r0 >> 8) & 0xFF, c = (r0 >> 16) & 0xFF;
    const int d = r1 & 0xFF, f = (r1 >> 16) & 0xFF;
    const int g = r2 & 0xFF, hh = (r2 >> 8) & 0xFF, ii = (r2 >> 16) & 0xFF;
    const int dx = 3 * (c - a) + 10 * (f - d) + 3 * (ii - g);
    const int dy = 3 * (g - a) + 10 * (hh - b) + 3 * (ii - c);
    return (float)atan2((double)dy, (double)dx);
  }
  const int ym = mg_reflect101(y - 1, h), yp = mg_reflect101(y + 1, h);
  const int xm = mg_reflect101(x - 1, w), xp = mg_reflect101(x + 1, w);
  const int a = pb[(int64_t)ym * w + xm], b = pb[(int64_t)ym * w + x], c = pb[(int64_t)ym * w + xp];
  const int d = pb[(int64_t)y * w + xm], f = pb[(int64_t)y * w + xp];
  const int g = pb[(int64_t)yp * w + xm], hh = pb[(int64_t)yp * w + x], ii = pb[(int64_t)yp * w + xp];
  const int dx = 3 * (c - a) + 10 * (f - d) + 3 * (ii - g);
  const int dy = 3 * (g - a) + 10 * (hh - b) + 3 * (ii - c);
  return (float)atan2((double)dy, (double)dx);
}

// ---- the scoring tail shared by k_score_tiles (mg_circles.hip) and k_prefilter / k_exact (mg_score.hip) ----
// One term of mean_grad (utils.py:225-251): |angle - expected| folded to [0, pi], then 4 |d - pi/2| / pi - 1.
// x / pi is correctly rounded without the division (Markstein: y = RN(1/pi), q0 = RN(x y), r = x - q0 pi exactly by
// FMA, q = RN(q0 + r y) == RN(x / pi) because pi's significand is not all ones; verified against x / pi on 1e9
// operands of exactly this form).
__device__ __forceinline__ double mg_alignment_term(float angle, double expected) {
  const double PI = 3.141592653589793, INV_PI = 1.0 / 3.141592653589793;
  double d = fabs((double)angle - expected);
  if (d > PI) d = d - PI;
  const double x4 = 4.0 * fabs(d - PI / 2.0);
  const double q0 = x4 * INV_PI;
  return fma(fma(-q0, PI, x4), INV_PI, q0) - 1.0;
}
// What the sum of a perimeter of `len` points has to reach: a circle passes with sum / len >= min_roundness in float32;
// the 1e-3 margin is far above any rounding of the real sum.
__device__ __forceinline__ double mg_score_floor(float min_roundness, int len) {
  return (double)min_roundness * (double)len - 1e-3;
}
// Circle i of the plane's list passed the threshold: onto the alive list, its centre into the plane's maxima (the
// extent of the claim grid).  WRITE: (row, col, r) is not in `circles` yet (keyed lists hold keys until here).
template <bool WRITE>
__device__ __forceinline__ void mg_emit_alive(int32_t* __restrict__ d_num_alive, int32_t* __restrict__ d_alive,
                                              int32_t* __restrict__ d_max_rc, int plane, int64_t circle_cap,
                                              int32_t* __restrict__ circles, int64_t i, int row, int col, int rad) {
  const int k = atomicAdd(&d_num_alive[plane], 1);
  d_alive[(int64_t)plane * circle_cap + k] = (int32_t)i;
  if (WRITE) circles[3 * i] = row, circles[3 * i + 1] = col, circles[3 * i + 2] = rad;
  atomicMax(&d_max_rc[2 * plane], row);
  atomicMax(&d_max_rc[2 * plane + 1], col);
}
