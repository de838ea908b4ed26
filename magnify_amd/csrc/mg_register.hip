// Tile registration ("stitch: registration by seam cross-correlation"): the sums behind the zero-mean
// normalised cross-correlation of the two overlap strips of every seam, for every displacement of a (2m + 1)^2 window
// (mg_seam_sums), and the stitch of tiles moved by one integer shift each (mg_*_apply_stitch_shift).
//
// Seam sums.  A patch of tile B (the second tile of the seam) is compared with the patch of tile A displaced by
// delta; per (plane, seam): fixed = [n, sum B, sum B^2] and per delta [sum A, sum A^2, sum A B], exact in 64-bit
// integers for integer pixels, float64 for float pixels.
//   * k_seam_partial: a workgroup takes one (plane, seam, strip of SEAM_STRIP positions along the patch's long side)
//     and walks the strip in square tiles: the B tile and the A tile with its halo of m are staged in LDS, then every
//     work item (delta, k) -- K of them per displacement, k = rows k, k + K, ... of the tile -- runs over its pixels.
//     Consecutive lanes own the K row groups of one displacement, then the next delta_x: the B read is one address per
//     row group (a broadcast inside it), the A reads are consecutive for consecutive delta_x.  The row strides of both
//     LDS tiles are padded to 32 / K banks past a multiple of 32, so the K rows a 32-lane group reads at once fall on
//     disjoint banks.  The K accumulators of a displacement are added in lane order (shuffles), the strip's sums go
//     to the scratch.
//   * k_seam_reduce: adds the strips in strip order and makes `fixed` with a fixed lane assignment.  No atomics
//     anywhere: the result is the same bits run to run, for float pixels too.
//
// Roofline: ALU / LDS, not HBM.  3 n (2m + 1)^2 multiply-adds per seam with 64-bit accumulators, two LDS reads per
// three of them: the 8 x 8 chip of 1024^2 tiles at overlap 102, m = 8 has 112 seams of n = 1008 x 86 pixels --
// 8.4e9 multiply-adds -- against 40 MB of pixels read once from HBM (8 us at 5 TB/s).
//
// Shifted stitch.  tile'[y, x] = value[clamp(y - ey, 0, ty - 1), clamp(x - ex, 0, tx - 1)] for the tile's shift
// (ey, ex), `value` what the plain pass writes (tile_value of mg_blendop.h); then the plain crop / concat or, with
// blend, the linear mix of mg_blend.hip, from the same functions.  It moves the bytes of the plain pass, but is not at
// that pass's HBM roofline: the reads are per pixel (a shifted chunk is no longer 16-byte aligned and may cross the
// clamped border), the table entry and the correction's operands are fetched per pixel.
#include <math.h>

#include <vector>

#include "mg_blendop.h"
#include "mg_common.h"
#include "mg_stitch.h"

namespace {

// ---- seam sums ---------------------------------------------------------------------------------------------------

constexpr int SEAM_STRIP = 128;             // positions along the patch's long side per workgroup
constexpr int SEAM_LDS_BUDGET = 48 * 1024;  // bytes of LDS a workgroup may stage
constexpr int SEAM_MAX_SHIFT = 32;          // largest m whose smallest tile (8 x 8 + halo) still fits the budget in float64

// LDS element and accumulator of a pixel type
template <typename T>
struct SeamTypes {
  using L = uint16_t;
  using Acc = unsigned long long;
  using Out = long long;
};
template <>
struct SeamTypes<float> {
  using L = float;
  using Acc = double;
  using Out = double;
};
template <>
struct SeamTypes<double> {
  using L = double;
  using Acc = double;
  using Out = double;
};

__device__ __forceinline__ void seam_accumulate(unsigned long long& sa, unsigned long long& saa, unsigned long long& sab,
                                                uint16_t a, uint16_t b) {
  const uint32_t ai = a, bi = b;
  sa += ai;
  saa += (unsigned long long)ai * ai;
  sab += (unsigned long long)ai * bi;
}
template <typename L>
__device__ __forceinline__ void seam_accumulate(double& sa, double& saa, double& sab, L a, L b) {
  const double ad = (double)a, bd = (double)b;
  sa += ad;
  saa = fma(ad, ad, saa);
  sab = fma(ad, bd, sab);
}

struct SeamGeom {
  int n_tr, n_tc, ty, tx, v, m;
  int n_horizontal;  // seams (r, c) | (r, c + 1); the vertical ones follow
  int tile, aw, bw, K;  // LDS tile side, row strides of the A and B tiles (elements), row groups per displacement
  int n_strips;
};

// The seam's tiles and its patch in B: rows [y0, y1), columns [x0, x1); A is read at + (oy, ox) + delta.
struct SeamPatch {
  int tile_a, tile_b, y0, y1, x0, x1, oy, ox;
  bool along_y;  // the long side
};
__device__ __forceinline__ SeamPatch seam_patch(const SeamGeom& g, int seam) {
  SeamPatch p;
  if (seam < g.n_horizontal) {
    const int r = seam / (g.n_tc - 1), c = seam - r * (g.n_tc - 1);
    p.tile_a = r * g.n_tc + c, p.tile_b = p.tile_a + 1;
    p.y0 = g.m, p.y1 = g.ty - g.m, p.x0 = g.m, p.x1 = g.v - g.m, p.oy = 0, p.ox = g.tx - g.v, p.along_y = true;
  } else {
    const int s = seam - g.n_horizontal;
    p.tile_a = s, p.tile_b = s + g.n_tc;
    p.y0 = g.m, p.y1 = g.v - g.m, p.x0 = g.m, p.x1 = g.tx - g.m, p.oy = g.ty - g.v, p.ox = 0, p.along_y = false;
  }
  return p;
}

// grid (strip, seam, plane); partial (plane, seam, strip, delta, 3)
template <typename T>
__global__ __launch_bounds__(256) void k_seam_partial(const T* __restrict__ planes, SeamGeom g,
                                                      typename SeamTypes<T>::Out* __restrict__ partial) {
  using L = typename SeamTypes<T>::L;
  using Acc = typename SeamTypes<T>::Acc;
  extern __shared__ __attribute__((aligned(16))) unsigned char seam_lds[];
  L* sA = reinterpret_cast<L*>(seam_lds);
  L* sB = sA + (size_t)(g.tile + 2 * g.m) * g.aw;
  const int strip = blockIdx.x, seam = blockIdx.y, plane = blockIdx.z, n_seams = gridDim.y;
  const int m = g.m, W = 2 * m + 1, D = W * W, K = g.K, tile = g.tile;
  SeamPatch p = seam_patch(g, seam);
  if (p.along_y) {
    p.y0 = min(p.y0 + strip * SEAM_STRIP, p.y1);
    p.y1 = min(p.y0 + SEAM_STRIP, p.y1);
  } else {
    p.x0 = min(p.x0 + strip * SEAM_STRIP, p.x1);
    p.x1 = min(p.x0 + SEAM_STRIP, p.x1);
  }
  const int64_t tile_elems = (int64_t)g.ty * g.tx, plane_base = (int64_t)plane * g.n_tr * g.n_tc * tile_elems;
  const T* A = planes + plane_base + (int64_t)p.tile_a * tile_elems;
  const T* B = planes + plane_base + (int64_t)p.tile_b * tile_elems;
  typename SeamTypes<T>::Out* out = partial + (((int64_t)plane * n_seams + seam) * g.n_strips + strip) * D * 3;
  const int n_items = D * K;
  for (int base = 0; base < n_items; base += 256) {  // (uniform: every lane walks every pass, idle or not)
    const int item = base + threadIdx.x;
    const bool live = item < n_items;
    const int d = live ? item / K : 0, k = item - (item / K) * K;
    const int dy = d / W, dx = d - dy * W;  // delta + m
    Acc sa = 0, saa = 0, sab = 0;
    for (int ty0 = p.y0; ty0 < p.y1; ty0 += tile) {
      const int th = min(tile, p.y1 - ty0);
      for (int tx0 = p.x0; tx0 < p.x1; tx0 += tile) {
        const int tw = min(tile, p.x1 - tx0);
        __syncthreads();  // the tile before has been read
        const int a_rows = th + 2 * m, a_cols = tw + 2 * m;
        for (int e = threadIdx.x; e < a_rows * a_cols; e += 256) {
          const int i = e / a_cols, j = e - i * a_cols;
          sA[i * g.aw + j] = (L)A[(int64_t)(ty0 + p.oy - m + i) * g.tx + (tx0 + p.ox - m + j)];
        }
        for (int e = threadIdx.x; e < th * tw; e += 256) {
          const int i = e / tw, j = e - i * tw;
          sB[i * g.bw + j] = (L)B[(int64_t)(ty0 + i) * g.tx + (tx0 + j)];
        }
        __syncthreads();
        if (live) {
          for (int i = k; i < th; i += K) {
            const L* rowA = sA + (i + dy) * g.aw + dx;
            const L* rowB = sB + i * g.bw;
#pragma unroll 4
            for (int j = 0; j < tw; ++j) seam_accumulate(sa, saa, sab, rowA[j], rowB[j]);
          }
        }
      }
    }
    // the K row groups of a displacement sit in K consecutive lanes (K divides 64): added in lane order
    Acc ta = sa, taa = saa, tab = sab;
    for (int j = 1; j < K; ++j) {
      ta += __shfl_down(sa, j);
      taa += __shfl_down(saa, j);
      tab += __shfl_down(sab, j);
    }
    if (live && k == 0) {
      out[3 * d] = (typename SeamTypes<T>::Out)ta;
      out[3 * d + 1] = (typename SeamTypes<T>::Out)taa;
      out[3 * d + 2] = (typename SeamTypes<T>::Out)tab;
    }
  }
}

__device__ __forceinline__ long long seam_wave_sum(long long v) { return mg_wave_sum_i64(v); }
__device__ __forceinline__ double seam_wave_sum(double v) { return mg_wave_sum_f64(v); }

// grid (seam, plane): sums[plane, seam, delta, 3] = the strips' partial sums added in strip order; fixed[plane, seam] =
// [n, sum B, sum B^2] with every lane taking the same pixels on every run.
template <typename T>
__global__ __launch_bounds__(256) void k_seam_reduce(const T* __restrict__ planes, SeamGeom g,
                                                     const typename SeamTypes<T>::Out* __restrict__ partial,
                                                     typename SeamTypes<T>::Out* __restrict__ sums,
                                                     typename SeamTypes<T>::Out* __restrict__ fixed) {
  using Out = typename SeamTypes<T>::Out;
  const int seam = blockIdx.x, plane = blockIdx.y, n_seams = gridDim.x;
  const int W = 2 * g.m + 1, n_entries = W * W * 3;
  const int64_t slot = (int64_t)plane * n_seams + seam;
  const Out* part = partial + slot * g.n_strips * n_entries;
  for (int e = threadIdx.x; e < n_entries; e += 256) {
    Out acc = part[e];
    for (int s = 1; s < g.n_strips; ++s) acc += part[(int64_t)s * n_entries + e];
    sums[slot * n_entries + e] = acc;
  }
  const SeamPatch p = seam_patch(g, seam);
  const int64_t tile_elems = (int64_t)g.ty * g.tx;
  const T* B = planes + ((int64_t)plane * g.n_tr * g.n_tc + p.tile_b) * tile_elems;
  const int pw = p.x1 - p.x0, n = (p.y1 - p.y0) * pw;
  Out sb = 0, sbb = 0;
  for (int e = threadIdx.x; e < n; e += 256) {
    const int i = e / pw, j = e - i * pw;
    const T b = B[(int64_t)(p.y0 + i) * g.tx + p.x0 + j];
    if (std::is_integral<T>::value) {
      sb += (Out)b;
      sbb += (Out)((unsigned long long)b * (unsigned long long)b);
    } else {
      sb += (Out)b;
      sbb = (Out)fma((double)b, (double)b, (double)sbb);
    }
  }
  __shared__ Out s_part[2][MG_MINMAX_WAVES];
  sb = seam_wave_sum(sb);
  sbb = seam_wave_sum(sbb);
  if ((threadIdx.x & 63) == 0) s_part[0][threadIdx.x >> 6] = sb, s_part[1][threadIdx.x >> 6] = sbb;
  __syncthreads();
  if (threadIdx.x == 0) {
    fixed[3 * slot] = (Out)n;
    fixed[3 * slot + 1] = ((s_part[0][0] + s_part[0][1]) + s_part[0][2]) + s_part[0][3];
    fixed[3 * slot + 2] = ((s_part[1][0] + s_part[1][1]) + s_part[1][2]) + s_part[1][3];
  }
}

inline int64_t seam_count(int n_tr, int n_tc) { return (int64_t)n_tr * (n_tc - 1) + (int64_t)(n_tr - 1) * n_tc; }
inline bool seam_args_ok(int64_t n_planes, int n_tr, int n_tc, int ty, int tx, int v, int m) {
  // 4 m <= v: the patch keeps at least half the overlap; v <= tile: the strips lie inside the tiles
  return n_planes >= 0 && n_planes <= 65535 && n_tr > 0 && n_tc > 0 && ty > 0 && tx > 0 && m >= 1 && m <= SEAM_MAX_SHIFT &&
         4 * (int64_t)m <= v && v <= ty && v <= tx && seam_count(n_tr, n_tc) <= 65535;
}

// The LDS layout for an element of `elem` bytes: the largest tile of 32, 16, 8 whose two staged tiles fit the budget.
inline bool seam_layout(int elem, SeamGeom& g, size_t& lds_bytes) {
  const int W = 2 * g.m + 1, D = W * W;
  // row groups per displacement: of 1, 2, 4, 8 the one that leaves the fewest idle lanes in the last pass of 256
  double best = 1e30;
  for (int K = 1; K <= 8; K *= 2) {
    const int items = D * K;
    const double waste = (double)((items + 255) / 256 * 256) / items;
    if (waste < best - 1e-9) best = waste, g.K = K;
  }
  // row strides: the smallest that are 32 / K banks past a multiple of 32 banks (K = 1: one row at a time, any stride)
  const int unit = elem == 2 ? 64 : 32, pad = (32 / g.K) * (elem == 2 ? 2 : 1);  // elements per 32 banks
  auto stride = [&](int cols) { return g.K == 1 ? cols : cols + ((pad - cols) % unit + unit) % unit; };
  for (int tile = 32; tile >= 8; tile /= 2) {
    g.tile = tile;
    g.aw = stride(tile + 2 * g.m);
    g.bw = stride(tile);
    lds_bytes = ((size_t)(tile + 2 * g.m) * g.aw + (size_t)tile * g.bw) * elem;
    if (lds_bytes <= (size_t)SEAM_LDS_BUDGET) return true;
    if (tile == 8 && g.K != 1) g.K = 1, tile = 64;  // no padded layout fits: once more without row groups
  }
  return false;
}

inline SeamGeom seam_geom(int n_tr, int n_tc, int ty, int tx, int v, int m) {
  SeamGeom g{n_tr, n_tc, ty, tx, v, m, n_tr * (n_tc - 1), 0, 0, 0, 1, 0};
  const int longest = std::max(n_tc > 1 ? ty - 2 * m : 0, n_tr > 1 ? tx - 2 * m : 0);
  g.n_strips = std::max(1, (longest + SEAM_STRIP - 1) / SEAM_STRIP);
  return g;
}

// ---- shifted stitch ----------------------------------------------------------------------------------------------

struct ShiftTable {
  const int32_t* shift;  // (n_tables, n_tr, n_tc, 2): (ey, ex)
  int n_tables, n_time;
};

// What the plain pass writes for pixel (y, x) of tile (tr, tc) moved by its shift: edge replication at the borders.
template <typename T, int MODE>
__device__ __forceinline__ T shifted_value(const StitchSrc<T>& s, const int32_t* __restrict__ table, int plane, int tr,
                                           int tc, int y, int x, const GroupMax& g) {
  const int32_t* e = table + 2 * (tr * s.n_tc + tc);
  const int yy = min(max(y - e[0], 0), s.ty - 1), xx = min(max(x - e[1], 0), s.tx - 1);
  return tile_value<T, MODE>(s, plane, tr, tc, yy, xx, g);
}

// The grid and the chunks of k_stitch (mg_stitch_kernel.h); every pixel of a chunk is fetched on its own.
template <typename T, int MODE, bool BLEND>
__global__ __launch_bounds__(256) void k_shift_stitch(StitchSrc<T> s, ShiftTable st, int n_planes, int v, int hy, int hx,
                                                       T* __restrict__ image, double* __restrict__ d_minmax,
                                                       int rows_per_block) {
  constexpr int N = VecOf<T>::N;
  constexpr int PB = PLANES_PER_BLOCK;
  const int clip = v / 2, rem = v % 2, n_tr = s.n_tr, n_tc = s.n_tc;
  const Axis ay{v, clip, rem, hy, n_tr}, ax{v, clip, rem, hx, n_tc};
  const int plane0 = blockIdx.z * PB;
  const int np = min(PB, n_planes - plane0);
  const int h_out = n_tr * hy, w_out = n_tc * hx;
  const int ox0 = (blockIdx.x * blockDim.x + threadIdx.x) * N;
  PlaneMinMax<T, PB> mm;
  if (ox0 < w_out) {
    const int cnt = min(N, w_out - ox0);
    for (int yg = blockIdx.y; yg * rows_per_block < h_out; yg += gridDim.y) {
      const int row_end = min((yg + 1) * rows_per_block, h_out);
      for (int oy = yg * rows_per_block; oy < row_end; ++oy) {
        const int tr = oy / hy;
        const int y = oy - tr * hy + clip;
        int oth_y = 0, ny = 2 * v;
        if (BLEND) axis_term(ay, tr, y - clip, oth_y, ny);
#pragma unroll 1
        for (int b = 0; b < np; ++b) {
          const int plane = plane0 + b;
          GroupMax g;
          if (MODE == BL_FLAT) g = group_maxima(s.d_max2, plane, s.planes_per_group);
          const int32_t* table = st.shift + (st.n_tables == 1 ? 0 : (int64_t)(plane % st.n_time) * n_tr * n_tc * 2);
          T o[N];
#pragma unroll
          for (int j = 0; j < N; ++j) {
            const int ox = ox0 + min(j, cnt - 1), tc = ox / hx, x = ox - tc * hx + clip;
            T c00 = shifted_value<T, MODE>(s, table, plane, tr, tc, y, x, g);
            if (BLEND) {
              int oth_x, nx;
              axis_term(ax, tc, x - clip, oth_x, nx);
              if (oth_x != 0 || oth_y != 0) {
                const int tr1 = tr + oth_y, y1 = y - oth_y * hy, tc1 = tc + oth_x, x1 = x - oth_x * hx;
                T c01 = (T)0, c10 = (T)0, c11 = (T)0;
                if (oth_x != 0) c01 = shifted_value<T, MODE>(s, table, plane, tr, tc1, y, x1, g);
                if (oth_y != 0) c10 = shifted_value<T, MODE>(s, table, plane, tr1, tc, y1, x, g);
                if (oth_x != 0 && oth_y != 0) c11 = shifted_value<T, MODE>(s, table, plane, tr1, tc1, y1, x1, g);
                c00 = mix_tiles<T>(c00, c01, c10, c11, oth_x != 0, oth_y != 0, nx, ny, v);
              }
            }
            o[j] = c00;
          }
          if (d_minmax) mm.add_select(b, o, cnt);  // (b is a loop variable)
          store_chunk<T, N>(image + ((int64_t)plane * h_out + oy) * w_out + ox0, o, cnt);
        }
      }
    }
  }
  if (d_minmax) mm.flush(np, d_minmax, plane0);
}

template <int MODE, typename T>
int launch_shift(const StitchSrc<T>& src, const ShiftTable& st, int64_t n_planes, int overlap, int blend, void* d_image,
                 double* d_minmax, hipStream_t s) {
  const MgStitchGeom g = mg_stitch_geom(src.ty, src.tx, overlap, src.n_tr, src.n_tc);
  if (n_planes == 0 || g.h_out == 0 || g.w_out == 0) return MG_OK;
  int rows;
  const dim3 grid = stitch_grid<VecOf<T>::N>(g.h_out, g.w_out, n_planes, rows);
  if (grid.y > MG_WALK_MAX_Y || grid.z > MG_WALK_MAX_Y) return MG_EINVAL;
  return with_flag(blend, [&](auto bl) {
    hipLaunchKernelGGL((k_shift_stitch<T, MODE, decltype(bl)::value>), grid, dim3(256), 0, s, src, st, (int)n_planes, overlap,
                       g.hy, g.hx, (T*)d_image, d_minmax, rows);
    MG_CHECK_LAUNCH();
    return (int)MG_OK;
  });
}

inline bool shift_shape_ok(int n_tr, int n_tc, int ty, int tx, int overlap, int blend) {
  // blend: 2 overlap <= tile, as mg_flatfield_apply_stitch_blend; else the plain pass's overlap < tile
  if (!(n_tr > 0 && n_tc > 0 && ty > 0 && tx > 0 && overlap >= 0 && (blend == 0 || blend == 1))) return false;
  const int64_t need = blend ? 2 * (int64_t)overlap : (int64_t)overlap + 1;
  return need <= ty && need <= tx;
}
// The shift tables, read back: every entry within [-clip, clip] (the stream is waited for).
inline int shift_tables_ok(const int32_t* d_shift, int n_tables, int n_time, int64_t n_planes, int n_tr, int n_tc,
                           int overlap, hipStream_t s) {
  if (!d_shift || n_time < 1 || !(n_tables == 1 || n_tables == n_time) || n_planes > 0x7FFFFFF0) return MG_EINVAL;
  std::vector<int32_t> host((size_t)n_tables * n_tr * n_tc * 2);
  if (hipMemcpyAsync(host.data(), d_shift, host.size() * sizeof(int32_t), hipMemcpyDeviceToHost, s) != hipSuccess ||
      hipStreamSynchronize(s) != hipSuccess)
    return MG_ELAUNCH;
  const int clip = overlap / 2;
  for (int32_t e : host)
    if (e < -clip || e > clip) return MG_EINVAL;
  return MG_OK;
}

}  // namespace

extern "C" int64_t mg_seam_sums_scratch_bytes(int64_t n_planes, int n_tile_rows, int n_tile_cols, int ty, int tx,
                                              int overlap, int max_shift) {
  if (!seam_args_ok(n_planes, n_tile_rows, n_tile_cols, ty, tx, overlap, max_shift)) return -1;
  const SeamGeom g = seam_geom(n_tile_rows, n_tile_cols, ty, tx, overlap, max_shift);
  const int64_t W = 2 * max_shift + 1;
  return n_planes * seam_count(n_tile_rows, n_tile_cols) * g.n_strips * W * W * 3 * 8;
}

extern "C" int mg_seam_sums(const void* d_planes, int dtype, int64_t n_planes, int n_tile_rows, int n_tile_cols, int ty,
                            int tx, int overlap, int max_shift, void* d_sums, void* d_fixed, void* d_scratch,
                            int64_t scratch_bytes, void* stream) {
  if (!seam_args_ok(n_planes, n_tile_rows, n_tile_cols, ty, tx, overlap, max_shift)) return MG_EINVAL;
  const int64_t n_seams = seam_count(n_tile_rows, n_tile_cols);
  if (n_planes == 0 || n_seams == 0) return MG_OK;
  if (!d_planes || !d_sums || !d_fixed || !d_scratch ||
      scratch_bytes < mg_seam_sums_scratch_bytes(n_planes, n_tile_rows, n_tile_cols, ty, tx, overlap, max_shift))
    return MG_EINVAL;
  hipStream_t s = mg_stream(stream);
  return mg_dispatch_pixel(dtype, [&](auto t) {
    using T = decltype(t);
    using Out = typename SeamTypes<T>::Out;
    SeamGeom g = seam_geom(n_tile_rows, n_tile_cols, ty, tx, overlap, max_shift);
    size_t lds = 0;
    if (!seam_layout((int)sizeof(typename SeamTypes<T>::L), g, lds)) return (int)MG_EINVAL;
    hipLaunchKernelGGL((k_seam_partial<T>), dim3(g.n_strips, (unsigned)n_seams, (unsigned)n_planes), dim3(256), lds, s,
                       (const T*)d_planes, g, (Out*)d_scratch);
    MG_CHECK_LAUNCH();
    hipLaunchKernelGGL((k_seam_reduce<T>), dim3((unsigned)n_seams, (unsigned)n_planes), dim3(256), 0, s, (const T*)d_planes,
                       g, (const Out*)d_scratch, (Out*)d_sums, (Out*)d_fixed);
    MG_CHECK_LAUNCH();
    return (int)MG_OK;
  });
}

extern "C" int mg_flatfield_apply_stitch_shift(const void* d_tiles, int dtype, int64_t n_planes, int n_tile_rows,
                                               int n_tile_cols, int ty, int tx, int overlap, int apply_flatfield,
                                               int planes_per_group, double dark, const void* d_dark, int dark_dtype,
                                               double flat, const void* d_flat, int flat_dtype, const double* d_max2,
                                               void* d_image, double* d_minmax, const int32_t* d_shift, int n_tables,
                                               int n_time, int blend, void* stream) {
  if (!shift_shape_ok(n_tile_rows, n_tile_cols, ty, tx, overlap, blend)) return MG_EINVAL;
  hipStream_t s = mg_stream(stream);
  const ShiftTable st{d_shift, n_tables, n_time};
  return flatfield_stitch_entry(
      d_tiles, dtype, n_planes, n_tile_rows, n_tile_cols, ty, tx, apply_flatfield, planes_per_group, dark, d_dark, dark_dtype,
      flat, d_flat, flat_dtype, d_max2, d_image, [&](const auto& src, auto mode) {
        // (the tables are read back only for a call whose other arguments are in order)
        if (const int rc = shift_tables_ok(d_shift, n_tables, n_time, n_planes, n_tile_rows, n_tile_cols, overlap, s)) return rc;
        return launch_shift<decltype(mode)::value>(src, st, n_planes, overlap, blend, d_image, d_minmax, s);
      });
}

extern "C" int mg_shading_apply_stitch_shift(const void* d_tiles, int dtype, int n_fields, int64_t planes_per_field,
                                             int n_tile_rows, int n_tile_cols, int ty, int tx, int overlap,
                                             const float* d_flat, const float* d_dark, void* d_image, double* d_minmax,
                                             const int32_t* d_shift, int n_tables, int n_time, int blend, void* stream) {
  if (!shift_shape_ok(n_tile_rows, n_tile_cols, ty, tx, overlap, blend)) return MG_EINVAL;
  hipStream_t s = mg_stream(stream);
  const ShiftTable st{d_shift, n_tables, n_time};
  return shading_stitch_entry(
      d_tiles, dtype, n_fields, planes_per_field, n_tile_rows, n_tile_cols, ty, tx, d_flat, d_dark, d_image,
      [&] {  // (after the argument checks, before an empty stack is answered: the tables, as the flat-field entry)
        return shift_tables_ok(d_shift, n_tables, n_time, (int64_t)n_fields * planes_per_field, n_tile_rows, n_tile_cols,
                               overlap, s);
      },
      [&](const auto& src, int64_t n_planes) {
        return launch_shift<BL_SHADE>(src, st, n_planes, overlap, blend, d_image, d_minmax, s);
      });
}
