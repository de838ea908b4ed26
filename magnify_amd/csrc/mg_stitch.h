// What the stitch passes share (mg_flatfield.hip: crop / concat; mg_blend.hip: the same with the seams blended;
// mg_register.hip: the stitch of shifted tiles; mg_shading.hip: the shading apply): the chunk of N pixels a lane
// handles and its 16-byte accesses, the source record, the selection of planes, a plane's group maxima, the chunk's
// addresses and dark / flat operands, the per-plane min / max accumulator, the store tail, the launch grid and the
// prologue of the entry points.  The generic kernel built from them is in mg_stitch_kernel.h.
#pragma once
#include <algorithm>

#include "mg_common.h"
#include "mg_flatcorr.h"

namespace {

template <typename T>
struct VecOf;
template <>
struct VecOf<uint8_t> {
  static constexpr int N = 16;
};
template <>
struct VecOf<uint16_t> {
  static constexpr int N = 8;
};
template <>
struct VecOf<float> {
  static constexpr int N = 4;
};
template <>
struct VecOf<double> {
  static constexpr int N = 2;
};

__host__ __device__ __forceinline__ bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

// Load N consecutive elements; one 16-byte load when the address is aligned.
template <typename T, int N>
__device__ __forceinline__ void load_vec(const T* p, T (&v)[N]) {
  if (aligned16(p)) {
    const uint4 raw = *reinterpret_cast<const uint4*>(p);
    __builtin_memcpy(v, &raw, 16);
  } else {
#pragma unroll
    for (int j = 0; j < N; ++j) v[j] = p[j];
  }
}
template <typename T, int N>
__device__ __forceinline__ void store_vec(T* p, const T (&v)[N]) {
  if (aligned16(p)) {
    uint4 raw;
    __builtin_memcpy(&raw, v, 16);
    *reinterpret_cast<uint4*>(p) = raw;
  } else {
#pragma unroll
    for (int j = 0; j < N; ++j) p[j] = v[j];
  }
}
// The store of a chunk of which `cnt` pixels lie inside the image: one vector, or the pixels one by one.
template <typename T, int N>
__device__ __forceinline__ void store_chunk(T* dst, const T (&o)[N], int cnt) {
  if (cnt == N) {
    store_vec<T, N>(dst, o);
  } else {
    for (int j = 0; j < cnt; ++j) dst[j] = o[j];
  }
}

// N consecutive float32 values from a 16-byte aligned address.
template <int N>
__device__ __forceinline__ void load_f32(const float* __restrict__ p, float (&out)[N]) {
#pragma unroll
  for (int q = 0; q < N / 4; ++q) {
    const float4 f = reinterpret_cast<const float4*>(p)[q];
    out[4 * q] = f.x, out[4 * q + 1] = f.y, out[4 * q + 2] = f.z, out[4 * q + 3] = f.w;
  }
}

// N consecutive dark/flat operands as float64 (image of float32/float64, or the scalar).
template <int N>
__device__ __forceinline__ void load_field(const void* __restrict__ img, int dt, int64_t p, double scalar,
                                           double (&out)[N]) {
  if (!img) {
#pragma unroll
    for (int j = 0; j < N; ++j) out[j] = scalar;
  } else if (dt == MG_F32) {
    const float* f = (const float*)img + p;
    if ((N % 4) == 0 && aligned16(f)) {
#pragma unroll
      for (int q = 0; q < N / 4; ++q) {
        const float4 v = reinterpret_cast<const float4*>(f)[q];
        out[4 * q] = v.x;
        out[4 * q + 1] = v.y;
        out[4 * q + 2] = v.z;
        out[4 * q + 3] = v.w;
      }
    } else {
#pragma unroll
      for (int j = 0; j < N; ++j) out[j] = f[j];
    }
  } else {
    const double* d = (const double*)img + p;
#pragma unroll
    for (int j = 0; j < N; ++j) out[j] = d[j];
  }
}

// ---- the source of a pass -----------------------------------------------------------------------------------------

enum { BL_COPY, BL_FLAT, BL_SHADE };  // the value of a tile's pixel: raw, flat-field corrected, shading corrected

// The operands of the pass (those of mg_flatfield_apply_stitch; BL_SHADE: d_dark / d_flat are the float32 fields,
// one per group of planes_per_group planes).
template <typename T>
struct StitchSrc {
  const T* tiles;
  int n_tr, n_tc, ty, tx, planes_per_group;
  double dark;
  const void* d_dark;
  int dark_dt;
  double flat;
  const void* d_flat;
  int flat_dt;
  const double* d_max2;
};

// Selected planes of every group (mg_flatfield_apply_stitch_planes): bit c of `mask` selects plane c of each group of
// planes_per_group planes; the s-th selected plane of the stack is plane (s / n_sel) * planes_per_group + the
// (s % n_sel)-th set bit.  A workgroup takes PLANES_PER_BLOCK consecutive SELECTED planes; without a selection
// (SUBSET false) plane s is plane s.
struct PlaneSel {
  uint32_t mask;
  int n_sel;
};
template <bool SUBSET>
__device__ __forceinline__ int sel_plane(int s, int planes_per_group, PlaneSel sel) {
  if (!SUBSET) return s;
  const int g = s / sel.n_sel;
  uint32_t m = sel.mask;
  for (int k = s - g * sel.n_sel; k > 0; --k) m &= m - 1u;  // without its k lowest set bits
  return g * planes_per_group + __builtin_ctz(m);
}
// plane0 of mg_block_minmax for a selection: `base + b` is the plane the workgroup's b-th running pair belongs to
struct SelBase {
  int s0, planes_per_group;
  PlaneSel sel;
  __device__ __forceinline__ int operator+(int b) const { return sel_plane<true>(s0 + b, planes_per_group, sel); }
};

// The maxima of a plane's group (pass 1), their quotient and whether the correction's fast path holds for them; the
// neutral values where nothing is corrected.
struct GroupMax {
  double m1 = 0.0, m2 = 1.0, kk = 1.0;
  bool fast_ok = false;
};
__device__ __forceinline__ GroupMax group_maxima(const double* __restrict__ d_max2, int plane, int planes_per_group) {
  GroupMax g;
  const int group = plane / planes_per_group;
  g.m1 = d_max2[2 * group];
  g.m2 = d_max2[2 * group + 1];
  g.fast_ok = group_quotient(g.m1, g.m2, g.kk);
  return g;
}

// ---- the chunk of a lane ------------------------------------------------------------------------------------------

// The N output pixels from column ox0 on: tile column and x inside that tile of the first one, whether all N lie in
// that tile (and inside the image), how many lie inside the image.
struct StitchChunk {
  int ox0, tc0, x0, cnt;
  bool one_tile;
};
template <int N>
__device__ __forceinline__ StitchChunk stitch_chunk(int ox0, int hx, int clip, int w_out) {
  StitchChunk c;
  c.ox0 = ox0;
  c.tc0 = ox0 / hx;
  c.x0 = ox0 - c.tc0 * hx + clip;
  c.one_tile = (ox0 + N <= w_out) && (c.x0 - clip + N <= hx);
  c.cnt = c.one_tile ? N : min(N, w_out - ox0);
  return c;
}
// The chunk's pixels in row y of tile row tr: pixel index inside the tile, element offset of the tile in a plane (a
// pixel past the image repeats the last one inside).
template <int N>
__device__ __forceinline__ void chunk_row(const StitchChunk& c, int hx, int clip, int n_tc, int tx, int64_t tile_elems,
                                          int tr, int y, int64_t (&pix)[N], int64_t (&toff)[N]) {
#pragma unroll
  for (int j = 0; j < N; ++j) {
    const int ox = c.ox0 + (c.one_tile ? j : min(j, c.cnt - 1));
    const int tc = c.one_tile ? c.tc0 : ox / hx;
    const int xx = c.one_tile ? c.x0 + j : ox - tc * hx + clip;
    pix[j] = (int64_t)y * tx + xx;
    toff[j] = ((int64_t)tr * n_tc + tc) * tile_elems;
  }
}
// The chunk's pixels of one plane, and one of its operands (dark or flat) as float64: one vector where the chunk
// lies in one tile, pixel by pixel otherwise.
template <typename T, int N>
__device__ __forceinline__ void load_chunk(const T* __restrict__ plane, bool one_tile, const int64_t (&pix)[N],
                                           const int64_t (&toff)[N], T (&x)[N]) {
  if (one_tile) {
    load_vec<T, N>(plane + toff[0] + pix[0], x);
  } else {
#pragma unroll
    for (int j = 0; j < N; ++j) x[j] = plane[toff[j] + pix[j]];
  }
}
template <int N>
__device__ __forceinline__ void load_chunk_field(const void* __restrict__ img, int dt, double scalar, bool one_tile,
                                                 const int64_t (&pix)[N], double (&out)[N]) {
  if (one_tile) {
    load_field<N>(img, dt, pix[0], scalar, out);
  } else {
#pragma unroll
    for (int j = 0; j < N; ++j) out[j] = img ? mg_load_f64(img, dt, pix[j]) : scalar;
  }
}

// ---- per-plane min / max ------------------------------------------------------------------------------------------

// The running min / max of what a lane wrote of PB planes: integer pixels in uint32 registers (identity min > max),
// floating ones in float64 with NaN propagating as in np.min / np.max (identity +inf, -inf).
template <typename T, int PB>
struct PlaneMinMax {
  static constexpr bool kInt = IsIntegral<T>::value;
  using V = std::conditional_t<kInt, uint32_t, double>;
  V lo[PB], hi[PB];
  static __device__ __forceinline__ V top() {
    if constexpr (kInt) return 0xFFFFFFFFu;
    else return INFINITY;
  }
  static __device__ __forceinline__ V bottom() {
    if constexpr (kInt) return 0u;
    else return -INFINITY;
  }
  static __device__ __forceinline__ void fold(V& l, V& h, V vl, V vh) {
    if constexpr (kInt) {
      l = min(l, vl);
      h = max(h, vh);
    } else {
      l = mg_nanmin(l, vl);
      h = mg_nanmax(h, vh);
    }
  }
  __device__ __forceinline__ PlaneMinMax() {
#pragma unroll
    for (int b = 0; b < PB; ++b) lo[b] = top(), hi[b] = bottom();
  }
  // b: a constant once the caller's loop over the planes is unrolled (the arrays stay in registers)
  __device__ __forceinline__ void add(int b, T v) { fold(lo[b], hi[b], (V)v, (V)v); }
  template <int N>
  __device__ __forceinline__ void add(int b, const T (&o)[N], int cnt = N) {
#pragma unroll
    for (int j = 0; j < N; ++j)
      if (j < cnt) add(b, o[j]);
  }
  // b: a run-time index.  The chunk's own min / max first, then into plane b's slot with selects (indexing the
  // register arrays with a loop variable would move them to scratch memory)
  template <int N>
  __device__ __forceinline__ void add_select(int b, const T (&o)[N], int cnt) {
    V l = top(), h = bottom();
#pragma unroll
    for (int j = 0; j < N; ++j)
      if (j < cnt) fold(l, h, (V)o[j], (V)o[j]);
#pragma unroll
    for (int bb = 0; bb < PB; ++bb)
      if (bb == b) fold(lo[bb], hi[bb], l, h);
  }
  // the tail of the kernel (mg_block_minmax: called by all threads); base: the first plane, or a SelBase
  template <class I>
  __device__ __forceinline__ void flush(int np, double* __restrict__ d_minmax, I base) {
    if constexpr (kInt) mg_block_minmax_u32<PB>(lo, hi, np, d_minmax, base);
    else mg_block_minmax_f64<PB>(lo, hi, np, d_minmax, base);
  }
};

// ---- launch ---------------------------------------------------------------------------------------------------------

constexpr int ROWS_PER_BLOCK = 32;  // rows of a workgroup at large batches; fewer when the grid would not fill the chip
constexpr int PLANES_PER_BLOCK = 8;

// The grid of a stitch pass (256 lanes x N pixels wide, `rows` output rows per row group, PLANES_PER_BLOCK planes deep)
// and its rows per row group.
template <int N>
inline dim3 stitch_grid(int h_out, int w_out, int64_t n_planes, int& rows) {
  // rows per workgroup: 32 when that still gives ~8 workgroups per CU, down to 2 for a single assay
  rows = ROWS_PER_BLOCK;
  const int64_t cols_planes = (int64_t)((w_out + 256 * N - 1) / (256 * N)) * ((n_planes + PLANES_PER_BLOCK - 1) / PLANES_PER_BLOCK);
  while (rows > 2 && cols_planes * ((h_out + rows - 1) / rows) < MG_STITCH_WALK_FILL) rows /= 2;
  // ... and at most ~1024 workgroups per plane group walk them (each ends with min/max atomics on the plane's one
  // cache line: 2048 workgroups finishing together took 100 us over them)
  int y_blocks = (h_out + rows - 1) / rows;
  if (rows < ROWS_PER_BLOCK) y_blocks = (int)std::min<int64_t>(y_blocks, std::max<int64_t>(1, MG_STITCH_WALK_PER_GROUP / std::max<int64_t>(1, cols_planes)));
  return dim3((w_out + 256 * N - 1) / (256 * N), y_blocks, (unsigned)((n_planes + PLANES_PER_BLOCK - 1) / PLANES_PER_BLOCK));
}

// f(std::true_type / std::false_type) for a run-time flag: a kernel's compile-time switches from the launcher's flags
template <class F>
inline int with_flag(bool v, F&& f) {
  return v ? f(std::true_type{}) : f(std::false_type{});
}

// ---- entry points ---------------------------------------------------------------------------------------------------

inline bool field_dtype_ok(const void* p, int dt) { return p == nullptr || dt == MG_F32 || dt == MG_F64; }

// What mg_flatfield_apply_stitch, _blend and _shift do after their own shape check: the other argument checks, the
// identity shortcut, then launch(StitchSrc<T>, BL_FLAT or BL_COPY as a std::integral_constant) for the pixel type.
template <class F>
inline int flatfield_stitch_entry(const void* d_tiles, int dtype, int64_t n_planes, int n_tr, int n_tc, int ty, int tx,
                                  int apply_flatfield, int planes_per_group, double dark, const void* d_dark,
                                  int dark_dtype, double flat, const void* d_flat, int flat_dtype, const double* d_max2,
                                  const void* d_image, F&& launch) {
  if (!d_tiles || !d_image || n_planes < 0) return MG_EINVAL;
  // Integer pixels, dark 0 and flat 1 (the reference's defaults, preprocess.py:62): ((t / 1) * M1) / M2 with
  // M2 = M1 / 1 is t itself -- the product of two integers below 2^16 is exact in float64 and so is its quotient by
  // one of them; an all-zero group gives 0 either way (NaN -> 0).  Every pixel would otherwise take the exact
  // two-division path (its fast result is an integer), 2.3x the time of a copy.
  if (apply_flatfield && mg_flatfield_is_identity(dtype, dark, d_dark, flat, d_flat)) apply_flatfield = 0;
  if (apply_flatfield && (!d_max2 || planes_per_group <= 0)) return MG_EINVAL;
  if (!field_dtype_ok(d_dark, dark_dtype) || !field_dtype_ok(d_flat, flat_dtype)) return MG_EINVAL;
  return mg_dispatch_pixel(dtype, [&](auto t) {
    using T = decltype(t);
    const StitchSrc<T> src{(const T*)d_tiles, n_tr, n_tc, ty, tx, planes_per_group > 0 ? planes_per_group : 1,
                           dark, d_dark, dark_dtype, flat, d_flat, flat_dtype, d_max2};
    return apply_flatfield ? launch(src, std::integral_constant<int, BL_FLAT>{})
                           : launch(src, std::integral_constant<int, BL_COPY>{});
  });
}

// The same for mg_shading_apply_stitch_blend and _shift: `check()` (what the entry has to look at before an empty stack
// is answered with MG_OK; non-zero: returned), then launch(StitchSrc<T>, n_planes).
template <class C, class F>
inline int shading_stitch_entry(const void* d_tiles, int dtype, int n_fields, int64_t planes_per_field, int n_tr, int n_tc,
                                int ty, int tx, const float* d_flat, const float* d_dark, const void* d_image, C&& check,
                                F&& launch) {
  if (!d_tiles || !d_image || !d_flat || !d_dark || n_fields < 1 || planes_per_field < 0 || planes_per_field > 0x7FFFFFF0)
    return MG_EINVAL;
  if (const int rc = check()) return rc;
  if (planes_per_field == 0) return MG_OK;
  return mg_dispatch_pixel(dtype, [&](auto t) {
    using T = decltype(t);
    const StitchSrc<T> src{(const T*)d_tiles, n_tr, n_tc, ty, tx, (int)planes_per_field,
                           0.0, d_dark, MG_F32, 1.0, d_flat, MG_F32, nullptr};
    return launch(src, (int64_t)n_fields * planes_per_field);
  });
}

}  // namespace
