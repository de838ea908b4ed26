// A2 flat-field correction (preprocess.py:83-87) fused with A1 stitch (stitch.py:22-39),
// and the per-plane min/max that feeds to_uint8 (utils.py:24-26).
//
// Roofline: HBM.  Algorithmic bytes per pixel (u16): pass 1 reads 2 B, pass 2 reads 2 B and
// writes 2 B -> 6 B/px.  The two global maxima make the second read compulsory.
#include <math.h>

#include "mg_common.h"
#include "mg_flatcorr.h"
#include "mg_stitch.h"
#include "mg_stitch_kernel.h"

namespace {

// 16-byte accesses at addresses the caller knows to be aligned; `nt`: nontemporal (streamed once, not kept in cache)
typedef uint32_t mg_u32x4 __attribute__((ext_vector_type(4)));
template <typename T, int N>
__device__ __forceinline__ void load_vec16(const T* p, T (&v)[N], bool nt) {
  const mg_u32x4* q = reinterpret_cast<const mg_u32x4*>(p);
  const mg_u32x4 raw = nt ? __builtin_nontemporal_load(q) : *q;
  __builtin_memcpy(v, &raw, 16);
}
template <typename T, int N>
__device__ __forceinline__ void store_vec16(T* p, const T (&v)[N], bool nt) {
  mg_u32x4 raw;
  __builtin_memcpy(&raw, v, 16);
  mg_u32x4* q = reinterpret_cast<mg_u32x4*>(p);
  if (nt) __builtin_nontemporal_store(raw, q);
  else *q = raw;
}

__device__ __forceinline__ void block_atomic_max2(double m1, double m2, double* out) {
  __shared__ double s1[16], s2[16];
  m1 = mg_wave_nanmax(m1);
  m2 = mg_wave_nanmax(m2);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  if (lane == 0) {
    s1[wave] = m1;
    s2[wave] = m2;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    const int nw = (blockDim.x + 63) >> 6;
    for (int i = 1; i < nw; ++i) {
      m1 = mg_nanmax(m1, s1[i]);
      m2 = mg_nanmax(m2, s2[i]);
    }
    mg_atomic_nanmax(out, m1);
    mg_atomic_nanmax(out + 1, m2);
  }
}

// ---- pass 1: global maxima -----------------------------------------------------------
// Division-free filter for M2 = max(t / flat): the float32 reciprocal gives the quotient to
// ~2e-7; only pixels whose approximate quotient is within 1e-6 of the running maximum pay for
// the exact float64 division, so the result is the exact maximum of the exact quotients.
__device__ __forceinline__ void max_step(double t, double fl, bool fast_m2, double& m1, double& m2) {
  m1 = mg_nanmax(m1, t);
  if (fast_m2) return;
  if (flat_in_range(fl) && t == t) {
    if (t == 0.0) {
      m2 = mg_nanmax(m2, 0.0);
      return;
    }
    const double qa = t * (double)__builtin_amdgcn_rcpf((float)fl);
    if (m2 == m2 && qa < m2 * (1.0 - 1e-6)) return;  // provably below the running maximum
  }
  m2 = mg_nanmax(m2, t / fl);
}

// Thread = one chunk of N pixels of the tile grid; it walks over the tiles of its group, so the
// dark/flat operands are loaded once per chunk and reused for every tile (channel) of the group.
template <typename T>
__global__ __launch_bounds__(256) void k_flatfield_max(const T* __restrict__ tiles, int64_t tiles_per_group,
                                                        int64_t tile_elems, double dark,
                                                        const void* __restrict__ d_dark, int dark_dt, double flat,
                                                        const void* __restrict__ d_flat, int flat_dt,
                                                        double* __restrict__ out) {
  constexpr int N = VecOf<T>::N;
  const int group = blockIdx.y;
  tiles += (int64_t)group * tiles_per_group * tile_elems;
  out += 2 * group;
  const bool fast_m2 = (d_flat == nullptr) && (flat > 0.0);  // x / flat is monotone: M2 = M1 / flat
  double m1 = -INFINITY, m2 = -INFINITY;
  const int64_t nvec = tile_elems / N;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t v = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; v < nvec; v += stride) {
    double dk[N], fl[N];
    load_field<N>(d_dark, dark_dt, v * N, dark, dk);
    load_field<N>(d_flat, flat_dt, v * N, flat, fl);
    for (int64_t g = 0; g < tiles_per_group; ++g) {
      T x[N];
      load_vec<T, N>(tiles + g * tile_elems + v * N, x);
#pragma unroll
      for (int j = 0; j < N; ++j) {
        double t = (double)x[j] - dk[j];
        t = t < 0.0 ? 0.0 : t;
        max_step(t, fl[j], fast_m2, m1, m2);
      }
    }
  }
  // tail pixels of every tile (tile_elems not a multiple of N)
  for (int64_t p = nvec * N + (int64_t)blockIdx.x * blockDim.x + threadIdx.x; p < tile_elems; p += stride) {
    const double dk = d_dark ? mg_load_f64(d_dark, dark_dt, p) : dark;
    const double fl = d_flat ? mg_load_f64(d_flat, flat_dt, p) : flat;
    for (int64_t g = 0; g < tiles_per_group; ++g) {
      double t = (double)tiles[g * tile_elems + p] - dk;
      t = t < 0.0 ? 0.0 : t;
      max_step(t, fl, fast_m2, m1, m2);
    }
  }
  if (fast_m2) m2 = (m1 == -INFINITY) ? m1 : m1 / flat;
  block_atomic_max2(m1, m2, out);
}

// Pass 1 for integer pixels with a scalar dark AND a scalar flat > 0: t = max(x - dark, 0) and t / flat are monotone
// in x, so both maxima follow from the integer maximum of the group -- a pure streaming read (the generic kernel
// spends ~10 float64 operations per pixel on the same answer: 143 us instead of ~30 for one 4 x 4096^2 assay).
template <typename T>
__global__ __launch_bounds__(256) void k_flatfield_max_int(const T* __restrict__ tiles, int64_t group_elems, double dark,
                                                            double flat, double* __restrict__ out) {
  constexpr int N = VecOf<T>::N;
  tiles += (int64_t)blockIdx.y * group_elems;
  out += 2 * blockIdx.y;
  uint32_t xmax = 0;
  const int64_t nvec = group_elems / N;  // the launcher guarantees 16-byte alignment of every group
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  int64_t v = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  for (; v + 3 * stride < nvec; v += 4 * stride) {  // four loads in flight per lane
    T x[4][N];
#pragma unroll
    for (int q = 0; q < 4; ++q) load_vec<T, N>(tiles + (v + q * stride) * N, x[q]);
#pragma unroll
    for (int q = 0; q < 4; ++q)
#pragma unroll
      for (int j = 0; j < N; ++j) xmax = max(xmax, (uint32_t)x[q][j]);
  }
  for (; v < nvec; v += stride) {
    T x[N];
    load_vec<T, N>(tiles + v * N, x);
#pragma unroll
    for (int j = 0; j < N; ++j) xmax = max(xmax, (uint32_t)x[j]);
  }
  for (int64_t p = nvec * N + (int64_t)blockIdx.x * blockDim.x + threadIdx.x; p < group_elems; p += stride)
    xmax = max(xmax, (uint32_t)tiles[p]);
  double m1 = (double)xmax - dark;  // every workgroup sees at least one pixel (grid <= nvec / 256 + 1)
  m1 = m1 < 0.0 ? 0.0 : m1;
  block_atomic_max2(m1, m1 / flat, out);
}

// One pixel of the fast paths below: can it beat the running maximum of t / flat?  The test runs in float32 against
// the lane's own threshold `thr` and an extra one, `gthr`; a pixel that passes pays for the exact float64 division and
// raises m2 and thr.  rc: the float32 reciprocal of fl.
__device__ __forceinline__ void max2_step(uint32_t xi, float dk_f, double dark, float fl, float rc, float gthr, double& m2,
                                          float& thr) {
  const float t_f = fmaxf((float)xi - dk_f, 0.0f);
  if (flat_in_range_f32(fl) && t_f * rc <= fmaxf(thr, gthr)) return;  // provably below the running maximum
  double t = (double)xi - dark;
  t = t < 0.0 ? 0.0 : t;
  m2 = mg_nanmax(m2, t / (double)fl);
  thr = (m2 == m2 && m2 < 1e30) ? (float)m2 * (1.0f - 1e-5f) : -INFINITY;
}

// Fast path of pass 1 for integer pixels, scalar dark and a float32 flat image: the test "can this
// pixel beat the running maximum of t / flat?" runs in float32 (reciprocal + multiply, error
// < 1e-6 relative against a 1e-5 margin); only pixels that pass pay for the exact float64 division,
// so the result is still the exact maximum of the exact quotients.  M1 comes from the integer max.
template <typename T>
__global__ __launch_bounds__(256) void k_flatfield_max_fast(const T* __restrict__ tiles, int64_t tiles_per_group,
                                                             int64_t tile_elems, double dark,
                                                             const float* __restrict__ d_flat,
                                                             double* __restrict__ out) {
  constexpr int N = VecOf<T>::N;
  const int group = blockIdx.y;
  tiles += (int64_t)group * tiles_per_group * tile_elems;
  out += 2 * group;
  const float dk_f = (float)dark;
  uint32_t xmax = 0;
  bool any = false;
  double m2 = -INFINITY;
  float thr = -INFINITY;
  const int64_t nvec = tile_elems / N;  // the launcher guarantees tile_elems % N == 0
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t v = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; v < nvec; v += stride) {
    float fl[N], rc[N];
    load_f32<N>(d_flat + v * N, fl);
#pragma unroll
    for (int j = 0; j < N; ++j) rc[j] = __builtin_amdgcn_rcpf(fl[j]);
    any = true;
    // four tiles (channels) of the group per trip: their loads are issued together -- behind the data-dependent
    // test below the compiler keeps them one round trip apart
    for (int64_t g0 = 0; g0 < tiles_per_group; g0 += 4) {
      T x4[4][N];
#pragma unroll
      for (int q = 0; q < 4; ++q)
        if (g0 + q < tiles_per_group) load_vec<T, N>(tiles + (g0 + q) * tile_elems + v * N, x4[q]);
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        if (g0 + q >= tiles_per_group) break;
        // the float32 test for all N pixels first, one branch for the chunk: after the first few chunks a pixel that
        // can beat the running maximum is rare, and a branch per pixel cost more than the arithmetic
        bool cand = false;
#pragma unroll
        for (int j = 0; j < N; ++j) {
          const uint32_t xi = (uint32_t)x4[q][j];
          xmax = max(xmax, xi);
          const float t_f = fmaxf((float)xi - dk_f, 0.0f);
          cand |= !(flat_in_range_f32(fl[j]) && t_f * rc[j] <= thr);
        }
        if (!cand) continue;
#pragma unroll
        // (gthr = -inf: no threshold besides the lane's own)
        for (int j = 0; j < N; ++j) max2_step((uint32_t)x4[q][j], dk_f, dark, fl[j], rc[j], -INFINITY, m2, thr);
      }
    }
  }
  double m1 = -INFINITY;
  if (any) {
    m1 = (double)xmax - dark;
    m1 = m1 < 0.0 ? 0.0 : m1;
  }
  block_atomic_max2(m1, m2, out);
}

// The same pass with the flat image read at an eighth of its size: d_rcmax[v] = the largest float32 reciprocal of the
// N flat values of chunk v (-1 if one of them is outside the range the float32 test is valid in).  A chunk whose
// largest pixel, times that, cannot beat the running maximum is done after a few integer maxima -- its flat values are
// not even loaded; after the first chunks that is all but a handful.  (Before: 64 MB of flat image re-read for every
// assay, 2 GB of the pass's 10.7 GB of traffic at 64 assays, and a float32 multiply / compare per pixel.)
template <int N>
__global__ __launch_bounds__(256) void k_flat_rcmax(const float* __restrict__ d_flat, int64_t nvec, float* __restrict__ d_rcmax) {
  for (int64_t v = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; v < nvec; v += (int64_t)gridDim.x * blockDim.x) {
    float m = 0.0f, fl[N];
    bool ok = true;
    load_f32<N>(d_flat + v * N, fl);
#pragma unroll
    for (int j = 0; j < N; ++j) {
      ok = ok && flat_in_range_f32(fl[j]);
      m = fmaxf(m, __builtin_amdgcn_rcpf(fl[j]));
    }
    d_rcmax[v] = ok ? m : -1.0f;
  }
}

template <typename T, bool SHARE>
__global__ __launch_bounds__(256) void k_flatfield_max_lean(const T* __restrict__ tiles, int64_t tiles_per_group,
                                                             int64_t tile_elems, double dark,
                                                             const float* __restrict__ d_flat,
                                                             const float* __restrict__ d_rcmax,
                                                             double* __restrict__ out) {
  constexpr int N = VecOf<T>::N;
  constexpr int UV = 2;  // chunk positions per trip: UV x 4 sixteen-byte loads in flight per lane
  const int group = blockIdx.y;
  tiles += (int64_t)group * tiles_per_group * tile_elems;
  out += 2 * group;
  const float dk_f = (float)dark;
  uint32_t xmax = 0;
  bool any = false;
  double m2 = -INFINITY;
  float thr = -INFINITY;
  const int64_t nvec = tile_elems / N;  // the launcher guarantees tile_elems % N == 0
  // (grid-strided, nontemporal loads.  Measured beside it: contiguous spans per workgroup -- 7.0 TB/s against 5.5 in a
  // plain read, tools/micro/copy_bw.hip -- 1.66 ms here instead of 1.51: four tiles 32 MiB apart walk in step)
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  const int64_t vend = nvec;
  // The threshold a lane tests against comes from its own running maximum AND from the group's (out[1]): the first
  // PUBLISHERS workgroups of a group add the maximum of their first trip to it (a wave at a time, look-first), every
  // lane looks at it on trips 1, 2, 4, 8, ....  A lane of a small batch sees a few dozen chunks: on its own maximum alone a sixth
  // of them took the exact path (one 4 x 4096^2 assay: 81 -> 62 us; 8 assays: 277 -> 239 us).  Any value found there
  // is the exact quotient of a pixel some lane holds in its m2, so a pixel skipped against it cannot be the maximum.
  // SHARE is off where a lane has hundreds of chunks of its own (64 assays: the sharing cost 5 %).
  constexpr int PUBLISHERS = 32;
  float gthr = -INFINITY;
  int trip = 0;
  const bool publish = SHARE && blockIdx.x < PUBLISHERS && (int64_t)(blockIdx.x + 1) * blockDim.x <= nvec;  // (whole waves on trip 0)
  for (int64_t v0 = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; v0 < nvec; v0 += UV * stride) {
    float rcm[UV];
#pragma unroll
    for (int u = 0; u < UV; ++u) rcm[u] = d_rcmax[min(v0 + u * stride, nvec - 1)];
    if (SHARE && trip > 0 && (trip & (trip - 1)) == 0) {  // trips 1, 2, 4, 8, ...: a look every trip cost 10 % at 64 assays
      const double gm = __hip_atomic_load(out + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      if (gm == gm && gm < 1e30 && gm > -INFINITY) gthr = fmaxf(gthr, (float)gm * (1.0f - 1e-5f));
    }
    any = true;
    for (int64_t g0 = 0; g0 < tiles_per_group; g0 += 4) {  // four tiles (channels) of the group per trip, loads together
      T x4[UV][4][N];
#pragma unroll
      for (int u = 0; u < UV; ++u)
#pragma unroll
        for (int q = 0; q < 4; ++q)
          load_vec16<T, N>(tiles + min(g0 + q, tiles_per_group - 1) * tile_elems + min(v0 + u * stride, nvec - 1) * N, x4[u][q],
                           true);
#pragma unroll
      for (int u = 0; u < UV; ++u) {
        const int64_t v = v0 + u * stride;
        if (v >= vend) break;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          if (g0 + q >= tiles_per_group) break;
          uint32_t cm = 0;
#pragma unroll
          for (int j = 0; j < N; ++j) cm = max(cm, (uint32_t)x4[u][q][j]);
          xmax = max(xmax, cm);
          // t -> float(x) - dark -> max(., 0) and the product with a non-negative reciprocal are monotone: if the chunk's
          // largest pixel with the chunk's largest reciprocal stays at or below the threshold, every pixel does
          const float tf = fmaxf((float)cm - dk_f, 0.0f);
          if (rcm[u] >= 0.0f && tf * rcm[u] <= fmaxf(thr, gthr)) continue;
          float fl[N];
          load_f32<N>(d_flat + v * N, fl);
#pragma unroll
          for (int j = 0; j < N; ++j)
            max2_step((uint32_t)x4[u][q][j], dk_f, dark, fl[j], __builtin_amdgcn_rcpf(fl[j]), gthr, m2, thr);
        }
      }
    }
    if (trip == 0 && publish) {  // (block-uniform: every lane of the wave is here)
      const double wm = mg_wave_nanmax(m2);
      if ((threadIdx.x & 63) == 0 && wm == wm && wm > -INFINITY) mg_atomic_nanmax(out + 1, wm);
    }
    ++trip;
  }
  double m1 = -INFINITY;
  if (any) {
    m1 = (double)xmax - dark;
    m1 = m1 < 0.0 ? 0.0 : m1;
  }
  block_atomic_max2(m1, m2, out);
}

// ---- pass 2: apply + stitch (+ output min/max) ----------------------------------------
// The generic pass is k_stitch<T, BL_COPY or BL_FLAT, false, SUBSET> (mg_stitch_kernel.h).
//
// Lean variant for the aligned case (hx % N == 0 and aligned bases: every N-pixel chunk lies
// inside one tile and all accesses are 16-byte vectors); integer pixel types only.
// Arithmetic of the correction, per pixel: the conversion, ONE float64 product with the position's factor, fract,
// the truncating conversion and three compares (15 vector instructions a pixel, measured, where the per-pixel form --
// subtract, clip, two products, floor, subtract, five compares, the group's M1 / M2 divided anew in every row -- took
// 24: 2.55 -> 1.65 ms of vector issue at 64 assays; what it bought is at small batches, 0.55 -> 0.50 ms at 8 assays --
// at 64 the pass waits for memory, see the workgroup order below).  INT_DARK: an integer-valued scalar dark,
// subtracted in the integer domain (two uint16 pixels per instruction).
template <typename T, bool APPLY, bool INT_DARK, bool SUBSET = false>
__global__ __launch_bounds__(256) void k_apply_stitch_aligned(StitchSrc<T> s, int n_planes, int clip, int hy, int hx,
                                                               T* __restrict__ image, double* __restrict__ d_minmax,
                                                               int rows_per_block, PlaneSel sel) {
  constexpr int N = VecOf<T>::N;
  constexpr int PB = PLANES_PER_BLOCK;
  const int n_tr = s.n_tr, n_tc = s.n_tc, tx = s.tx, planes_per_group = s.planes_per_group;
  // Which part of the grid this workgroup is: the plane groups (z) of one (x, y) part read the same rows of the flat /
  // dark images -- 64 MB of float32 per plane group at 4096^2, 2 GB of the pass's 19 GB at 64 assays when the parts
  // are worked through plane group by plane group (the hardware's order: x, y, then z).  Workgroups are dealt to the
  // eight XCDs in turn, each XCD has its own L2: XCD k takes the (x, y) parts k, k + 8, ... and runs all plane groups
  // of a part one after the other, so the flat rows of a part are fetched once and then found in that XCD's L2.
  int bx = blockIdx.x, by = blockIdx.y, bz = blockIdx.z;
  if (APPLY && gridDim.z >= 16 && ((gridDim.x * gridDim.y) & 7) == 0) {  // (4 plane groups: 0.50 -> 0.55 ms; 32: 3.76 -> 3.47)
    const uint32_t lin = blockIdx.x + gridDim.x * (blockIdx.y + gridDim.y * blockIdx.z);
    const uint32_t xcd = lin & 7, slot = lin >> 3;
    bz = slot % gridDim.z;
    const uint32_t xy = (slot / gridDim.z) * 8 + xcd;
    bx = xy % gridDim.x;
    by = xy / gridDim.x;
  }
  const int plane0 = bz * PB;  // (SUBSET: n_planes, plane0 count SELECTED planes; pl[b] is the plane itself)
  const int np = min(PB, n_planes - plane0);
  const int h_out = n_tr * hy, w_out = n_tc * hx;
  const int ox0 = (bx * blockDim.x + threadIdx.x) * N;
  int pl[PB];
#pragma unroll
  for (int b = 0; b < PB; ++b) pl[b] = (!SUBSET || b < np) ? sel_plane<SUBSET>(plane0 + b, planes_per_group, sel) : 0;
  PlaneMinMax<T, PB> mm;
  const int64_t tile_elems = (int64_t)s.ty * tx, plane_elems = (int64_t)n_tr * n_tc * tile_elems;
  // per plane, once per workgroup (scalar registers): the quotient of the group's maxima and whether the fast path
  // holds for them (the maxima themselves are read again by the rare exact path: 16 more scalar registers spilled)
  double kka[PB];
  uint32_t ok_mask = 0;
#pragma unroll
  for (int b = 0; b < PB; ++b) {
    kka[b] = 1.0;
    if (APPLY && b < np) {
      const int group = pl[b] / planes_per_group;
      const double m1 = s.d_max2[2 * group], m2 = s.d_max2[2 * group + 1];
      double kk;
      const bool ok = group_quotient(m1, m2, kk);
      kka[b] = uniform_f64(kk);
      ok_mask |= ok ? (1u << b) : 0u;
    }
  }
  ok_mask = __builtin_amdgcn_readfirstlane(ok_mask);
  const uint32_t dark_i = INT_DARK ? (uint32_t)s.dark : 0u;
  if (ox0 < w_out)
  for (int yg = by; yg * rows_per_block < h_out; yg += gridDim.y) {  // (as in k_stitch)
    const int row_end = min((yg + 1) * rows_per_block, h_out);
    const int tc0 = ox0 / hx;
    const int x0 = ox0 - tc0 * hx + clip;
    for (int oy = yg * rows_per_block; oy < row_end; ++oy) {
      const int tr = oy / hy;
      const int64_t p0 = (int64_t)(oy - tr * hy + clip) * tx + x0;
      const int64_t src0 = ((int64_t)tr * n_tc + tc0) * tile_elems + p0;
      double dk[N], fl[N], rr[N];
      bool flat_bad = false;  // a flat value outside the range the reciprocal path is valid in
      if (APPLY) {
        if (!INT_DARK) load_field<N>(s.d_dark, s.dark_dt, p0, s.dark, dk);
        load_field<N>(s.d_flat, s.flat_dt, p0, s.flat, fl);
#pragma unroll
        for (int j = 0; j < N; ++j) {
          rr[j] = refined_rcp(fl[j]);
          flat_bad |= rr[j] == 0.0;
        }
      }
      // all planes' loads are issued before the first pixel is corrected (more bytes in flight per lane)
      T xin[PB][N];
#pragma unroll
      for (int b = 0; b < PB; ++b)
        if (b < np) load_vec16<T, N>(s.tiles + (int64_t)pl[b] * plane_elems + src0, xin[b], false);
      double rk[N];
      double kk_of_rk = -1.0;  // the quotient rk was made with (planes of one group follow each other)
      bool rk_large = true;
#pragma unroll
      for (int b = 0; b < PB; ++b) {
        if (b >= np) break;
        T o[N];
        T(&x)[N] = xin[b];
        if (APPLY) {
          if (kka[b] != kk_of_rk) {  // (uniform: a new group)
            kk_of_rk = kka[b];
            rk_large = chunk_factors<N>(rr, kk_of_rk, rk);
          }
          const bool rk_bad = rk_large || flat_bad || !((ok_mask >> b) & 1u);
          correct_chunk_rk<T, N, INT_DARK>(x, dark_i, dk, fl, rk, rk_bad, s.d_max2, pl[b], planes_per_group, o);
        } else {
#pragma unroll
          for (int j = 0; j < N; ++j) o[j] = x[j];
        }
        if (d_minmax) mm.add(b, o);
        store_vec16<T, N>(image + ((int64_t)pl[b] * h_out + oy) * w_out + ox0, o, false);
      }
    }
  }
  if (d_minmax) {
    if constexpr (SUBSET) mm.flush(np, d_minmax, SelBase{plane0, planes_per_group, sel});
    else mm.flush(np, d_minmax, plane0);
  }
}

// ---- per-plane min/max of strided planes ------------------------------------------------
template <typename T>
__global__ __launch_bounds__(256) void k_plane_minmax(const T* __restrict__ src, int64_t plane_stride, int h, int w,
                                                       int64_t row_stride, double* __restrict__ d_minmax) {
  constexpr int N = VecOf<T>::N;
  const int plane = blockIdx.y;
  const T* base = src + (int64_t)plane * plane_stride;
  PlaneMinMax<T, 1> mm;
  const int vec_per_row = (w + N - 1) / N;
  const int64_t total = (int64_t)h * vec_per_row;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (IsIntegral<T>::value && w % N == 0 && aligned16(base) && (row_stride * (int64_t)sizeof(T)) % 16 == 0) {
    // integer pixels, rows of whole 16-byte vectors: integer min / max, four loads in flight per lane (one 4096^2
    // uint16 plane: 28 -> ~10 us; the float64 compares of the general loop kept the lanes busy, one load at a time)
    for (; i < total; i += 4 * stride) {
      T x[4][N];
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int64_t iq = min(i + q * stride, total - 1);  // (a clamped repeat does not change a min / max)
        const int r = (int)(iq / vec_per_row);
        const int c0 = (int)(iq - (int64_t)r * vec_per_row) * N;
        load_vec16<T, N>(base + (int64_t)r * row_stride + c0, x[q], false);
      }
#pragma unroll
      for (int q = 0; q < 4; ++q) mm.add(0, x[q]);
    }
    i = total;
  }
  for (; i < total; i += stride) {
    const int r = (int)(i / vec_per_row);
    const int c0 = (int)(i - (int64_t)r * vec_per_row) * N;
    const T* p = base + (int64_t)r * row_stride + c0;
    if (c0 + N <= w) {
      T x[N];
      load_vec<T, N>(p, x);
      mm.add(0, x);
    } else {
      for (int j = 0; c0 + j < w; ++j) mm.add(0, p[j]);
    }
  }
  mm.flush(1, d_minmax, plane);
}

template <typename T>
int launch_max(const void* d_tiles, int64_t tiles_per_group, int n_groups, int64_t tile_elems, double dark,
               const void* d_dark, int dark_dt, double flat, const void* d_flat, int flat_dt, double* d_max2,
               float* d_scratch, int64_t scratch_floats, hipStream_t s) {
  if (tiles_per_group == 0 || n_groups == 0 || tile_elems == 0) return MG_OK;
  constexpr int N = VecOf<T>::N;
  const int64_t nvec = tile_elems / N + 1;
  const int per_group = std::min(MG_FLATFIELD_MAX_WALK_PER_GROUP, std::max(1, MG_FLATFIELD_MAX_WALK / n_groups));
  int blocks = (int)std::min<int64_t>((nvec + 255) / 256, per_group);
  if constexpr (IsIntegral<T>::value) {  // (the integer-only kernels exist for integer pixels only)
    const int64_t group_elems = tiles_per_group * tile_elems;
    if (!d_dark && !d_flat && flat > 0.0 && flat < 1e300 && fabs(dark) < 1e300 && aligned16(d_tiles) &&
        (group_elems * (int64_t)sizeof(T)) % 16 == 0) {
      const int64_t gvec = group_elems / N;
      // (every workgroup ends with two compare-and-swap maxima on the group's cache line: few, long-running workgroups)
      const int gb = (int)std::max<int64_t>(1, std::min<int64_t>(gvec / 256, std::min(MG_FLATFIELD_MAX_WALK_PER_GROUP, std::max(MG_FLATFIELD_MAX_INT_WALK_MIN, MG_FLATFIELD_MAX_INT_WALK / n_groups))));
      hipLaunchKernelGGL((k_flatfield_max_int<T>), dim3(gb, n_groups), dim3(256), 0, s, (const T*)d_tiles, group_elems, dark,
                         flat, d_max2);
      MG_CHECK_LAUNCH();
      return MG_OK;
    }
    if (!d_dark && d_flat && flat_dt == MG_F32 && tile_elems % N == 0 && aligned16(d_flat) && aligned16(d_tiles) &&
        fabs(dark) < 16777216.0 && (double)(float)dark == dark) {
      if (d_scratch && scratch_floats >= tile_elems / N && (reinterpret_cast<uintptr_t>(d_scratch) & 3) == 0) {
        const int64_t cvec = tile_elems / N;  // (d_scratch: the bound of this flat image, mg_flatfield_bound)
        // one resident round of workgroups in all (74 VGPRs: 6 per CU), however many groups share them: every workgroup
        // ends with two compare-and-swap maxima on its group's cache line
        const int per = (int)std::max<int64_t>(1, std::min<int64_t>((cvec + 255) / 256, std::max(1, MG_FLATFIELD_MAX_LEAN_WALK / n_groups)));
        const int64_t chunks_per_lane = (cvec + (int64_t)per * 256 - 1) / ((int64_t)per * 256) * tiles_per_group;
        with_flag(chunks_per_lane < 512, [&](auto share) {
          hipLaunchKernelGGL((k_flatfield_max_lean<T, decltype(share)::value>), dim3(per, n_groups), dim3(256), 0, s,
                             (const T*)d_tiles, tiles_per_group, tile_elems, dark, (const float*)d_flat, d_scratch, d_max2);
          return 0;
        });
        MG_CHECK_LAUNCH();
        return MG_OK;
      }
      hipLaunchKernelGGL((k_flatfield_max_fast<T>), dim3(blocks, n_groups), dim3(256), 0, s, (const T*)d_tiles,
                         tiles_per_group, tile_elems, dark, (const float*)d_flat, d_max2);
      MG_CHECK_LAUNCH();
      return MG_OK;
    }
  }
  hipLaunchKernelGGL((k_flatfield_max<T>), dim3(blocks, n_groups), dim3(256), 0, s, (const T*)d_tiles, tiles_per_group,
                     tile_elems, dark, d_dark, dark_dt, flat, d_flat, flat_dt, d_max2);
  MG_CHECK_LAUNCH();
  return MG_OK;
}

// Pass 2 for a source: the aligned kernel where it applies, else the generic one.  plane_mask != 0: a selection
// (apply only).
template <typename T>
int launch_apply(const StitchSrc<T>& src, int64_t n_planes, int overlap, bool apply, void* d_image, double* d_minmax,
                 hipStream_t s, uint32_t plane_mask = 0) {
  const MgStitchGeom g = mg_stitch_geom(src.ty, src.tx, overlap, src.n_tr, src.n_tc);
  if (n_planes == 0 || g.h_out == 0 || g.w_out == 0) return MG_OK;
  constexpr int N = VecOf<T>::N;
  if (n_planes > 0x7FFFFFF0) return MG_EINVAL;
  // a selection: from here on n_planes counts the selected planes, the kernels map them
  const PlaneSel sel{plane_mask, __builtin_popcount(plane_mask)};
  if (plane_mask) n_planes = n_planes / src.planes_per_group * sel.n_sel;
  if constexpr (IsIntegral<T>::value) {
    const bool aligned = g.hx % N == 0 && src.tx % N == 0 && g.clip % N == 0 && aligned16(src.tiles) && aligned16(d_image) &&
                         (!src.d_flat || aligned16(src.d_flat)) && (!src.d_dark || aligned16(src.d_dark));
    if (aligned) {
      int rows;
      const dim3 grid = stitch_grid<N>(g.h_out, g.w_out, n_planes, rows);
      if (grid.y > MG_WALK_MAX_Y || grid.z > MG_WALK_MAX_Y) return MG_EINVAL;
      // an integer-valued scalar dark inside the pixel range: subtracted in the integer domain
      const bool int_dark = apply && dark_is_int(src.d_dark, src.dark);
      auto launch = [&](auto ap, auto id, auto sub) {
        hipLaunchKernelGGL((k_apply_stitch_aligned<T, decltype(ap)::value, decltype(id)::value, decltype(sub)::value>), grid,
                           dim3(256), 0, s, src, (int)n_planes, g.clip, g.hy, g.hx, (T*)d_image, d_minmax, rows, sel);
        MG_CHECK_LAUNCH();
        return (int)MG_OK;
      };
      if (!apply) return launch(std::false_type{}, std::false_type{}, std::false_type{});
      return with_flag(int_dark, [&](auto id) {
        return with_flag(plane_mask != 0, [&](auto sub) { return launch(std::true_type{}, id, sub); });
      });
    }
  }
  if (plane_mask) return launch_stitch<BL_FLAT, false, true>(src, n_planes, overlap, sel, d_image, d_minmax, s);
  if (apply) return launch_stitch<BL_FLAT, false, false>(src, n_planes, overlap, sel, d_image, d_minmax, s);
  return launch_stitch<BL_COPY, false, false>(src, n_planes, overlap, sel, d_image, d_minmax, s);
}

template <typename T>
int launch_minmax(const void* d_src, int n_planes, int64_t plane_stride, int h, int w, int64_t row_stride,
                  double* d_minmax, hipStream_t s) {
  if (n_planes == 0 || h == 0 || w == 0) return MG_OK;
  const int64_t total = (int64_t)h * ((w + VecOf<T>::N - 1) / VecOf<T>::N);
  int bx = (int)std::min<int64_t>((total + 255) / 256, MG_PLANE_MINMAX_WALK);
  hipLaunchKernelGGL((k_plane_minmax<T>), dim3(bx, n_planes), dim3(256), 0, s, (const T*)d_src, plane_stride, h, w,
                     row_stride, d_minmax);
  MG_CHECK_LAUNCH();
  return MG_OK;
}

// The chunk of the flat image one entry of mg_flatfield_bound's scratch stands for: that of the integer fast path
// of pass 1 (the only one that uses the scratch), 0 for the other pixel types.
constexpr int bound_chunk(int dtype) {
  return dtype == MG_U8 ? VecOf<uint8_t>::N : dtype == MG_U16 ? VecOf<uint16_t>::N : 0;
}

}  // namespace

extern "C" int mg_version(void) { return 1; }

extern "C" int64_t mg_flatfield_max_scratch_floats(int dtype, int ty, int tx) {
  if (ty <= 0 || tx <= 0) return -1;
  const int n = bound_chunk(dtype);
  return n ? ((int64_t)ty * tx + n - 1) / n : 0;
}

extern "C" int mg_flatfield_bound(const void* d_flat, int flat_dtype, int dtype, int ty, int tx, float* d_scratch,
                                  int64_t scratch_floats, void* stream) {
  if (!d_flat || !d_scratch || ty <= 0 || tx <= 0 || flat_dtype != MG_F32) return MG_EINVAL;
  const int64_t need = mg_flatfield_max_scratch_floats(dtype, ty, tx);
  const int64_t tile_elems = (int64_t)ty * tx;
  if (need <= 0 || scratch_floats < need || tile_elems % bound_chunk(dtype) || !aligned16(d_flat) ||
      (reinterpret_cast<uintptr_t>(d_scratch) & 3))
    return MG_EINVAL;
  hipStream_t s = mg_stream(stream);
  return mg_dispatch_pixel(dtype, [&](auto t) {
    using T = decltype(t);
    if constexpr (IsIntegral<T>::value) {  // (need > 0: an integer pixel type)
      constexpr int N = VecOf<T>::N;
      const int64_t cvec = tile_elems / N;
      const dim3 grid((unsigned)std::min<int64_t>((cvec + 255) / 256, MG_FLATFIELD_BOUND_WALK));
      hipLaunchKernelGGL((k_flat_rcmax<N>), grid, dim3(256), 0, s, (const float*)d_flat, cvec, d_scratch);
      MG_CHECK_LAUNCH();
      return (int)MG_OK;
    } else {
      return (int)MG_EINVAL;
    }
  });
}

extern "C" int mg_flatfield_max(const void* d_tiles, int dtype, int64_t n_tiles, int n_groups, int ty, int tx,
                                double dark, const void* d_dark, int dark_dtype, double flat, const void* d_flat,
                                int flat_dtype, double* d_max2, float* d_scratch, int64_t scratch_floats, void* stream) {
  if (!d_tiles || !d_max2 || n_tiles < 0 || ty <= 0 || tx <= 0 || n_groups <= 0 || n_groups > 65535) return MG_EINVAL;
  if (n_tiles % n_groups) return MG_EINVAL;
  if (!field_dtype_ok(d_dark, dark_dtype) || !field_dtype_ok(d_flat, flat_dtype)) return MG_EINVAL;
  const int64_t tile_elems = (int64_t)ty * tx, tpg = n_tiles / n_groups;
  hipStream_t s = mg_stream(stream);
  return mg_dispatch_pixel(dtype, [&](auto t) {
    return launch_max<decltype(t)>(d_tiles, tpg, n_groups, tile_elems, dark, d_dark, dark_dtype, flat, d_flat, flat_dtype,
                                   d_max2, d_scratch, scratch_floats, s);
  });
}

extern "C" int mg_flatfield_is_identity(int dtype, double dark, const void* d_dark, double flat, const void* d_flat) {
  return (dtype == MG_U8 || dtype == MG_U16) && !d_dark && !d_flat && dark == 0.0 && flat == 1.0;
}

extern "C" int mg_flatfield_apply_stitch(const void* d_tiles, int dtype, int64_t n_planes, int n_tile_rows,
                                         int n_tile_cols, int ty, int tx, int overlap, int apply_flatfield,
                                         int planes_per_group, double dark, const void* d_dark, int dark_dtype,
                                         double flat, const void* d_flat, int flat_dtype, const double* d_max2,
                                         void* d_image, double* d_minmax, void* stream) {
  if (n_tile_rows <= 0 || n_tile_cols <= 0 || ty <= 0 || tx <= 0) return MG_EINVAL;
  if (overlap < 0 || overlap >= ty || overlap >= tx) return MG_EINVAL;
  hipStream_t s = mg_stream(stream);
  return flatfield_stitch_entry(
      d_tiles, dtype, n_planes, n_tile_rows, n_tile_cols, ty, tx, apply_flatfield, planes_per_group, dark, d_dark, dark_dtype,
      flat, d_flat, flat_dtype, d_max2, d_image, [&](const auto& src, auto mode) {
        return launch_apply(src, n_planes, overlap, decltype(mode)::value == BL_FLAT, d_image, d_minmax, s);
      });
}

extern "C" int mg_flatfield_apply_stitch_planes(const void* d_tiles, int dtype, int64_t n_planes, int n_tile_rows,
                                                int n_tile_cols, int ty, int tx, int overlap, int planes_per_group,
                                                int plane_mask, double dark, const void* d_dark, int dark_dtype,
                                                double flat, const void* d_flat, int flat_dtype, const double* d_max2,
                                                void* d_image, double* d_minmax, void* stream) {
  if (!d_tiles || !d_image || !d_max2 || n_planes < 0 || n_tile_rows <= 0 || n_tile_cols <= 0 || ty <= 0 || tx <= 0)
    return MG_EINVAL;
  if (overlap < 0 || overlap >= ty || overlap >= tx) return MG_EINVAL;
  if (planes_per_group <= 0 || planes_per_group > 31 || n_planes % planes_per_group || plane_mask < 0 ||
      (plane_mask >> planes_per_group))
    return MG_EINVAL;
  if (!field_dtype_ok(d_dark, dark_dtype) || !field_dtype_ok(d_flat, flat_dtype)) return MG_EINVAL;
  if (plane_mask == 0) return MG_OK;  // nothing selected
  hipStream_t s = mg_stream(stream);
  // (no identity shortcut: the selected planes always go through the correction's arithmetic, whose result for the
  // identity operands is the pixel itself)
  return mg_dispatch_pixel(dtype, [&](auto t) {
    using T = decltype(t);
    const StitchSrc<T> src{(const T*)d_tiles, n_tile_rows, n_tile_cols, ty, tx, planes_per_group,
                           dark, d_dark, dark_dtype, flat, d_flat, flat_dtype, d_max2};
    return launch_apply(src, n_planes, overlap, true, d_image, d_minmax, s, (uint32_t)plane_mask);
  });
}

extern "C" int mg_plane_minmax(const void* d_src, int dtype, int n_planes, int64_t plane_stride, int h, int w,
                               int64_t row_stride, double* d_minmax, void* stream) {
  if (!d_src || !d_minmax || n_planes < 0 || h < 0 || w < 0) return MG_EINVAL;
  if (n_planes > 65535) return MG_EINVAL;
  hipStream_t s = mg_stream(stream);
  return mg_dispatch_pixel(dtype, [&](auto t) {
    return launch_minmax<decltype(t)>(d_src, n_planes, plane_stride, h, w, row_stride, d_minmax, s);
  });
}
