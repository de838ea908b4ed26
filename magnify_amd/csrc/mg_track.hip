// Following beads through a time series ("find_beads: following beads through time").  The reference cuts
// every timepoint's ROI at the bead's time-0 position (find.py:564: "TODO: Don't assume beads don't move across
// timesteps", find.py:564-602); mg_track_beads finds, per bead and timepoint, the integer displacement in
// [-max_drift, max_drift]^2 at which the patch around the bead in plane t correlates best with the patch at t_ref.
//
// Contract, per bead (row, col), timepoint t, md = max_drift, W = 2 md + 1:
//   * patch: the pixels (y, x) with |y - row| <= half, |x - col| <= half, md <= y < h - md, md <= x < w - md -- a
//     rectangle, every displaced read inside the image; n its size (the same for every displacement, may be 0);
//   * fixed = [n, sum B, sum B^2], B = plane[t_ref] over the patch; per displacement (dy, dx):
//     [sum A, sum A^2, sum A B] with A(y, x) = plane[t][y + dy, x + dx] -- the layout and meaning of mg_seam_sums;
//   * z = (n sAB - sA sB) / sqrt((n sAA - sA^2) (n sBB - sB^2)) in float64, every operation rounded on its own
//     (-ffp-contract=off), 0 where a variance term is <= 0 or z is not finite: register.seam_scores, operation for
//     operation.  Float64 `/` and sqrt are the IEEE ones: in the device listing of this file every one of the five
//     unrolled scoring passes of each instantiation has the v_div_scale_f64 / v_rcp_f64 / v_fma_f64 chain /
//     v_div_fmas_f64 / v_div_fixup_f64 sequence (the compiler's correctly rounded division) and the v_rsq_f64-seeded
//     sqrt with its correction steps and the v_cmp_class_f64 fix-up (its correctly rounded sqrt); -fno-fast-math
//     keeps both;
//   * pick: the largest z; ties to the smallest dy^2 + dx^2, then the smallest dy, then the smallest dx
//     (register.pick_displacements): a flat or empty patch gives (0, 0) with score 0.
//
// All sums are accumulated in float64.  For integer pixels that is exact: every partial sum is an integer of at most
// 9025 * 65535^2 < 2^46 < 2^53 (9025 = 95^2, the largest patch), so the float64 adds and fused multiply-adds never
// round and the int64 written is the exact sum (a 64-bit integer multiply-add is a quarter-rate instruction on
// gfx950, the float64 FMA a full-rate one).  For float pixels the order of the additions is fixed by the launch
// geometry alone: the same bits on every call.  No atomics.
//
// k_track: one workgroup of 256 per (bead, timepoint).  The patch is walked in strips of S rows (S = all of them
// where the layout fits); per strip
//   1. the template strip (S x pw) and the window strip of plane t with its halo ((S + 2 md) x (pw + 2 md)) are
//      staged in LDS as float (u8 / u16 / f32 pixels: exact) or double;
//   2. box sums: a thread per (window row, {A, A^2}) makes the W row sums of width pw from the row's core
//      [2 md, pw) and the prefix / suffix sums of the 2 md columns on either side -- O(row), additions only (no
//      running difference: nothing cancels for float pixels) -- into a (rows, W, 2) float64 table in LDS; then a
//      thread per displacement adds the table's S rows under it.  sum B, sum B^2: a block reduction in a fixed order;
//   3. sum A B: a work item is (dy, a run of TRK_R consecutive dx, row group k of K); it walks its rows of the strip
//      TRK_R template pixels at a time: TRK_R template values and 2 TRK_R - 1 window values in registers feed
//      TRK_R^2 fused multiply-adds on TRK_R accumulators (one per dx of the run).
// LDS rows are padded to 18 four-byte words past a multiple of 64: the rows a 32-lane group reads at once (K row
// groups x two or three dy) and the runs' 8-byte reads in them then fall on disjoint banks (ds_read_b64: 64 banks);
// lanes of one row group read one template address (a broadcast).  After the last strip the K row groups of a
// displacement are added in k order through LDS, the scores are made and the best one is picked with a total order
// (so the reduction tree does not matter).
//
// mg_track_beads_based ("find_beads: following a stage that moved") is the same kernel, instantiated with
// BASED: the search of timepoint t is centred on base[t] = (by, bx) -- the offset the whole stage moved by, found on
// binned planes (mg_bin.hip, track.stage_drift).  The patch of (bead, t) is then also cut to the image itself and to
// md <= y + by < h - md, md <= x + bx < w - md (in 64 bits: a base far outside the image leaves no pixel), so n and
// `fixed` are per (bead, t); A(y, x) = plane[t][y + by + dy, x + bx + dx]; the shift written is (by + dy, bx + dx);
// row t_ref ignores its base.  With an all-zero base every number is the plain instantiation's.  The plain
// instantiation compiles to the resources it had before the flag (117 VGPRs, 112 for float64 pixels; no scratch),
// the based one to 121 (117).
//
// Roofline: VALU (float64 FMA), not HBM: n W^2 multiply-adds per (bead, timepoint) against (pw + 2 md)^2 + pw^2
// pixels read once (DESIGN.md has the measured rates).
#include <math.h>

#include "mg_common.h"

namespace {

constexpr int TRK_R = 6;                     // consecutive dx per work item (even: the runs start 8-byte aligned)
constexpr int TRK_MAX_DRIFT = 16;            // W^2 = 1089 displacements: TRK_PASSES passes of 256 threads
constexpr int TRK_MAX_SIDE = 95;             // 2 half + 1
constexpr int TRK_MAX_WINDOW = 127;          // 2 half + 1 + 2 max_drift: a thread per (window row, {A, A^2})
constexpr int TRK_PASSES = ((2 * TRK_MAX_DRIFT + 1) * (2 * TRK_MAX_DRIFT + 1) + 255) / 256;
constexpr int TRK_LDS_SMALL = 40 * 1024;     // four workgroups per CU
constexpr int TRK_LDS_BUDGET = 64 * 1024;

template <typename T>
struct TrackTypes {
  using L = float;  // u8 / u16: exact in float
  using Out = long long;
};
template <>
struct TrackTypes<float> {
  using L = float;
  using Out = double;
};
template <>
struct TrackTypes<double> {
  using L = double;
  using Out = double;
};

struct TrackGeom {
  int n_t, h, w, t_ref, half, md;
  int64_t plane_stride;
  int S, stride, K, NR;  // strip rows, LDS row stride (elements) of both tiles, row groups, runs per dy
};

// N consecutive LDS elements from an 8-byte aligned address as float64 (N even)
template <int N>
__device__ __forceinline__ void trk_load(const float* __restrict__ p, double* out) {
#pragma unroll
  for (int i = 0; i < N; i += 2) {
    const float2 v = *reinterpret_cast<const float2*>(p + i);
    out[i] = (double)v.x, out[i + 1] = (double)v.y;
  }
}
template <int N>
__device__ __forceinline__ void trk_load(const double* __restrict__ p, double* out) {
#pragma unroll
  for (int i = 0; i < N; ++i) out[i] = p[i];
}

// candidate order of the pick: larger z first; ties: smaller dy^2 + dx^2, then smaller dy, then smaller dx
__device__ __forceinline__ bool trk_better(double za, int da, double zb, int db, int W, int md) {
  if (za != zb) return za > zb;
  const int ya = da / W - md, xa = da - (da / W) * W - md, yb = db / W - md, xb = db - (db / W) * W - md;
  const int ra = ya * ya + xa * xa, rb = yb * yb + xb * xb;
  if (ra != rb) return ra < rb;
  if (ya != yb) return ya < yb;
  return xa < xb;
}

// grid (bead * n_t + t).  BASED (mg_track_beads_based): the search of timepoint t is centred on base[t] = (by, bx), the
// patch is also cut to where the displaced reads stay inside the image (so n depends on t) and `fixed` has a row per
// (bead, t); with an all-zero base every number is the one the plain instantiation makes.
template <typename T, bool BASED>
__global__ __launch_bounds__(256) void k_track(const T* __restrict__ planes, TrackGeom g, const int32_t* __restrict__ beads,
                                               int32_t* __restrict__ shift, double* __restrict__ score,
                                               typename TrackTypes<T>::Out* __restrict__ sums,
                                               typename TrackTypes<T>::Out* __restrict__ fixed,
                                               const int32_t* __restrict__ base) {
  using L = typename TrackTypes<T>::L;
  using Out = typename TrackTypes<T>::Out;
  constexpr int R = TRK_R;
  extern __shared__ __attribute__((aligned(16))) unsigned char trk_lds[];
  __shared__ double s_part[2][MG_MINMAX_WAVES];
  __shared__ double s_best_z[MG_MINMAX_WAVES];
  __shared__ int s_best_d[MG_MINMAX_WAVES];
  const int tid = threadIdx.x;
  const int bead = blockIdx.x / g.n_t, t = blockIdx.x - bead * g.n_t;
  const int md = g.md, W = 2 * md + 1, D = W * W;
  const int64_t slot = (int64_t)bead * g.n_t + t;
  const bool is_ref = t == g.t_ref;
  if (is_ref && !sums && !fixed) {  // the product's call: row t_ref is a constant
    if (tid == 0) shift[2 * slot] = 0, shift[2 * slot + 1] = 0, score[slot] = 1.0;
    return;
  }
  // the patch: rows [y0, y0 + ph), columns [x0, x0 + pw)
  const long long row = beads[3 * bead], col = beads[3 * bead + 1];
  long long y0l = max(row - g.half, (long long)md), y1l = min(row + g.half, (long long)g.h - md - 1);
  long long x0l = max(col - g.half, (long long)md), x1l = min(col + g.half, (long long)g.w - md - 1);
  long long by = 0, bx = 0;
  if constexpr (BASED) {
    if (!is_ref) by = base[2 * t], bx = base[2 * t + 1];  // (row t_ref ignores its base)
    // inside the image, and md <= y + by < h - md, md <= x + bx < w - md; in 64 bits: a base far outside the image
    // leaves no pixel
    y0l = max(max(row - g.half, 0LL), md - by), y1l = min(min(row + g.half, (long long)g.h - 1), (long long)g.h - md - 1 - by);
    x0l = max(max(col - g.half, 0LL), md - bx), x1l = min(min(col + g.half, (long long)g.w - 1), (long long)g.w - md - 1 - bx);
  }
  // where `fixed` of this (bead, t) goes, if anywhere
  Out* out_fixed = !fixed ? nullptr : BASED ? fixed + 3 * slot : is_ref ? fixed + 3 * (int64_t)bead : nullptr;
  const int ph = (int)max(0LL, y1l - y0l + 1), pw = (int)max(0LL, x1l - x0l + 1);
  const int n = ph * pw;
  Out* out_sums = sums ? sums + slot * D * 3 : nullptr;
  if (n == 0) {  // (uniform: the whole workgroup leaves)
    if (out_sums)
      for (int e = tid; e < D * 3; e += 256) out_sums[e] = (Out)0;
    if (tid == 0) {
      shift[2 * slot] = 0, shift[2 * slot + 1] = 0, score[slot] = is_ref ? 1.0 : 0.0;
      if (out_fixed) out_fixed[0] = (Out)0, out_fixed[1] = (Out)0, out_fixed[2] = (Out)0;
    }
    return;
  }
  const int y0 = (int)y0l, x0 = (int)x0l;
  const int ay0 = BASED ? (int)(y0l + by) : y0, ax0 = BASED ? (int)(x0l + bx) : x0;  // the patch in plane t: in [md, . - md)
  const int S = g.S, stride = g.stride, K = g.K, NR = g.NR;
  // LDS: the box-sum table (S + 2 md, W, 2) float64, the window strip, the template strip; after the last strip the
  // row groups' partial sums (K, W, NR R) float64 from the start
  double* sR = reinterpret_cast<double*>(trk_lds);
  L* sA = reinterpret_cast<L*>(sR + (size_t)(S + 2 * md) * W * 2);
  L* sB = sA + (size_t)(S + 2 * md) * stride;
  const T* A = planes + (int64_t)t * g.plane_stride;
  const T* B = planes + (int64_t)g.t_ref * g.plane_stride;
  // this thread's work item of step 3: lanes run over k first, then the runs of a dy, then dy
  const int n_items = W * NR * K;
  const bool live = tid < n_items;
  const int k = tid % K, run = (tid / K) % NR, dyi = live ? tid / (K * NR) : 0, dx0 = run * R;
  double acc[R];
#pragma unroll
  for (int q = 0; q < R; ++q) acc[q] = 0.0;
  double sa[TRK_PASSES], saa[TRK_PASSES];
#pragma unroll
  for (int p = 0; p < TRK_PASSES; ++p) sa[p] = 0.0, saa[p] = 0.0;
  double sb = 0.0, sbb = 0.0;  // (thread 0)
  const int a_cols = pw + 2 * md;
  for (int s0 = 0; s0 < ph; s0 += S) {
    const int sh = min(S, ph - s0), a_rows = sh + 2 * md;
    __syncthreads();  // the strip before has been read
    for (int e = tid; e < a_rows * a_cols; e += 256) {
      const int i = e / a_cols, j = e - i * a_cols;
      sA[i * stride + j] = (L)A[(int64_t)(ay0 + s0 - md + i) * g.w + (ax0 - md + j)];
    }
    double pb = 0.0, pbb = 0.0;
    for (int e = tid; e < sh * pw; e += 256) {
      const int i = e / pw, j = e - i * pw;
      const L b = (L)B[(int64_t)(y0 + s0 + i) * g.w + (x0 + j)];
      sB[i * stride + j] = b;
      pb += (double)b;
      pbb = fma((double)b, (double)b, pbb);
    }
    pb = mg_wave_sum_f64(pb);
    pbb = mg_wave_sum_f64(pbb);
    if ((tid & 63) == 0) s_part[0][tid >> 6] = pb, s_part[1][tid >> 6] = pbb;
    __syncthreads();
    if (tid == 0) {
      sb += ((s_part[0][0] + s_part[0][1]) + s_part[0][2]) + s_part[0][3];
      sbb += ((s_part[1][0] + s_part[1][1]) + s_part[1][2]) + s_part[1][3];
    }
    // 2a. row sums of width pw at the W offsets, of A (which = 0) and A^2 (which = 1)
    if (tid < 2 * a_rows) {
      const int y = tid >> 1;
      const bool sq = tid & 1;
      const L* rowA = sA + y * stride;
      double* tab = sR + (size_t)y * W * 2 + (tid & 1);
      auto term = [&](int x) {
        const double v = (double)rowA[x];
        return sq ? v * v : v;
      };
      if (pw > 2 * md) {
        double core = 0.0, run_sum = 0.0;
        for (int x = 2 * md; x < pw; ++x) core += term(x);
        tab[2 * (2 * md)] = 0.0;
        for (int x = 2 * md - 1; x >= 0; --x) {  // suffix sums of the columns left of the core
          run_sum += term(x);
          tab[2 * x] = run_sum;
        }
        run_sum = 0.0;
        tab[0] = tab[0] + core;
        for (int dx = 1; dx < W; ++dx) {  // prefix sums of the columns right of it
          run_sum += term(pw + dx - 1);
          tab[2 * dx] = (tab[2 * dx] + core) + run_sum;
        }
      } else {
        for (int dx = 0; dx < W; ++dx) {
          double r = 0.0;
          for (int j = 0; j < pw; ++j) r += term(dx + j);
          tab[2 * dx] = r;
        }
      }
    }
    __syncthreads();
    // 2b. the strip's rows under every displacement
#pragma unroll
    for (int p = 0; p < TRK_PASSES; ++p) {
      const int d = tid + 256 * p;
      if (d < D) {
        const int dy = d / W, dx = d - dy * W;
        const double* tab = sR + ((size_t)dy * W + dx) * 2;
        double a1 = sa[p], a2 = saa[p];
        for (int i = 0; i < sh; ++i) {
          a1 += tab[(size_t)i * W * 2];
          a2 += tab[(size_t)i * W * 2 + 1];
        }
        sa[p] = a1, saa[p] = a2;
      }
    }
    // 3. sum A B
    if (live) {
      for (int i = k; i < sh; i += K) {
        const L* rowA = sA + (i + dyi) * stride + dx0;
        const L* rowB = sB + i * stride;
        int j = 0;
        for (; j + R <= pw; j += R) {
          double b[R], a[2 * R];
          trk_load<R>(rowB + j, b);
          trk_load<2 * R>(rowA + j, a);
#pragma unroll
          for (int u = 0; u < R; ++u)
#pragma unroll
            for (int q = 0; q < R; ++q) acc[q] = fma(a[u + q], b[u], acc[q]);
        }
        for (; j < pw; ++j) {
          const double b = (double)rowB[j];
#pragma unroll
          for (int q = 0; q < R; ++q) acc[q] = fma((double)rowA[j + q], b, acc[q]);
        }
      }
    }
  }
  // the K row groups of a displacement, added in k order
  __syncthreads();
  double* sP = reinterpret_cast<double*>(trk_lds);
  const int run_cols = NR * R;
  if (live) {
#pragma unroll
    for (int q = 0; q < R; ++q) sP[((size_t)k * W + dyi) * run_cols + dx0 + q] = acc[q];
  }
  if (tid == 0) s_part[0][0] = sb, s_part[1][0] = sbb;
  __syncthreads();
  const double fn = (double)n, fb = s_part[0][0], fbb = s_part[1][0];
  const double vb = fn * fbb - fb * fb;
  double best_z = -INFINITY;
  int best_d = 0;
#pragma unroll
  for (int p = 0; p < TRK_PASSES; ++p) {
    const int d = tid + 256 * p;
    if (d < D) {
      const int dy = d / W, dx = d - dy * W;
      double sab = sP[(size_t)dy * run_cols + dx];
      for (int kk = 1; kk < K; ++kk) sab += sP[((size_t)kk * W + dy) * run_cols + dx];
      if (out_sums) out_sums[3 * d] = (Out)sa[p], out_sums[3 * d + 1] = (Out)saa[p], out_sums[3 * d + 2] = (Out)sab;
      const double va = fn * saa[p] - sa[p] * sa[p];
      double z = (fn * sab - sa[p] * fb) / sqrt(va * vb);
      if (!(va > 0.0 && vb > 0.0 && fabs(z) <= 1.79769313486231570e308)) z = 0.0;  // (NaN fails the last test too)
      if (trk_better(z, d, best_z, best_d, W, md)) best_z = z, best_d = d;
    }
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    const double oz = __shfl_xor(best_z, off);
    const int od = __shfl_xor(best_d, off);
    if (trk_better(oz, od, best_z, best_d, W, md)) best_z = oz, best_d = od;
  }
  if ((tid & 63) == 0) s_best_z[tid >> 6] = best_z, s_best_d[tid >> 6] = best_d;
  __syncthreads();
  if (tid == 0) {
    for (int i = 1; i < MG_MINMAX_WAVES; ++i)
      if (trk_better(s_best_z[i], s_best_d[i], best_z, best_d, W, md)) best_z = s_best_z[i], best_d = s_best_d[i];
    const int dy = best_d / W, dx = best_d - dy * W;
    shift[2 * slot] = is_ref ? 0 : (int)by + dy - md;
    shift[2 * slot + 1] = is_ref ? 0 : (int)bx + dx - md;
    score[slot] = is_ref ? 1.0 : best_z;
    if (out_fixed) out_fixed[0] = (Out)n, out_fixed[1] = (Out)fb, out_fixed[2] = (Out)fbb;
  }
}

// The strip height, row stride and work-item shape for LDS elements of `elem` bytes; false if not even one row fits.
inline bool track_layout(int elem, TrackGeom& g, size_t& lds_bytes) {
  const int W = 2 * g.md + 1, side = 2 * g.half + 1;
  g.NR = (W + TRK_R - 1) / TRK_R;
  // the last run reads up to NR R - W columns past the window's: they lie inside the row stride
  const int cols = side + g.NR * TRK_R;
  // 18 four-byte words past a multiple of 64 words
  const int unit = 64 * 4 / elem, pad = 18 * 4 / elem;
  g.stride = cols + ((pad - cols) % unit + unit) % unit;
  auto bytes = [&](int S) {
    return (size_t)(S + 2 * g.md) * W * 16 + ((size_t)(S + 2 * g.md) + S) * g.stride * elem;
  };
  // the fewest strips: one or two where they fit the small budget, else what the large one asks for
  int n_strips = 0;
  for (int ns = 1; ns <= 2 && !n_strips; ++ns)
    if (bytes((side + ns - 1) / ns) <= (size_t)TRK_LDS_SMALL) n_strips = ns;
  for (int ns = 1; ns <= side && !n_strips; ++ns)
    if (bytes((side + ns - 1) / ns) <= (size_t)TRK_LDS_BUDGET) n_strips = ns;
  if (!n_strips) return false;
  g.S = (side + n_strips - 1) / n_strips;
  g.K = std::max(1, std::min(256 / (W * g.NR), g.S));
  lds_bytes = std::max(bytes(g.S), (size_t)g.K * W * g.NR * TRK_R * 8);
  return true;
}

// both entries: d_base null is the plain search around (0, 0)
int track_launch(const void* d_planes, int dtype, int n_t, int64_t plane_stride, int h, int w, int t_ref, const int32_t* d_beads,
                 int m, int half, int max_drift, const int32_t* d_base, int32_t* d_shift, double* d_score, void* d_sums,
                 void* d_fixed, void* stream) {
  // Exactness of the integer sums in float64 and of n * sum in the score's int64 reading: the largest term is
  // n * sum A B <= 9025 * (9025 * 65535^2) = 9025^2 * 65535^2 < 2^63, a single sum <= 9025 * 65535^2 < 2^46.
  if (!(max_drift >= 1 && max_drift <= TRK_MAX_DRIFT && half >= 1 && 2 * (int64_t)half + 1 <= TRK_MAX_SIDE &&
        2 * (int64_t)half + 1 + 2 * max_drift <= TRK_MAX_WINDOW && n_t >= 1 && t_ref >= 0 && t_ref < n_t && h > 0 && w > 0 &&
        m >= 0 && plane_stride >= 0 && (int64_t)m * n_t <= 0x7FFFFFFF))
    return MG_EINVAL;
  if (m == 0) return MG_OK;
  if (!d_planes || !d_beads || !d_shift || !d_score) return MG_EINVAL;
  hipStream_t s = mg_stream(stream);
  return mg_dispatch_pixel(dtype, [&](auto t) {
    using T = decltype(t);
    using Out = typename TrackTypes<T>::Out;
    TrackGeom g{n_t, h, w, t_ref, half, max_drift, plane_stride, 0, 0, 0, 0};
    size_t lds = 0;
    if (!track_layout((int)sizeof(typename TrackTypes<T>::L), g, lds)) return (int)MG_EINVAL;
    const dim3 grid((unsigned)((int64_t)m * n_t));
    if (d_base)
      hipLaunchKernelGGL((k_track<T, true>), grid, dim3(256), lds, s, (const T*)d_planes, g, d_beads, d_shift, d_score,
                         (Out*)d_sums, (Out*)d_fixed, d_base);
    else
      hipLaunchKernelGGL((k_track<T, false>), grid, dim3(256), lds, s, (const T*)d_planes, g, d_beads, d_shift, d_score,
                         (Out*)d_sums, (Out*)d_fixed, d_base);
    MG_CHECK_LAUNCH();
    return (int)MG_OK;
  });
}

}  // namespace

extern "C" int mg_track_beads(const void* d_planes, int dtype, int n_t, int64_t plane_stride, int h, int w, int t_ref,
                              const int32_t* d_beads, int m, int half, int max_drift, int32_t* d_shift, double* d_score,
                              void* d_sums, void* d_fixed, void* stream) {
  return track_launch(d_planes, dtype, n_t, plane_stride, h, w, t_ref, d_beads, m, half, max_drift, nullptr, d_shift, d_score,
                      d_sums, d_fixed, stream);
}

extern "C" int mg_track_beads_based(const void* d_planes, int dtype, int n_t, int64_t plane_stride, int h, int w, int t_ref,
                                    const int32_t* d_beads, int m, int half, int max_drift, const int32_t* d_base,
                                    int32_t* d_shift, double* d_score, void* d_sums, void* d_fixed, void* stream) {
  if (!d_base && m > 0) return MG_EINVAL;
  return track_launch(d_planes, dtype, n_t, plane_stride, h, w, t_ref, d_beads, m, half, max_drift, d_base, d_shift, d_score,
                      d_sums, d_fixed, stream);
}
