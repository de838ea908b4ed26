// Sub-pixel circle fit of every marker (mg_roi_refine_circles; not in the reference, which drops even the integer
// radius): a radial edge search along n_rays rays about the finder's circle, then a centred Kasa fit with one rejection
// round.  include/magnify_hip.h states the rules, tests/refine_ref.py restates them; float64 throughout, nothing
// contracted, no square root and no trigonometric function -- the directions come in as a table.
//
// One workgroup per (marker, time), three phases with a barrier between them:
//   samples  the n_rays * (4 reach + 1) bilinear values are dealt over the 256 lanes, one sample after the other along a
//            ray, and written to LDS as float64 (a sample outside the window is NaN: not finite, like a NaN pixel).  The
//            four taps of a sample are read where they lie: the annulus is a few hundred pixels of a window that the
//            finder has just written, neighbouring lanes read neighbouring samples of one ray -- the same or adjoining
//            cache lines -- and a staged bounding box would read the disk's inside, which no sample touches.
//   rays     lane k owns ray k: derivative, polarity vote, first arg-max, parabola vertex.  A ray's samples are 4 reach + 1
//            doubles apart, an odd number: the 32 lanes of a half wave read 32 different banks.  The votes are summed in
//            ascending k by every lane for itself (broadcast reads), which saves a barrier.
//   fit      the ray lanes form the terms of rules 7 and 8 and leave them in LDS as rows; each ordered sum is one row,
//            added up in ascending k by one lane -- the two or five sums of a step side by side in as many lanes --
//            so the serial part is n_rays dependent additions per step, not per sum.  Counts go through the barrier
//            (__syncthreads_count), the largest strength through a broadcast loop: neither depends on an order.
//
// Roofline: latency.  Per window 4 n_rays (4 reach + 1) taps, mostly cache hits; 56 bytes written.  The entry stands
// in mg_windows.h's frame (check, launch); the kernel streams no window and takes nothing else from it.
#include "mg_windows.h"

#include <cfloat>

namespace {

constexpr int NT = MG_WINDOW_THREADS;
constexpr int K_MAX = MG_REFINE_MAX_RAYS, REACH_MAX = MG_REFINE_MAX_REACH, SUB = MG_PROFILE_SUBPIXEL;
constexpr int J_MAX = 4 * REACH_MAX + 1;
static_assert(K_MAX <= NT, "one lane per ray");
static_assert((size_t)K_MAX * J_MAX * 8 + 12 * 1024 <= 64 * 1024, "the samples and the per-ray tables fit the default LDS");

enum { ST_OK = 0, ST_FEW = 1, ST_DEGENERATE = 2, ST_REACH = 3 };

struct RefineArgs {
  const void* roi;
  int64_t roi_stride_m, roi_stride_t;
  const int32_t* circle;
  int64_t circle_stride_m, circle_stride_t;
  const double* cs;
  int n_t, len, n_rays, reach, polarity, min_rays;
  double reject, min_strength;
  int32_t* info;
  double* fit;
};

__device__ __forceinline__ bool is_finite(double v) { return v - v == 0.0; }  // (inf - inf and NaN - NaN are NaN)

struct Circle {
  bool ok;
  double a, b, r2;
};

__device__ __forceinline__ double residual(double u, double v, const Circle& c) {
  const double da = u - c.a, db = v - c.b;
  return (da * da + db * db) - c.r2;
}

template <typename T>
__global__ __launch_bounds__(NT) void k_refine_circles(RefineArgs a) {
  extern __shared__ __attribute__((aligned(16))) double s_val[];  // [n_rays][J]
  __shared__ double s_cs[K_MAX][2], s_w[K_MAX], s_hi[K_MAX], s_lo[K_MAX];
  __shared__ double s_term[5][K_MAX + 1], s_sum[5];  // (+ 1: the five rows start on different banks)
  __shared__ uint8_t s_usable[K_MAX];

  const int g = (int)(blockIdx.x / (unsigned)a.n_t), t = (int)(blockIdx.x % (unsigned)a.n_t);
  const int64_t window = (int64_t)blockIdx.x;
  const int L = a.len, K = a.n_rays, reach = a.reach, J = 4 * reach + 1;
  const T* win = (const T*)a.roi + (int64_t)g * a.roi_stride_m + (int64_t)t * a.roi_stride_t;
  const int32_t* circle = a.circle + (int64_t)g * a.circle_stride_m + (int64_t)t * a.circle_stride_t;
  const double cy = (double)min(max(circle[0], MG_PROFILE_CENTRE_MIN), MG_PROFILE_CENTRE_MAX) / (double)SUB;
  const double cx = (double)min(max(circle[1], MG_PROFILE_CENTRE_MIN), MG_PROFILE_CENTRE_MAX) / (double)SUB;
  const double r = (double)min(max(circle[2], 0), MG_REFINE_MAX_RADIUS) / (double)SUB;
  const double rho0 = r - (double)reach;  // rho_j = rho0 + 0.5 j, exact: multiples of 1/16 below 2^11
  int j_lo = 0;
  while (rho0 + 0.5 * (double)j_lo < 0.0) ++j_lo;  // (<= 2 reach: rho_{2 reach} = r >= 0)
  const int first = j_lo + 1, last = J - 2;         // the derivative indices; first <= last
  const double nan = __longlong_as_double(0x7FF8000000000000ll);

  // ---- samples
  for (int i = threadIdx.x; i < 2 * K; i += NT) (&s_cs[0][0])[i] = a.cs[i];
  const double edge = (double)(L - 1);
  for (int i = threadIdx.x; i < K * J; i += NT) {
    const int k = i / J, j = i - k * J;
    if (j < j_lo) continue;  // never read
    const double c = a.cs[2 * k], s = a.cs[2 * k + 1], rho = rho0 + 0.5 * (double)j;
    const double y = cy + rho * s, x = cx + rho * c;
    double val = nan;
    if (y >= 0.0 && y < edge && x >= 0.0 && x < edge) {  // 0 <= floor, floor + 1 <= L - 1; a NaN direction is outside
      const double fly = floor(y), flx = floor(x);
      const double fy = y - fly, fx = x - flx;
      const T* p = win + (int64_t)(int)fly * L + (int)flx;
      const double w00 = (double)p[0], w01 = (double)p[1], w10 = (double)p[L], w11 = (double)p[L + 1];
      const double top = w00 * (1.0 - fx) + w01 * fx;
      const double bot = w10 * (1.0 - fx) + w11 * fx;
      val = top * (1.0 - fy) + bot * fy;
    }
    s_val[i] = val;
  }
  __syncthreads();

  // ---- rays: lane k owns ray k
  const int k = threadIdx.x;
  const double* ray = s_val + (k < K ? k : 0) * J;
  bool usable = k < K;
  if (k < K) {
    for (int j = j_lo; j < J; ++j) usable = usable && is_finite(ray[j]);
    double hi = 0.0, lo = 0.0;
    if (usable) {
      hi = ray[first + 1] - ray[first - 1], lo = -hi;
      for (int j = first + 1; j <= last; ++j) {
        const double d = ray[j + 1] - ray[j - 1];
        if (d > hi) hi = d;
        if (-d > lo) lo = -d;
      }
    }
    s_hi[k] = hi, s_lo[k] = lo, s_usable[k] = usable ? 1 : 0;
  }
  __syncthreads();
  int pol = a.polarity > 0 ? 1 : -1;
  if (a.polarity == 0) {  // the votes, in ascending k: every lane sums them for itself
    double pp = 0.0, pm = 0.0;
    for (int q = 0; q < K; ++q)
      if (s_usable[q]) pp = pp + s_hi[q], pm = pm + s_lo[q];
    pol = pp >= pm ? 1 : -1;
  }
  bool valid = false;
  double rho_k = nan, w_k = nan;
  if (usable) {
    const double sign = (double)pol;
    int js = first;
    double e0 = sign * (ray[first + 1] - ray[first - 1]);
    for (int j = first + 1; j <= last; ++j) {
      const double e = sign * (ray[j + 1] - ray[j - 1]);
      if (e > e0) e0 = e, js = j;
    }
    if (e0 > 0.0 && js != first && js != last) {
      const double em = sign * (ray[js] - ray[js - 2]), ep = sign * (ray[js + 2] - ray[js]);
      const double delta = (0.5 * (em - ep)) / ((em - 2.0 * e0) + ep);
      rho_k = (rho0 + 0.5 * (double)js) + 0.5 * delta;
      w_k = e0;
      valid = true;
    }
  }
  const double u = k < K ? rho_k * s_cs[k][0] : nan, v = k < K ? rho_k * s_cs[k][1] : nan;

  // ---- fit: the workgroup together.  Terms are formed by the ray lanes; every ordered sum is a row of s_term that ONE
  // lane adds up in ascending k -- the rows of a step side by side in as many lanes.  A ray outside the set adds +0.0,
  // which changes no sum: a sum starts at +0.0 and is never -0.0.
  if (k < K) s_w[k] = valid ? w_k : 0.0;
  __syncthreads();
  double wmax = 0.0;
  for (int q = 0; q < K; ++q) wmax = s_w[q] > wmax ? s_w[q] : wmax;
  const double gate = a.min_strength * wmax;
  bool kept = valid && w_k >= gate;
  const int n_valid = __syncthreads_count(valid);
  int n_kept = __syncthreads_count(kept);

  auto sums = [&](int rows) {  // s_sum[i] = the ordered sum of row i < rows; a barrier on either side
    __syncthreads();
    if ((int)threadIdx.x < rows) {
      const double* row = s_term[threadIdx.x];
      double s = 0.0;
      for (int q = 0; q < K; ++q) s = s + row[q];
      s_sum[threadIdx.x] = s;
    }
    __syncthreads();
  };
  auto fit_kept = [&]() {  // rule 7 over the kept rays; the same value in every lane
    const double n = (double)n_kept;
    if (k < K) s_term[0][k] = kept ? u : 0.0, s_term[1][k] = kept ? v : 0.0;
    sums(2);
    const double mu = s_sum[0] / n, mv = s_sum[1] / n;
    const double du = u - mu, dv = v - mv;
    const double z = du * du + dv * dv;
    if (k < K) {
      s_term[0][k] = kept ? du * du : 0.0, s_term[1][k] = kept ? du * dv : 0.0, s_term[2][k] = kept ? dv * dv : 0.0;
      s_term[3][k] = kept ? du * z : 0.0, s_term[4][k] = kept ? dv * z : 0.0;
    }
    sums(5);
    const double suu = s_sum[0], suv = s_sum[1], svv = s_sum[2], suz = s_sum[3], svz = s_sum[4];
    Circle c = {false, 0.0, 0.0, 0.0};
    const double det = suu * svv - suv * suv;
    if (!(det > 0.0)) return c;
    const double a1 = (0.5 * (suz * svv - svz * suv)) / det;
    const double b1 = (0.5 * (svz * suu - suz * suv)) / det;
    c.a = mu + a1, c.b = mv + b1;
    c.r2 = (a1 * a1 + b1 * b1) + (suu + svv) / n;
    c.ok = c.r2 > 0.0;
    return c;
  };

  int status = ST_OK;
  double out[5] = {nan, nan, nan, nan, nan};
  if (n_kept < a.min_rays) {  // (block-uniform, as every branch below: the lanes hold the same sums)
    status = ST_FEW;
  } else {
    Circle c = fit_kept();
    if (c.ok) {
      const double g = residual(u, v, c);
      const bool drop = kept && g * g > (4.0 * (a.reject * a.reject)) * c.r2;
      const int n_rest = n_kept - __syncthreads_count(drop);
      if (n_rest < n_kept && n_rest >= a.min_rays) {
        kept = kept && !drop;
        n_kept = n_rest;
        c = fit_kept();
      }
    }
    if (!c.ok) {
      status = ST_DEGENERATE;
    } else {
      const double n = (double)n_kept, g = residual(u, v, c);
      if (k < K) s_term[0][k] = kept ? g * g : 0.0, s_term[1][k] = kept ? w_k : 0.0;
      sums(2);
      const double msq = s_sum[0] / ((4.0 * c.r2) * n), mw = s_sum[1] / n;
      double lo = r - (double)reach;
      if (lo < 0.0) lo = 0.0;
      const double hi = r + (double)reach;
      if (!(is_finite(c.a) && is_finite(c.b) && is_finite(c.r2) && is_finite(msq) && is_finite(mw))) {
        status = ST_DEGENERATE;
      } else if (c.a * c.a + c.b * c.b > (double)reach * (double)reach || c.r2 < lo * lo || c.r2 > hi * hi) {
        status = ST_REACH;
      } else {
        out[0] = c.b, out[1] = c.a, out[2] = c.r2, out[3] = msq, out[4] = mw;
      }
    }
  }
  if (threadIdx.x != 0) return;
  int32_t* info = a.info + 4 * window;
  double* fit = a.fit + 5 * window;
  info[0] = status, info[1] = n_kept, info[2] = n_valid, info[3] = pol;
#pragma unroll
  for (int e = 0; e < 5; ++e) fit[e] = out[e];
}

}  // namespace

extern "C" int mg_roi_refine_circles(const void* d_roi, int dtype, int64_t roi_stride_m, int64_t roi_stride_t,
                                     const int32_t* d_circle, int64_t circle_stride_m, int64_t circle_stride_t,
                                     const double* d_cs, int n_rays, int m, int n_t, int roi_len, int reach, int polarity,
                                     double reject, double min_strength, int min_rays, int32_t* d_info, double* d_fit,
                                     void* stream) {
  if (!d_roi || !d_circle || !d_cs || !d_info || !d_fit) return MG_EINVAL;
  if (!mg_windows_check(m, 1, n_t, roi_len, MG_REFINE_MAX_LEN,
                        {roi_stride_m, roi_stride_t, circle_stride_m, circle_stride_t}))
    return MG_EINVAL;
  if (n_rays < 8 || n_rays > K_MAX || reach < 1 || reach > REACH_MAX || min_rays < 3 || min_rays > n_rays) return MG_EINVAL;
  if (polarity < -1 || polarity > 1) return MG_EINVAL;
  if (!(reject > 0.0) || !(reject <= DBL_MAX) || !(min_strength >= 0.0) || !(min_strength <= 1.0)) return MG_EINVAL;
  RefineArgs a = {d_roi, roi_stride_m, roi_stride_t, d_circle, circle_stride_m, circle_stride_t, d_cs, n_t,  roi_len,
                  n_rays, reach,       polarity,     min_rays, reject,          min_strength,    d_info, d_fit};
  const size_t lds = (size_t)n_rays * (4 * reach + 1) * sizeof(double);
  hipStream_t s = mg_stream(stream);
  return mg_windows_launch(dtype, m, n_t, [&](auto t, dim3 grid, dim3 block) {
    hipLaunchKernelGGL((k_refine_circles<decltype(t)>), grid, block, lds, s, a);
  });
}
