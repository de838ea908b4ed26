// Per-pixel linear unmixing (mg_roi_unmix_stats, mg_unmix_planes; not in the reference, whose identify_mrbles unmixes one
// mean per bead): at every pixel the channels are combined into lanthanide volumes v_k = sum_j matrix[k][j] x_j, left to
// right in float64 with nothing contracted, and into the ratios r_k = v_k / v_0.  tests/unmix_ref.py restates both
// entries in NumPy.
//
// mg_roi_unmix_stats: one workgroup per (marker, time).  The ingest pass reads the mask once and the used channels under
// it, counts and sums every derived value in registers (every thread its own pixels in the order it meets them, then
// shuffles and the four waves' partials as (0 + 1) + (2 + 3): no floating-point atomic, the same bits in every call)
// and leaves the n_ln volumes of the masked pixels in LDS -- where they are n_masked * n_ln * 8 bytes at most
// MG_UNMIX_LDS_KEY_BYTES.  A wave takes the slots of its step's pixels with one integer LDS add, so where a pixel lies
// in LDS depends on timing; nothing that is written out does: sums never come from LDS and a selection does not care
// for the order of its items.  The order statistics are the radix select of mg_select.h over the order-preserving keys
// of the kept volumes, the ratios formed from them on the way -- eight passes for sorted[lo], one more for
// sorted[lo + 1] (next_above; the walk over the fractions is order_pairs, both mg_select.h's).  A window with more
// masked pixels computes every value again from global memory in each pass, by the same operations, so the bits are the
// same.  The entry stands in mg_windows.h's frame (check, fractions, launch).
//
// mg_unmix_planes: a streaming kernel, four pixels a thread, one vector load per used channel and one float4 store per
// output plane where the planes' addresses allow, pixel by pixel otherwise and for the last hw % 4 pixels.
//
// Roofline: the planes kernel HBM (n_k sizeof(T) bytes read and 4 n_out written per pixel).  The statistics read
// L*L + n_fg n_k sizeof(T) bytes per window at most and then make 8 passes over LDS per selected rank: LDS and barrier
// latency, not memory, set their time.
#include "mg_planes.h"
#include "mg_windows.h"

namespace {

constexpr int NT = MG_WINDOW_THREADS, WV = MG_WINDOW_WAVES;
constexpr int K_MAX = MG_UNMIX_MAX_CHANNELS, LN_MAX = MG_UNMIX_MAX_LN, Q_MAX = MG_UNMIX_MAX_Q, D_MAX = 2 * LN_MAX - 1;
constexpr int GROUP = 4;  // channels whose loads are issued before the first is used

// What both kernels know of the unmixing: the table, the used channels, the constant offsets (planes) and the fractions
// (statistics).  A kernel argument: its entries are read with uniform indices, as scalar loads.
struct Unmix {
  double w[LN_MAX][K_MAX], off[K_MAX], q[Q_MAX];
  int ch[K_MAX];
  int n_k, n_ln;
};

// The per-pixel arithmetic of both kernels: channel j's term of one volume, v = w x_0 for the first channel, then
// v = v + w x_j: the product rounded, then the sum (-ffp-contract=off); taken left to right by the callers' loops.
__device__ __forceinline__ void unmix_term(double w, double x, bool first, double& v) {
  const double term = w * x;
  v = first ? term : v + term;
}
// ... of every volume
__device__ __forceinline__ void unmix_step(const Unmix& u, int j, double x, double (&v)[LN_MAX]) {
#pragma unroll
  for (int k = 0; k < LN_MAX; ++k)
    if (k < u.n_ln) unmix_term(u.w[k][j], x, j == 0, v[k]);
}

inline int64_t keep_cap(int n_ln) { return MG_UNMIX_LDS_KEY_BYTES / (8 * (int64_t)n_ln); }

// One workgroup per (marker, time).  `cap`: the masked pixels whose volumes fit the budget; `kept` = min(n, cap): the
// stride of s_vol, double[n_ln][kept] of dynamic LDS.
template <typename T>
__global__ __launch_bounds__(NT) void k_unmix_stats(const T* __restrict__ d_roi, const uint8_t* __restrict__ d_mask,
                                                    int64_t mask_stride_m, int64_t mask_stride_t,
                                                    const double* __restrict__ d_offset, Unmix u, int n_q, int n_c, int n_t,
                                                    int n, int cap, int kept, int32_t* __restrict__ d_count,
                                                    double* __restrict__ d_sum, double* __restrict__ d_order) {
  extern __shared__ __attribute__((aligned(16))) double s_vol[];
  __shared__ uint32_t hist[256];
  __shared__ double s_off[K_MAX], s_psum[WV][D_MAX];
  __shared__ int s_pcnt[WV][D_MAX], s_count[D_MAX], s_pick[2], s_next;
  const int g = (int)(blockIdx.x / (unsigned)n_t), t = (int)(blockIdx.x % (unsigned)n_t);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int n_k = u.n_k, n_ln = u.n_ln, D = 2 * n_ln - 1;
  const uint8_t* mask = d_mask ? d_mask + (int64_t)g * mask_stride_m + (int64_t)t * mask_stride_t : nullptr;
  const int64_t first = (int64_t)g * n_c * n_t + t;  // the window of channel c is first + c * n_t

  for (int i = threadIdx.x; i < 256; i += NT) hist[i] = 0u;  // (as select_kth wants it)
  for (int j = 0; j < n_k; ++j)  // (u is read with uniform indices only)
    if ((int)threadIdx.x == j) s_off[j] = d_offset ? d_offset[first + (int64_t)u.ch[j] * n_t] : 0.0;
  if (threadIdx.x == 0) s_next = 0;
  __syncthreads();

  // x_j of pixel p (< n); its volumes, GROUP channels' loads in flight
  auto pixel = [&](int j, int p) { return (double)d_roi[(first + (int64_t)u.ch[j] * n_t) * n + p] - s_off[j]; };
  auto volumes = [&](int p, double (&v)[LN_MAX]) {
    for (int j0 = 0; j0 < n_k; j0 += GROUP) {
      double x[GROUP];
#pragma unroll
      for (int e = 0; e < GROUP; ++e)
        x[e] = j0 + e < n_k ? pixel(j0 + e, p) : 0.0;
#pragma unroll
      for (int e = 0; e < GROUP; ++e)
        if (j0 + e < n_k) unmix_step(u, j0 + e, x[e], v);
    }
  };

  // ---- ingest: counts and sums in registers, the volumes of the masked pixels into LDS while they fit
  int vcnt[LN_MAX] = {}, rcnt[LN_MAX] = {};
  double vsum[LN_MAX] = {}, rsum[LN_MAX] = {};
  for (int base = 0; base < n; base += NT) {  // block-uniform trip count
    const int p = base + threadIdx.x;
    const bool mk = p < n && (!mask || mask[p] != 0);
    if (!__ballot(mk)) continue;  // wave-uniform: none of these 64 pixels is under the mask
    double v[LN_MAX] = {};
    volumes(min(p, n - 1), v);
    const int incl = mg_wave_scan_incl_i32(mk ? 1 : 0), total = __builtin_amdgcn_readlane(incl, 63);
    int at = 0;
    if (lane == 0) at = atomicAdd(&s_next, total);
    at = __builtin_amdgcn_readfirstlane(at);
    const int slot = at + incl - 1;
    if (!mk) continue;
#pragma unroll
    for (int k = 0; k < LN_MAX; ++k) {
      if (k >= n_ln) continue;
      if (slot < cap) s_vol[(int64_t)k * kept + slot] = v[k];
      if (v[k] == v[k]) ++vcnt[k], vsum[k] += v[k];
      if (k > 0) {
        const double r = v[k] / v[0];
        if (r == r) ++rcnt[k], rsum[k] += r;
      }
    }
  }
  // the waves' partials, then derived value d by thread d
#pragma unroll
  for (int k = 0; k < LN_MAX; ++k) {
    if (k >= n_ln) continue;  // (uniform)
    const int c = mg_wave_sum_i32(vcnt[k]), rc = mg_wave_sum_i32(rcnt[k]);
    const double s = mg_wave_sum_f64(vsum[k]), rs = mg_wave_sum_f64(rsum[k]);
    if (lane == 0) {
      s_pcnt[wave][k] = c, s_psum[wave][k] = s;
      if (k > 0) s_pcnt[wave][n_ln - 1 + k] = rc, s_psum[wave][n_ln - 1 + k] = rs;
    }
  }
  __syncthreads();
  const int64_t out = (int64_t)blockIdx.x * D;
  if (threadIdx.x < D) {
    const int d = threadIdx.x;
    const int c = (s_pcnt[0][d] + s_pcnt[1][d]) + (s_pcnt[2][d] + s_pcnt[3][d]);
    s_count[d] = c;
    d_count[out + d] = c;
    d_sum[out + d] = c ? (s_psum[0][d] + s_psum[1][d]) + (s_psum[2][d] + s_psum[3][d]) : 0.0;
  }
  __syncthreads();
  if (n_q == 0) return;

  // ---- the order statistics: over the kept volumes, or over the window's pixels in global memory
  const int n_masked = s_next;
  const bool in_lds = n_masked <= cap;  // block-uniform
  for (int d = 0; d < D; ++d) {
    const bool ratio = d >= n_ln;
    const int k = ratio ? d - n_ln + 1 : d;
    // the key of item i: of kept pixel i, or of pixel i of the window -- false where it has none (masked out, NaN)
    auto kept_key = [&](int i, uint64_t* key) {
      double val = s_vol[(int64_t)k * kept + i];
      if (ratio) val = val / s_vol[i];
      return median_key<double>::key(val, key);
    };
    auto pixel_key = [&](int p, uint64_t* key) {  // (rows k and 0 only: an array indexed by k would go to scratch)
      if (mask && !mask[p]) return false;
      double val = 0.0, v0 = 0.0;
      for (int j = 0; j < n_k; ++j) {
        const double x = pixel(j, p);
        unmix_term(u.w[k][j], x, j == 0, val);
        if (ratio) unmix_term(u.w[0][j], x, j == 0, v0);
      }
      if (ratio) val = val / v0;
      return median_key<double>::key(val, key);
    };
    auto select = [&](int rank) -> uint64_t {
      if (in_lds) return select_kth<uint64_t, 8>(n_masked, kept_key, rank, hist, s_pick);
      return select_kth<uint64_t, 8>(n, pixel_key, rank, hist, s_pick);
    };
    auto next = [&](uint64_t below, int rank) -> uint64_t {
      return next_above<uint64_t>(below, rank, [&](auto see) {
        uint64_t key;
        if (in_lds) {
          for (int i = threadIdx.x; i < n_masked; i += NT)
            if (kept_key(i, &key)) see(key);
        } else {
          for (int p = threadIdx.x; p < n; p += NT)
            if (pixel_key(p, &key)) see(key);
        }
      });
    };
    // sorted[lo], sorted[hi] of every q -- NaN where the derived value has no item -- as k_masked_stats has them
    order_pairs<double>(s_count[d], u.q, n_q, select, next, d_order + (out + d) * n_q * 2);
  }
}

// Four pixels of one plane as one load, where the plane starts on 4 sizeof(T) bytes.
template <typename T>
struct alignas(4 * sizeof(T)) Quad {
  T px[4];
};

// blockIdx.y walks the timepoints, the workgroups of a row the groups of four pixels of a plane.
template <typename T>
__global__ __launch_bounds__(256) void k_unmix_planes(const T* __restrict__ d_src, int64_t chan_stride, int64_t time_stride,
                                                      Unmix u, int ratios, int n_t, int64_t hw, float* __restrict__ d_dst) {
  const int n_k = u.n_k, n_ln = u.n_ln, n_out = ratios ? 2 * n_ln - 1 : n_ln;
  const int64_t quads = (hw + 3) / 4;
  MG_FOR_BLOCK_PLANES(t, n_t) {
    const T* src = d_src + t * time_stride;
    float* dst = d_dst + t * hw;  // output plane o of this timepoint is dst + o * n_t * hw
    bool wide = true;  // block-uniform: every plane this timepoint reads and writes starts on a vector
    for (int j = 0; j < n_k; ++j) wide &= (reinterpret_cast<uintptr_t>(src + u.ch[j] * chan_stride) % sizeof(Quad<T>)) == 0;
    for (int o = 0; o < n_out; ++o) wide &= (reinterpret_cast<uintptr_t>(dst + (int64_t)o * n_t * hw) & 15) == 0;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < quads; i += (int64_t)gridDim.x * 256) {
      const int64_t p0 = 4 * i;
      const int cnt = (int)min((int64_t)4, hw - p0);
      const bool whole = wide && cnt == 4;
      double v[4][LN_MAX] = {};
      for (int j = 0; j < n_k; ++j) {
        const T* plane = src + u.ch[j] * chan_stride + p0;
        Quad<T> raw = {};
        if (whole) {
          raw = *reinterpret_cast<const Quad<T>*>(plane);
        } else {
#pragma unroll
          for (int e = 0; e < 4; ++e)
            if (e < cnt) raw.px[e] = plane[e];
        }
#pragma unroll
        for (int e = 0; e < 4; ++e) unmix_step(u, j, (double)raw.px[e] - u.off[j], v[e]);
      }
      auto put = [&](int o, const float (&f)[4]) {
        float* at = dst + (int64_t)o * n_t * hw + p0;
        if (whole) {
          *reinterpret_cast<float4*>(at) = make_float4(f[0], f[1], f[2], f[3]);
        } else {
#pragma unroll
          for (int e = 0; e < 4; ++e)
            if (e < cnt) at[e] = f[e];
        }
      };
#pragma unroll
      for (int k = 0; k < LN_MAX; ++k) {
        if (k >= n_ln) continue;
        const float f[4] = {(float)v[0][k], (float)v[1][k], (float)v[2][k], (float)v[3][k]};
        put(k, f);
        if (ratios && k > 0) {
          const float r[4] = {(float)(v[0][k] / v[0][0]), (float)(v[1][k] / v[1][0]), (float)(v[2][k] / v[2][0]),
                              (float)(v[3][k] / v[3][0])};
          put(n_ln - 1 + k, r);
        }
      }
    }
  }
}

// The host arguments both entries share, checked and copied: false for what they refuse.
bool unmix_table(const int* channels, int n_k, const double* matrix, int n_ln, int n_c, Unmix* u) {
  if (!channels || !matrix || n_k < 1 || n_k > K_MAX || n_ln < 1 || n_ln > LN_MAX) return false;
  *u = Unmix{};
  u->n_k = n_k, u->n_ln = n_ln;
  for (int j = 0; j < n_k; ++j) {
    if (channels[j] < 0 || channels[j] >= n_c) return false;
    for (int i = 0; i < j; ++i)
      if (channels[i] == channels[j]) return false;
    u->ch[j] = channels[j];
  }
  for (int k = 0; k < n_ln; ++k)
    for (int j = 0; j < n_k; ++j) {
      if (!std::isfinite(matrix[k * n_k + j])) return false;
      u->w[k][j] = matrix[k * n_k + j];
    }
  return true;
}

}  // namespace

extern "C" int mg_roi_unmix_keys_in_lds(int n_ln, int64_t n_masked) {
  if (n_ln < 1 || n_ln > LN_MAX || n_masked < 0) return MG_EINVAL;
  return (int)(n_masked <= keep_cap(n_ln));
}

extern "C" int mg_roi_unmix_stats(const void* d_roi, int dtype, const uint8_t* d_mask, int64_t mask_stride_m,
                                  int64_t mask_stride_t, int m, int n_c, int n_t, int roi_len, const int* channels, int n_k,
                                  const double* matrix, int n_ln, const double* d_offset, const double* q, int n_q,
                                  int32_t* d_count, double* d_sum, double* d_order, void* stream) {
  if (!d_roi || !d_count || !d_sum) return MG_EINVAL;
  if (!mg_windows_check(m, n_c, n_t, roi_len, MG_UNMIX_MAX_LEN, {mask_stride_m, mask_stride_t})) return MG_EINVAL;
  Unmix u;
  if (!unmix_table(channels, n_k, matrix, n_ln, n_c, &u)) return MG_EINVAL;
  if (!mg_fractions(q, n_q, Q_MAX, u.q) || (n_q > 0 && !d_order)) return MG_EINVAL;
  if ((int64_t)m * n_t * (2 * n_ln - 1) > INT32_MAX) return MG_EINVAL;
  const int n = roi_len * roi_len, cap = (int)keep_cap(n_ln), kept = n < cap ? n : cap;
  hipStream_t s = mg_stream(stream);
  return mg_windows_launch(dtype, m, n_t, [&](auto t, dim3 grid, dim3 block) {
    typedef decltype(t) T;
    hipLaunchKernelGGL(k_unmix_stats<T>, grid, block, (size_t)kept * n_ln * 8, s, (const T*)d_roi, d_mask, mask_stride_m,
                       mask_stride_t, d_offset, u, n_q, n_c, n_t, n, cap, kept, d_count, d_sum, d_order);
  });
}

extern "C" int mg_unmix_planes(const void* d_src, int dtype, int64_t chan_stride, int64_t time_stride, int n_c, int n_t,
                               int h, int w, const int* channels, int n_k, const double* matrix, int n_ln,
                               const double* offset, int ratios, float* d_dst, void* stream) {
  if (!d_src || !d_dst || (ratios != 0 && ratios != 1)) return MG_EINVAL;
  if (n_c <= 0 || n_t <= 0 || h <= 0 || w <= 0 || chan_stride < 0 || time_stride < 0) return MG_EINVAL;
  if (mg_planes_check(dtype, n_t, h, w, {d_src}) != MG_PLANES_RUN) return MG_EINVAL;
  if (reinterpret_cast<uintptr_t>(d_dst) % sizeof(float)) return MG_EINVAL;
  Unmix u;
  if (!unmix_table(channels, n_k, matrix, n_ln, n_c, &u)) return MG_EINVAL;
  for (int j = 0; j < n_k; ++j) {
    if (offset && !std::isfinite(offset[j])) return MG_EINVAL;
    u.off[j] = offset ? offset[j] : 0.0;
  }
  if ((int64_t)n_t * (2 * n_ln - 1) > INT32_MAX) return MG_EINVAL;
  const int64_t hw = (int64_t)h * w, quads = (hw + 3) / 4;
  hipStream_t s = mg_stream(stream);
  return mg_dispatch_pixel(dtype, [&](auto t) {
    typedef decltype(t) T;
    hipLaunchKernelGGL(k_unmix_planes<T>, mg_plane_grid((quads + 255) / 256, n_t, 0, MG_UNMIX_PLANES_WALK_PER_PLANE), dim3(256), 0, s,
                       (const T*)d_src, chan_stride, time_stride, u, ratios, n_t, hw, d_dst);
    MG_CHECK_LAUNCH();
    return MG_OK;
  });
}
