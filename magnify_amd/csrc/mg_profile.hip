// Radial intensity profiles of already gathered ROI windows (mg_roi_radial_profile; not in the reference): per
// (marker, channel, time) and ring k the count, the sum and the sum of squares of the pixels whose distance d from the
// window's centre satisfies edges[k] <= d < edges[k + 1], everything in integers of 1 / MG_PROFILE_SUBPIXEL pixel.
//
// One workgroup per (marker, time) walks the windows of all channels: ring membership depends on (marker, time) only,
// so the first channel's pass keeps, where the window has at most KEEP_BYTES pixels, one byte per pixel in LDS -- the
// ring, or NO_RING where the pixel has none -- and the later channels compute no distance.  The windows are
// ingested as in k_masked_stats: a pass is a body of mg_windows.h's walk_chunks (16-byte chunks, IN_FLIGHT steps of
// loads issued before the first is worked on), and the entry stands in that header's frame (check, launch).
//
// Integer pixels: count, sum and sum of squares go to the workgroup's table with integer LDS atomics -- exact, and
// integer addition does not care for the order.  Float pixels: no atomic touches a float.  Of every lane's chunk the
// j-th pixels form, in lane order, a walk along the rows with stride VW; inside one row and on one side of the centre
// column the ring is monotone, so pixels with the same (row, side, ring) are neighbouring lanes: a segmented DPP scan
// folds each such run, its last lane adds the run's sums to the wave's own slots, the runs of one (row, side) -- all of
// different rings -- in one instruction, one (row, side) after the other.  The four waves' slots are added 0 + 1 + 2 +
// 3.  The order of every float addition is therefore fixed by the launch shape: every call gives the same bits.  A step
// in which no lane has a pixel under the mask is skipped by the whole wave.
//
// Roofline: HBM.  Per window L*L*sizeof(T) bytes read, the mask's L*L once per (marker, time); 20 n_rings bytes written.
#include "mg_windows.h"

namespace {

constexpr int NT = MG_WINDOW_THREADS, WV = MG_WINDOW_WAVES;
constexpr int R_MAX = MG_PROFILE_MAX_RINGS, SUB = MG_PROFILE_SUBPIXEL;
constexpr int KEEP_BYTES = 16384;    // ring bytes kept in LDS for the later channels: windows up to 128 x 128
constexpr uint32_t NO_RING = 255u;   // > any ring index
constexpr int NO_KEY = 0x7FFFFFFF;   // the run key of a pixel without a ring
static_assert(R_MAX <= 128, "a ring index is 7 bits of a run key and a byte below NO_RING");

// The squared edges, and e0 / width > 0 where the edges are e0 + k * width (the square-root path).
struct Edges {
  uint32_t e2[R_MAX + 1];
  int e0, width;
};

// What a pass knows of its window's geometry.  e2 points into LDS.
struct Geo {
  const uint32_t* e2;
  int cy, cx, len, n_rings, e0, width;
  float inv_width, inv_len;
};

// The ring of squared distance d2 (<= 2^31 inside a window: mg_roi_radial_profile's limits), NO_RING where it has none.
// Uniform edges: the candidate floor((sqrt(d2) - e0) / width) in float32 is off by at most one (the error of the
// conversion, of v_sqrt_f32 and of the product stays below 0.02 ring widths), and one exact comparison with the
// squares of its two edges -- both <= MG_PROFILE_MAX_EDGE: 32 bits hold them -- settles it.  Otherwise the largest k < n_rings
// with e2[k] <= d2, by bisection over the table.
__device__ __forceinline__ uint32_t ring_of(const Geo& g, uint32_t d2) {
  if (g.width > 0) {
    const float f = __builtin_amdgcn_sqrtf((float)d2);
    int k = (int)((f - (float)g.e0) * g.inv_width);
    k = min(max(k, 0), g.n_rings - 1);
    const uint32_t lo = (uint32_t)(g.e0 + k * g.width), hi = lo + (uint32_t)g.width;
    k += d2 < lo * lo ? -1 : d2 >= hi * hi ? 1 : 0;
    return (k < 0 || k >= g.n_rings) ? NO_RING : (uint32_t)k;
  }
  int k = 0;
#pragma unroll
  for (int step = R_MAX / 2; step >= 1; step >>= 1) {
    const int t = k + step;
    if (t < g.n_rings && d2 >= g.e2[t]) k = t;
  }
  return (d2 < g.e2[0] || d2 >= g.e2[g.n_rings]) ? NO_RING : (uint32_t)k;
}

__device__ __forceinline__ uint32_t dist2(const Geo& g, int row, int col) {
  const uint32_t dy = (uint32_t)(row * SUB - g.cy), dx = (uint32_t)(col * SUB - g.cx);  // (squares modulo 2^32)
  return dy * dy + dx * dx;
}

// The tables of a workgroup.  Integer pixels: one exact table.  Float pixels: {sum, sum of squares} per wave and ring.
template <typename T, bool INTEGER = std::is_integral<T>::value>
struct Slots;
template <typename T>
struct Slots<T, true> {
  unsigned long long sum[R_MAX], sq[R_MAX];
};
template <typename T>
struct Slots<T, false> {
  double m[WV][R_MAX][2];
};

template <int CTRL, int ROWS>
__device__ __forceinline__ int dpp_key(int key) {  // lanes without a source keep -1: no key
  return __builtin_amdgcn_update_dpp(-1, key, CTRL, ROWS, 0xF, false);
}
template <int CTRL, int ROWS>
__device__ __forceinline__ double dpp_f64(double v) {  // lanes without a source get 0.0
  const long long b = __double_as_longlong(v);
  const int lo = __builtin_amdgcn_update_dpp(0, (int)(uint32_t)b, CTRL, ROWS, 0xF, false);
  const int hi = __builtin_amdgcn_update_dpp(0, (int)(uint32_t)((unsigned long long)b >> 32), CTRL, ROWS, 0xF, false);
  return __longlong_as_double((long long)(((unsigned long long)(uint32_t)hi << 32) | (uint32_t)lo));
}
template <int CTRL, int ROWS>
__device__ __forceinline__ void seg_step(int key, double& a, double& b) {
  const int from = dpp_key<CTRL, ROWS>(key);
  const double au = dpp_f64<CTRL, ROWS>(a), bu = dpp_f64<CTRL, ROWS>(b);
  if (from == key) a += au, b += bu;
}
// Inclusive scan of (a, b) inside every run of equal keys (equal keys are neighbouring lanes): the steps of
// mg_wave_scan_incl_i32, each taken only where the source lane has the same key -- and then every lane between has.
__device__ __forceinline__ void seg_scan(int key, double& a, double& b) {
  seg_step<0x111, 0xF>(key, a, b);
  seg_step<0x112, 0xF>(key, a, b);
  seg_step<0x114, 0xF>(key, a, b);
  seg_step<0x118, 0xF>(key, a, b);
  seg_step<0x142, 0xA>(key, a, b);
  seg_step<0x143, 0xC>(key, a, b);
}

// One window.  MASKED: `mask` is the window's mask in global memory, else there is none.  KEPT: the ring of every pixel
// is read from `keep` (LDS), where an earlier pass left it; else it is computed, and left there if `keep` is not null.
// The kept byte is the ring the geometry gives, whatever the mask says: a pixel that is masked out or NaN stays in its
// run with nothing to add, so the pixels of one (row, side, ring) stay neighbours.
template <typename T, int VW, bool MASKED, bool KEPT>
__device__ __forceinline__ void pass(const T* __restrict__ v, const uint8_t* __restrict__ mask, int n, const Geo& g,
                                     uint8_t* keep, uint32_t* s_cnt, Slots<T>& acc) {
  constexpr bool INTEGER = std::is_integral<T>::value;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  walk_chunks<T, VW, MASKED>(v, mask, n, [&](const RawChunk<T, VW>& raw, int c, const WaveRun& run) {
    // (wave-uniform: nothing of these 64 chunks is under the mask, and no ring byte is owed to a later channel)
    if ((KEPT || !keep) && !__ballot((raw.mw[0] | raw.mw[1] | raw.mw[2] | raw.mw[3]) != 0u)) return;
    const int end = run.end, p0 = c * VW;  // (< 2^24: a float holds it)
    int row = (int)((float)p0 * g.inv_len), col = p0 - row * g.len;
    if (col < 0) --row, col += g.len;
    if (col >= g.len) ++row, col -= g.len;
    uint32_t rings[4] = {};
    const bool whole = VW > 1 && c < end && (c + 1) * VW <= n;
    if (KEPT && whole) load_bytes<VW>(keep + p0, rings);
#pragma unroll
    for (int j = 0; j < VW; ++j) {
      const bool inside = c < end && p0 + j < n;  // (beyond `end` lie another wave's pixels)
      uint32_t ring = NO_RING;
      if (KEPT) {
        if (whole) ring = (rings[j >> 2] >> (8 * (j & 3))) & 0xFFu;
        else if (inside) ring = keep[p0 + j];
      } else if (inside) {
        ring = ring_of(g, dist2(g, row, col));
        if (keep) keep[p0 + j] = (uint8_t)ring;
      }
      const T x = raw.px[j];
      const bool ok = ring != NO_RING && raw.under_mask(j) && x == x;
      if constexpr (INTEGER) {
        if (ok) {
          atomicAdd(&s_cnt[ring], 1u);
          atomicAdd(&acc.sum[ring], (unsigned long long)x);
          atomicAdd(&acc.sq[ring], (unsigned long long)((uint32_t)x * (uint32_t)x));
        }
      } else {
        if (ok) atomicAdd(&s_cnt[ring], 1u);
        if (!__ballot(ok)) {  // wave-uniform: 64 times + 0.0, which changes no slot (a slot is never -0.0)
          if (++col == g.len) col = 0, ++row;
          continue;
        }
        double a = ok ? (double)x : 0.0, b = a * a;
        const int key = ring == NO_RING ? NO_KEY : (int)((uint32_t)row << 8 | (col * SUB >= g.cx ? 128u : 0u) | ring);
        seg_scan(key, a, b);
        const int next = __shfl_down(key, 1);  // (by every lane, before any condition: a lane that sits out returns 0)
        const bool last = key != NO_KEY && (lane == 63 || next != key);
        unsigned long long pending = __ballot(last);
        while (pending) {  // wave-uniform: the runs of the first pending lane's (row, side), all of different rings
          const int side = __builtin_amdgcn_readlane(key, __ffsll((long long)pending) - 1) >> 7;
          const bool now = last && (key >> 7) == side;
          if (now) {
            double* s = acc.m[wave][key & 127];
            s[0] += a, s[1] += b;
          }
          pending &= ~__ballot(now);
        }
      }
      if (++col == g.len) col = 0, ++row;
    }
  });
}

template <typename T>
__global__ __launch_bounds__(NT) void k_radial_profile(const T* __restrict__ d_roi, const uint8_t* __restrict__ d_mask,
                                                       int64_t mask_stride_m, int64_t mask_stride_t,
                                                       const int32_t* __restrict__ d_centre, int64_t centre_stride_m,
                                                       int64_t centre_stride_t, Edges edges, int n_rings, int n_c, int n_t,
                                                       int len, int kept, int32_t* __restrict__ d_count,
                                                       double* __restrict__ d_moments) {
  constexpr bool INTEGER = std::is_integral<T>::value;
  extern __shared__ __attribute__((aligned(16))) unsigned char s_keep[];  // `kept`: n ring bytes
  __shared__ uint32_t s_e2[R_MAX + 1], s_cnt[R_MAX];
  __shared__ Slots<T> s_acc;
  const int g_ = (int)(blockIdx.x / (unsigned)n_t), t = (int)(blockIdx.x % (unsigned)n_t), n = len * len;
  auto clear = [&](int r) {
    s_cnt[r] = 0u;
    if constexpr (INTEGER) {
      s_acc.sum[r] = 0ull, s_acc.sq[r] = 0ull;
    } else {
#pragma unroll
      for (int w = 0; w < WV; ++w) s_acc.m[w][r][0] = 0.0, s_acc.m[w][r][1] = 0.0;
    }
  };
  for (int i = threadIdx.x; i <= n_rings; i += NT) s_e2[i] = edges.e2[i];
  if (threadIdx.x < R_MAX) clear(threadIdx.x);
  const int32_t* centre = d_centre + (int64_t)g_ * centre_stride_m + (int64_t)t * centre_stride_t;
  Geo geo;
  geo.e2 = s_e2;
  geo.cy = min(max(centre[0], MG_PROFILE_CENTRE_MIN), MG_PROFILE_CENTRE_MAX);
  geo.cx = min(max(centre[1], MG_PROFILE_CENTRE_MIN), MG_PROFILE_CENTRE_MAX);
  geo.len = len, geo.n_rings = n_rings, geo.e0 = edges.e0, geo.width = edges.width;
  geo.inv_width = edges.width > 0 ? 1.0f / (float)edges.width : 0.0f, geo.inv_len = 1.0f / (float)len;
  const uint8_t* mask = d_mask ? d_mask + (int64_t)g_ * mask_stride_m + (int64_t)t * mask_stride_t : nullptr;
  __syncthreads();

  for (int ch = 0; ch < n_c; ++ch) {  // block-uniform throughout
    const int64_t window = ((int64_t)g_ * n_c + ch) * n_t + t;
    const T* v = d_roi + window * n;
    uint8_t* keep = kept ? s_keep : nullptr;
    const bool wide = window_is_wide(v, mask);
    auto walk = [&](auto masked, auto kept_) {
      with_chunk_width<T>(wide, [&](auto vw) {
        pass<T, decltype(vw)::value, decltype(masked)::value, decltype(kept_)::value>(v, mask, n, geo, keep, s_cnt, s_acc);
      });
    };
    if (kept && ch > 0) {
      if (mask) walk(std::true_type{}, std::true_type{});
      else walk(std::false_type{}, std::true_type{});
    } else {
      if (mask) walk(std::true_type{}, std::false_type{});
      else walk(std::false_type{}, std::false_type{});
    }
    __syncthreads();
    if (threadIdx.x < n_rings) {
      const int r = threadIdx.x;
      const int64_t at = window * n_rings + r;
      d_count[at] = (int32_t)s_cnt[r];
      if constexpr (INTEGER) {
        d_moments[2 * at] = (double)s_acc.sum[r], d_moments[2 * at + 1] = (double)s_acc.sq[r];
      } else {
#pragma unroll
        for (int e = 0; e < 2; ++e)
          d_moments[2 * at + e] = ((s_acc.m[0][r][e] + s_acc.m[1][r][e]) + s_acc.m[2][r][e]) + s_acc.m[3][r][e];
      }
      clear(r);
    }
    __syncthreads();  // (the ring bytes of the first pass are in place for the others behind the first of these)
  }
}

}  // namespace

extern "C" int mg_roi_radial_profile(const void* d_roi, int dtype, const uint8_t* d_mask, int64_t mask_stride_m,
                                     int64_t mask_stride_t, const int32_t* d_centre, int64_t centre_stride_m,
                                     int64_t centre_stride_t, const int32_t* edges, int n_rings, int m, int n_c, int n_t,
                                     int roi_len, int32_t* d_count, double* d_moments, void* stream) {
  if (!d_roi || !d_centre || !edges || !d_count || !d_moments) return MG_EINVAL;
  if (!mg_windows_check(m, n_c, n_t, roi_len, MG_PROFILE_MAX_LEN,
                        {mask_stride_m, mask_stride_t, centre_stride_m, centre_stride_t}))
    return MG_EINVAL;
  if (n_rings < 1 || n_rings > R_MAX) return MG_EINVAL;
  if (edges[0] < 0 || edges[n_rings] > MG_PROFILE_MAX_EDGE) return MG_EINVAL;
  Edges e = {};
  e.e0 = edges[0], e.width = edges[1] - edges[0];
  for (int k = 0; k <= n_rings; ++k) {
    if (k > 0 && edges[k] <= edges[k - 1]) return MG_EINVAL;
    if (k > 0 && edges[k] - edges[k - 1] != e.width) e.width = 0;
    e.e2[k] = (uint32_t)edges[k] * (uint32_t)edges[k];
  }
  const int n = roi_len * roi_len, kept = n_c > 1 && n <= KEEP_BYTES;
  hipStream_t s = mg_stream(stream);
  return mg_windows_launch(dtype, m, n_t, [&](auto t, dim3 grid, dim3 block) {
    typedef decltype(t) T;
    hipLaunchKernelGGL(k_radial_profile<T>, grid, block, kept ? (size_t)((n + 15) & ~15) : 0, s, (const T*)d_roi, d_mask,
                       mask_stride_m, mask_stride_t, d_centre, centre_stride_m, centre_stride_t, e, n_rings, n_c, n_t,
                       roi_len, kept, d_count, d_moments);
  });
}
