// roi.where(mask).{sum, mean, std, var, min, max, count, quantile}(dim=[roi_y, roi_x]) of an already gathered roi
// (README.md:21-22, identify.py:76-80, filter.py:20-22): one workgroup per (marker, channel-time) reads the window and
// its mask ONCE from global memory, reduces count / sum / min / max on the way in and keeps the keys of the surviving
// pixels in LDS; the squared deviations and every order statistic asked for then run out of LDS.  The masked median
// (mg_roi_masked_median: numpy's nanmedian) is the same kernel in its median mode: the middle ranks, nothing else.
//
// Roofline: HBM.  Per window L*L*(sizeof(T) + 1) bytes read, 4 + 32 + 16 n_q bytes written.
#include "mg_select.h"

namespace {

constexpr int NT = MG_SELECT_THREADS, WV = NT / 64;
static_assert(WV == MG_FOLD_WAVES, "mg_block_fold folds four waves");
constexpr double QNAN = __builtin_nan("");

struct StatsQ {
  double q[MG_ROISTATS_MAX_Q];
};

// Do the keys of a window fit the LDS budget?  (n = roi_len^2 pixels, key_bytes = 4 or 8)
inline bool keys_fit(int64_t n, int key_bytes) { return n * key_bytes <= MG_ROISTATS_LDS_KEY_BYTES; }

// What a thread has seen of its window.  Integer pixels are their own keys and are summed exactly; float pixels are
// summed in float64, every thread its own pixels in the order it meets them.
template <typename T>
struct Seen {
  typedef typename median_key<T>::type K;
  typedef std::conditional_t<std::is_integral<T>::value, unsigned long long, double> Acc;
  int count = 0;
  Acc sum = 0;
  K kmin = ~(K)0, kmax = 0;
  __device__ __forceinline__ void take(K key) {
    ++count;
    if constexpr (std::is_integral<T>::value) sum += key; else sum += median_key<T>::value(key);
    kmin = key < kmin ? key : kmin;
    kmax = key > kmax ? key : kmax;
  }
};

// The pass over the window.  The window is cut into chunks of VW consecutive pixels (VW = 16 bytes of pixels where the
// window starts on 16 bytes and its mask on VW bytes: one 16-byte load per lane and chunk; VW = 1 otherwise), the chunks
// into WV equal runs, one per wave, which its lanes walk 64 chunks at a time, the loads of IN_FLIGHT such steps issued
// before the first is worked on.  COMPACT: wave w writes the keys of its surviving pixels to keys[seg .. seg + its
// count), seg = its first pixel, in pixel order -- no wave waits for another, and a survivor's slot depends on the mask
// and the pixels alone.  Returns the wave's count of survivors.
constexpr int IN_FLIGHT = 4;
template <typename T, int VW, bool COMPACT>
__device__ __forceinline__ int ingest(const T* __restrict__ v, const uint8_t* __restrict__ mask, int n,
                                      typename median_key<T>::type* keys, Seen<T>& seen) {
  typedef typename median_key<T>::type K;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int chunks = (n + VW - 1) / VW, per_wave = (chunks + WV - 1) / WV;
  const int begin = min(wave * per_wave, chunks), end = min(begin + per_wave, chunks);
  int written = 0;  // wave-uniform
  for (int c0 = begin; c0 < end; c0 += 64 * IN_FLIGHT) {  // wave-uniform trip counts: every lane takes part in the scans
    RawChunk<T, VW> raw[IN_FLIGHT];
#pragma unroll
    for (int u = 0; u < IN_FLIGHT; ++u) raw[u] = fetch<T, VW>(v, mask, n, c0 + 64 * u + lane, end);
#pragma unroll
    for (int u = 0; u < IN_FLIGHT; ++u) {
      if (c0 + 64 * u >= end) break;
      K ks[VW];
      bool ok[VW];
      int mine = 0;
#pragma unroll
      for (int j = 0; j < VW; ++j) {
        ok[j] = median_key<T>::key(raw[u].px[j], &ks[j]) && ((raw[u].mw[j >> 2] >> (8 * (j & 3))) & 0xFFu) != 0u;
        if (ok[j]) {
          seen.take(ks[j]);
          ++mine;
        }
      }
      const int incl = mg_wave_scan_incl_i32(mine);
      if (COMPACT) {
        int at = begin * VW + written + incl - mine;  // < the wave's last pixel: no more survivors than pixels
#pragma unroll
        for (int j = 0; j < VW; ++j)
          if (ok[j]) keys[at++] = ks[j];
      }
      written += __builtin_amdgcn_readlane(incl, 63);
    }
  }
  return written;
}

// Where survivor i (0 <= i < count) of the window lies in `keys`: the waves' runs one after the other.  (Scalars and
// conditional adds, not arrays: a table indexed by the run would go to scratch.)
struct Runs {
  int first1, first2, first3;  // index of the first survivor of waves 1, 2, 3
  int shift0, step1, step2, step3;  // slot - index inside the run of wave 0; what every later run adds to it
  __device__ __forceinline__ int slot(int i) const {
    return i + shift0 + (i >= first1 ? step1 : 0) + (i >= first2 ? step2 : 0) + (i >= first3 ? step3 : 0);
  }
};

// One workgroup per (marker, channel-time) window.  IN_LDS: the keys of the window fit `keys` (dynamic LDS, n keys);
// otherwise nothing is kept, the deviations and the selections read the window again from global memory.
// MEDIAN (mg_roi_masked_median): d_order is one double per window, numpy's nanmedian -- the mean of the two middle
// values in float64 (exact for every type but float64 itself), NaN where nothing takes part; no deviations, nothing
// else is written.
template <typename T, bool IN_LDS, bool MEDIAN = false>
__global__ __launch_bounds__(NT) void k_masked_stats(const T* __restrict__ d_roi, const uint8_t* __restrict__ d_mask,
                                                     int64_t mask_stride_m, int64_t mask_stride_t, int n_t, int n_ct,
                                                     int n, StatsQ qs, int n_q, int32_t* __restrict__ d_count,
                                                     double* __restrict__ d_stats, double* __restrict__ d_order) {
  typedef typename median_key<T>::type K;
  extern __shared__ __attribute__((aligned(16))) unsigned char s_dyn[];
  __shared__ uint32_t hist[256];
  __shared__ int s_pick[2], s_run[WV];
  K* keys = reinterpret_cast<K*>(s_dyn);
  const int64_t window = blockIdx.x;
  const int g = (int)(window / n_ct), ct = (int)(window % n_ct);
  const T* v = d_roi + window * n;
  // (the mask stays three scalar arguments and this line: as an MgMaskView argument its fields are fetched one by one
  // and three median instances take more scalar registers; through at() the prologue is scheduled another way, and
  // the uint16 statistics measured 0.7 % slower)
  const uint8_t* mask = d_mask + (int64_t)g * mask_stride_m + (int64_t)(ct % n_t) * mask_stride_t;
  constexpr int VW = 16 / (int)sizeof(T);
  const bool wide = (reinterpret_cast<uintptr_t>(v) & 15) == 0 && (reinterpret_cast<uintptr_t>(mask) & (VW - 1)) == 0;

  Seen<T> seen;
  const int run = wide ? ingest<T, VW, IN_LDS>(v, mask, n, keys, seen) : ingest<T, 1, IN_LDS>(v, mask, n, keys, seen);
  for (int i = threadIdx.x; i < 256; i += NT) hist[i] = 0u;  // (as select_kth wants it)
  if (IN_LDS && (threadIdx.x & 63) == 0) s_run[threadIdx.x >> 6] = run;
  // (mg_block_fold synchronises: s_run, hist and the keys are in place after the first of these)
  const int count = mg_block_fold(seen.count, [](int a, int b) { return a + b; });
  typename Seen<T>::Acc sum = 0;
  K kmin = 0, kmax = 0;
  if (!MEDIAN) {
    sum = mg_block_fold(seen.sum, [](auto a, auto b) { return a + b; });
    kmin = mg_block_fold(seen.kmin, [](K a, K b) { return a < b ? a : b; });
    kmax = mg_block_fold(seen.kmax, [](K a, K b) { return a > b ? a : b; });
  }

  double* stats = d_stats + window * 4;
  double* order = d_order + window * (MEDIAN ? 1 : n_q * 2);  // (not touched when n_q = 0)
  if (count == 0) {  // block-uniform
    if (MEDIAN) {
      if (threadIdx.x == 0) order[0] = QNAN;
      return;
    }
    if (threadIdx.x == 0) {
      d_count[window] = 0;
      stats[0] = 0.0, stats[1] = 0.0, stats[2] = QNAN, stats[3] = QNAN;
    }
    for (int i = threadIdx.x; i < 2 * n_q; i += NT) order[i] = QNAN;
    return;
  }

  Runs runs = {};
  if (IN_LDS) {
    // run w starts at pixel min(w * per_wave, chunks) * chunk (ingest) and holds s_run[w] survivors
    const int chunk = wide ? VW : 1, chunks = (n + chunk - 1) / chunk, per_wave = (chunks + WV - 1) / WV;
    const int p1 = min(per_wave, chunks) * chunk, p2 = min(2 * per_wave, chunks) * chunk;
    const int p3 = min(3 * per_wave, chunks) * chunk;
    runs.first1 = s_run[0], runs.first2 = runs.first1 + s_run[1], runs.first3 = runs.first2 + s_run[2];
    runs.shift0 = 0;
    runs.step1 = p1 - runs.first1;
    runs.step2 = (p2 - runs.first2) - (p1 - runs.first1);
    runs.step3 = (p3 - runs.first3) - (p2 - runs.first2);
  }
  // sorted[rank]: over the survivors' keys in LDS, or over the window's pixels in global memory
  auto select = [&](int rank) -> K {
    if (IN_LDS)
      return select_kth<K, median_key<T>::LEVELS>(
          count, [&](int i, K* key) { *key = keys[runs.slot(i)]; return true; }, rank, hist, s_pick);
    return select_kth<K, median_key<T>::LEVELS>(
        n, [&](int p, K* key) { return mask[p] && median_key<T>::key(v[p], key); }, rank, hist, s_pick);
  };
  if (MEDIAN) {
    const K lo = select((count - 1) / 2);
    const K hi = (count & 1) ? lo : select(count / 2);  // block-uniform
    if (threadIdx.x == 0) order[0] = (median_key<T>::value(lo) + median_key<T>::value(hi)) / 2.0;
    return;
  }

  // m2 = sum (x - mean)^2, each thread its own survivors in index order, then the fold's fixed tree
  // (where every survivor has the same value that value is the mean, whatever the rounded sum of n of them gives: m2
  // of a constant window is exactly 0 -- NaN if the constant is an infinity, as with any infinity under the mask)
  const double total = (double)sum, mean = kmin == kmax ? median_key<T>::value(kmin) : total / (double)count;
  double dev = 0.0;
  if (IN_LDS) {
    for (int i = threadIdx.x; i < count; i += NT) {
      const double d = median_key<T>::value(keys[runs.slot(i)]) - mean;
      dev += d * d;
    }
  } else {
    for (int p = threadIdx.x; p < n; p += NT) {
      K key;
      if (!mask[p] || !median_key<T>::key(v[p], &key)) continue;
      const double d = median_key<T>::value(key) - mean;
      dev += d * d;
    }
  }
  const double m2 = mg_block_fold(dev, [](double a, double b) { return a + b; });
  if (threadIdx.x == 0) {
    d_count[window] = count;
    stats[0] = total, stats[1] = m2, stats[2] = median_key<T>::value(kmin), stats[3] = median_key<T>::value(kmax);
  }

  // sorted[lo], sorted[hi] of every q: pos = (count - 1) q, lo = floor(pos), hi = min(lo + 1, count - 1)
  int have_rank = -1;  // the last selection, kept: hi of one q is often lo of the next, or lo itself
  K have_key = 0;
  for (int j = 0; j < n_q; ++j) {
    const double pos = (double)(count - 1) * qs.q[j];
    const int lo = (int)floor(pos), hi = min(lo + 1, count - 1);
    K pair[2];
#pragma unroll
    for (int e = 0; e < 2; ++e) {
      const int rank = e ? hi : lo;
      if (rank != have_rank) {  // block-uniform
        have_key = select(rank);
        have_rank = rank;
      }
      pair[e] = have_key;
    }
    if (threadIdx.x == 0) {
      order[2 * j] = median_key<T>::value(pair[0]);
      order[2 * j + 1] = median_key<T>::value(pair[1]);
    }
  }
}

// MEDIAN: d_order is the (m, n_c, n_t) medians, and d_count, d_stats, qs are not looked at.  Runs inside
// mg_dispatch_pixel, which has refused every other dtype code by now: no markers is MG_OK for a valid dtype only.
template <typename T, bool MEDIAN>
int launch_stats(const void* d_roi, const MgMaskView& mask, int m, int n_c, int n_t, int len, const StatsQ& qs, int n_q,
                 int32_t* d_count, double* d_stats, double* d_order, hipStream_t s) {
  typedef typename median_key<T>::type K;
  if (m == 0) return MG_OK;
  const int n = len * len, n_ct = n_c * n_t;
  const dim3 grid((unsigned)((int64_t)m * n_ct));
  if (keys_fit(n, sizeof(K)))
    hipLaunchKernelGGL((k_masked_stats<T, true, MEDIAN>), grid, dim3(NT), (size_t)n * sizeof(K), s, (const T*)d_roi, mask.p,
                       mask.stride_m, mask.stride_t, n_t, n_ct, n, qs, n_q, d_count, d_stats, d_order);
  else
    hipLaunchKernelGGL((k_masked_stats<T, false, MEDIAN>), grid, dim3(NT), 0, s, (const T*)d_roi, mask.p, mask.stride_m,
                       mask.stride_t, n_t, n_ct, n, qs, n_q, d_count, d_stats, d_order);
  MG_CHECK_LAUNCH();
  return MG_OK;
}

// What both entry points refuse: one workgroup a window, pixel indices are int.
bool windows_ok(const void* d_roi, const MgMaskView& mask, int m, int n_c, int n_t, int len) {
  return d_roi && mg_mask_view_ok(mask) && m >= 0 && n_c > 0 && n_t > 0 && len > 0 && len <= MG_ROISTATS_MAX_LEN &&
         (int64_t)n_c * n_t <= INT32_MAX && (int64_t)m * n_c * n_t <= INT32_MAX;
}

}  // namespace

extern "C" int mg_roi_masked_stats_keys_in_lds(int dtype, int roi_len) {
  if (roi_len <= 0 || roi_len > MG_ROISTATS_MAX_LEN) return MG_EINVAL;
  return mg_dispatch_pixel(dtype, [&](auto t) {
    return (int)keys_fit((int64_t)roi_len * roi_len, sizeof(typename median_key<decltype(t)>::type));
  });
}

extern "C" int mg_roi_masked_stats(const void* d_roi, int dtype, const uint8_t* d_mask, int64_t mask_stride_m,
                                   int64_t mask_stride_t, int m, int n_c, int n_t, int roi_len, const double* q, int n_q,
                                   int32_t* d_count, double* d_stats, double* d_order, void* stream) {
  const MgMaskView mask = {d_mask, mask_stride_m, mask_stride_t};
  if (!windows_ok(d_roi, mask, m, n_c, n_t, roi_len) || !d_count || !d_stats) return MG_EINVAL;
  if (n_q < 0 || n_q > MG_ROISTATS_MAX_Q || (n_q > 0 && (!q || !d_order))) return MG_EINVAL;
  StatsQ qs = {};
  for (int j = 0; j < n_q; ++j) {
    if (!(q[j] >= 0.0 && q[j] <= 1.0)) return MG_EINVAL;  // (NaN fails both)
    qs.q[j] = q[j];
  }
  hipStream_t s = mg_stream(stream);
  return mg_dispatch_pixel(dtype, [&](auto t) {
    return launch_stats<decltype(t), false>(d_roi, mask, m, n_c, n_t, roi_len, qs, n_q, d_count, d_stats, d_order, s);
  });
}

extern "C" int mg_roi_masked_median(const void* d_roi, int dtype, const uint8_t* d_mask, int64_t mask_stride_m,
                                    int64_t mask_stride_t, int m, int n_c, int n_t, int roi_len, double* d_median,
                                    void* stream) {
  const MgMaskView mask = {d_mask, mask_stride_m, mask_stride_t};
  if (!windows_ok(d_roi, mask, m, n_c, n_t, roi_len) || !d_median) return MG_EINVAL;
  hipStream_t s = mg_stream(stream);
  return mg_dispatch_pixel(dtype, [&](auto t) {
    return launch_stats<decltype(t), true>(d_roi, mask, m, n_c, n_t, roi_len, StatsQ{}, 0, nullptr, nullptr, d_median, s);
  });
}
