// roi.where(mask).{sum, mean, std, var, min, max, count, quantile}(dim=[roi_y, roi_x]) of an already gathered roi
// (README.md:21-22, identify.py:76-80, filter.py:20-22): one workgroup per (marker, channel-time) reads the window and
// its mask ONCE from global memory, reduces count / sum / min / max on the way in and keeps the keys of the surviving
// pixels in LDS; the squared deviations and every order statistic asked for then run out of LDS.  The masked median
// (mg_roi_masked_median: numpy's nanmedian) is the same kernel in its median mode: the middle ranks, nothing else.
// The read walks mg_windows.h's chunks and runs (its loop frame is written out in ingest), the ranks of the fractions
// are walked by mg_select.h's order_pairs, and both entries stand in mg_windows.h's frame (check, fractions, launch).
//
// Roofline: HBM.  Per window L*L*(sizeof(T) + 1) bytes read, 4 + 32 + 16 n_q bytes written.
#include "mg_windows.h"

namespace {

constexpr int NT = MG_WINDOW_THREADS, WV = MG_WINDOW_WAVES;

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

// The pass over the window: mg_windows.h's walk -- chunks of VW pixels, a run of them per wave (wave_run), the loads of
// IN_FLIGHT steps issued before the first is worked on -- written out here, not as a body of walk_chunks: as a body
// the instances that select from global memory come out with other registers and the uint16 one 2 % slower a select
// (DESIGN.md section 38).  COMPACT: wave w writes the keys of its surviving pixels to keys[seg .. seg + its count),
// seg = its first pixel, in pixel order -- no wave waits for another, and a survivor's slot depends on the mask and the
// pixels alone.  Returns the wave's count of survivors.
template <typename T, int VW, bool COMPACT>
__device__ __forceinline__ int ingest(const T* __restrict__ v, const uint8_t* __restrict__ mask, int n,
                                      typename median_key<T>::type* keys, Seen<T>& seen) {
  typedef typename median_key<T>::type K;
  const int lane = threadIdx.x & 63;
  const WaveRun run = wave_run(n, VW, threadIdx.x >> 6);
  int written = 0;  // wave-uniform
  for (int c0 = run.begin; c0 < run.end; c0 += 64 * IN_FLIGHT) {  // wave-uniform trip counts: every lane scans
    RawChunk<T, VW> raw[IN_FLIGHT];
#pragma unroll
    for (int u = 0; u < IN_FLIGHT; ++u) raw[u] = fetch<T, VW>(v, mask, n, c0 + 64 * u + lane, run.end);
#pragma unroll
    for (int u = 0; u < IN_FLIGHT; ++u) {
      if (c0 + 64 * u >= run.end) break;
      K ks[VW];
      bool ok[VW];
      int mine = 0;
#pragma unroll
      for (int j = 0; j < VW; ++j) {
        ok[j] = median_key<T>::key(raw[u].px[j], &ks[j]) && raw[u].under_mask(j);
        if (ok[j]) {
          seen.take(ks[j]);
          ++mine;
        }
      }
      const int incl = mg_wave_scan_incl_i32(mine);
      if (COMPACT) {
        int at = run.begin * VW + written + incl - mine;  // < the wave's last pixel: no more survivors than pixels
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
  const bool wide = window_is_wide(v, mask);

  Seen<T> seen;
  const int run = with_chunk_width<T>(
      wide, [&](auto vw) { return ingest<T, decltype(vw)::value, IN_LDS>(v, mask, n, keys, seen); });
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
      if (threadIdx.x == 0) order[0] = MG_QNAN;
      return;
    }
    if (threadIdx.x == 0) {
      d_count[window] = 0;
      stats[0] = 0.0, stats[1] = 0.0, stats[2] = MG_QNAN, stats[3] = MG_QNAN;
    }
    order_pairs_of_none(n_q, order);
    return;
  }

  Runs runs = {};
  if (IN_LDS) {
    // run w starts at the first pixel of wave w's first chunk (ingest) and holds s_run[w] survivors
    const int chunk = wide ? wide_chunk<T> : 1;
    const int p1 = wave_run(n, chunk, 1).begin * chunk, p2 = wave_run(n, chunk, 2).begin * chunk;
    const int p3 = wave_run(n, chunk, 3).begin * chunk;
    runs.first1 = s_run[0], runs.first2 = runs.first1 + s_run[1], runs.first3 = runs.first2 + s_run[2];
    runs.shift0 = 0;
    runs.step1 = p1 - runs.first1;
    runs.step2 = (p2 - runs.first2) - (p1 - runs.first1);
    runs.step3 = (p3 - runs.first3) - (p2 - runs.first2);
  }
  // sorted[rank]: over the survivors' keys in LDS, or over the window's pixels in global memory
  auto kept_key = [&](int i, K* key) { *key = keys[runs.slot(i)]; return true; };
  auto pixel_key = [&](int p, K* key) { return mask[p] && median_key<T>::key(v[p], key); };
  auto select = [&](int rank) -> K {
    if (IN_LDS) return select_kth<K, median_key<T>::LEVELS>(count, kept_key, rank, hist, s_pick);
    return select_kth<K, median_key<T>::LEVELS>(n, pixel_key, rank, hist, s_pick);
  };
  // sorted[rank + 1], as order_pairs asks for it: a second selection, not next_above (DESIGN.md section 38 has the
  // figures of both and the rule that decided)
  auto next = [&](K, int rank) -> K { return select(rank + 1); };
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

  order_pairs<T>(count, qs.q, n_q, select, next, order);
}

// MEDIAN: d_order is the (m, n_c, n_t) medians, and d_count, d_stats, qs are not looked at.
template <bool MEDIAN>
int launch_stats(const void* d_roi, int dtype, const MgMaskView& mask, int m, int n_c, int n_t, int len, const StatsQ& qs,
                 int n_q, int32_t* d_count, double* d_stats, double* d_order, void* stream) {
  const int n = len * len, n_ct = n_c * n_t;
  hipStream_t s = mg_stream(stream);
  return mg_windows_launch(dtype, m, n_ct, [&](auto t, dim3 grid, dim3 block) {
    typedef decltype(t) T;
    typedef typename median_key<T>::type K;
    if (keys_fit(n, sizeof(K)))
      hipLaunchKernelGGL((k_masked_stats<T, true, MEDIAN>), grid, block, (size_t)n * sizeof(K), s, (const T*)d_roi, mask.p,
                         mask.stride_m, mask.stride_t, n_t, n_ct, n, qs, n_q, d_count, d_stats, d_order);
    else
      hipLaunchKernelGGL((k_masked_stats<T, false, MEDIAN>), grid, block, 0, s, (const T*)d_roi, mask.p, mask.stride_m,
                         mask.stride_t, n_t, n_ct, n, qs, n_q, d_count, d_stats, d_order);
  });
}

// What both entry points refuse beyond mg_windows_check: no roi, no mask (every other window entry takes a null
// mask), and more than 2^31 - 1 windows a marker -- n_ct is an int in the kernel.
bool windows_ok(const void* d_roi, const MgMaskView& mask, int m, int n_c, int n_t, int len) {
  return d_roi && mask.p && (int64_t)n_c * n_t <= INT32_MAX &&
         mg_windows_check(m, n_c, n_t, len, MG_ROISTATS_MAX_LEN, {mask.stride_m, mask.stride_t});
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
  StatsQ qs = {};
  if (!mg_fractions(q, n_q, MG_ROISTATS_MAX_Q, qs.q) || (n_q > 0 && !d_order)) return MG_EINVAL;
  return launch_stats<false>(d_roi, dtype, mask, m, n_c, n_t, roi_len, qs, n_q, d_count, d_stats, d_order, stream);
}

extern "C" int mg_roi_masked_median(const void* d_roi, int dtype, const uint8_t* d_mask, int64_t mask_stride_m,
                                    int64_t mask_stride_t, int m, int n_c, int n_t, int roi_len, double* d_median,
                                    void* stream) {
  const MgMaskView mask = {d_mask, mask_stride_m, mask_stride_t};
  if (!windows_ok(d_roi, mask, m, n_c, n_t, roi_len) || !d_median) return MG_EINVAL;
  return launch_stats<true>(d_roi, dtype, mask, m, n_c, n_t, roi_len, StatsQ{}, 0, nullptr, nullptr, d_median, stream);
}
