// Data-driven fg / bg masks of an already gathered roi (segment_rois; not in the reference, whose masks are drawn shapes:
// find.py:383-400, 561-586): per (marker, timepoint) window a threshold (Otsu on the 256 to_uint8 bins of the window, or a
// number), a 3x3 opening, a bounded growth of the drawn foreground inside the opened mask and a guard band cut out of the
// drawn background.  tests/segment_ref.py restates the contract in NumPy + scipy.ndimage; the kernel equals it bit for bit.
//
// One workgroup per window, one launch.  The window is read twice (range, then bins: the second read meets the caches),
// the three input masks once; bins are bytes in LDS, every mask a FLAT bit plane in LDS (bit p = pixel p = row * L + col,
// no row padding): a wave's ballot over 64 consecutive pixels IS two words of the plane, and a 3x3 step is two passes
// over the words -- left / right neighbours are the string shifted by one bit under a column mask, upper / lower
// neighbours the string shifted by L bits (a funnel shift of two words).  Integer histogram, integer prefix sums, a
// total order in the arg-max: nothing depends on the order in which threads arrive.  The entry stands in mg_windows.h's
// frame (check, launch); the pixel loop is the kernel's own (for_each_pixel: one plane, no mask, a pixel a lane -- on
// the chunk walk of mg_windows.h the uint8 instance took 92 VGPRs for 44).
#include "mg_windows.h"

namespace {

constexpr int NT = MG_WINDOW_THREADS, WV = MG_WINDOW_WAVES;
constexpr int HIST_COPIES = 4;  // a power of two

// the bit planes of a window, each `words` 32-bit words (an even number: ballots are stored as 64-bit pairs)
enum Plane { P_ON, P_OPEN, P_FG, P_TMP, P_FG0, P_BG0, P_ALLOWED, P_NOTFIRST, P_NOTLAST, P_VALID, N_PLANES };

struct SegArgs {
  const void* roi;
  int64_t stride_m, stride_t;
  MgMaskView fg0, bg0, allowed;  // allowed.p may be null: no such mask
  int n_t, len;
  int use_otsu;
  double threshold;
  int open_radius, max_grow, bg_guard, min_area;
  uint8_t *fg, *bg;
  double* thr;
  int32_t* counts;
  uint8_t* segmented;
};

// The drawn masks: src[k][0 .. n) bytes -> plane[k] bits (non-zero = set; bits n .. 64 chunks are clear), k < count, a
// wave per 64 pixels.  The loads of PACK_CHUNKS chunks of every mask are issued before the first ballot: the pass is a
// handful of memory round trips, not one per chunk.
constexpr int PACK_CHUNKS = 4;
template <int COUNT>
__device__ __forceinline__ void pack_bytes(const uint8_t* const (&src)[COUNT], int n, int chunks, uint32_t* const (&plane)[COUNT]) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (int c0 = PACK_CHUNKS * wave; c0 < chunks; c0 += PACK_CHUNKS * WV) {
    uint8_t byte[COUNT][PACK_CHUNKS];
#pragma unroll
    for (int k = 0; k < COUNT; ++k)
#pragma unroll
      for (int e = 0; e < PACK_CHUNKS; ++e) {
        const int p = (c0 + e) * 64 + lane;
        byte[k][e] = p < n ? src[k][p] : (uint8_t)0;  // (p < n: chunk c0 + e exists)
      }
#pragma unroll
    for (int k = 0; k < COUNT; ++k)
#pragma unroll
      for (int e = 0; e < PACK_CHUNKS; ++e) {
        const uint64_t bits = __ballot(byte[k][e] != 0);
        if (lane == 0 && c0 + e < chunks) reinterpret_cast<uint64_t*>(plane[k])[c0 + e] = bits;
      }
  }
}

// f(p, v[p]) for the pixels p = threadIdx.x, + NT, ... of a window, PIXEL_LOADS loads issued before the first use
constexpr int PIXEL_LOADS = 8;
template <typename T, class F>
__device__ __forceinline__ void for_each_pixel(const T* __restrict__ v, int n, F&& f) {
  for (int p0 = threadIdx.x; p0 < n; p0 += NT * PIXEL_LOADS) {
    T x[PIXEL_LOADS];
#pragma unroll
    for (int u = 0; u < PIXEL_LOADS; ++u) {
      const int p = p0 + u * NT;
      x[u] = p < n ? v[p] : T(0);
    }
#pragma unroll
    for (int u = 0; u < PIXEL_LOADS; ++u) {
      const int p = p0 + u * NT;
      if (p < n) f(p, x[u]);
    }
  }
}

// One 3x3 step in place: x = dilate(x) & keep, or x = erode(x) (outside the window is off).  `tmp` holds the row pass.
// q = L / 32, s = L % 32.  Called by all; x is final for every thread on return.
template <bool DILATE>
__device__ __forceinline__ void morph(uint32_t* x, uint32_t* tmp, const uint32_t* notfirst, const uint32_t* notlast,
                                      const uint32_t* keep, int words, int q, int s) {
  for (int i = threadIdx.x; i < words; i += NT) {
    const uint32_t a = x[i], l = i > 0 ? x[i - 1] : 0u, r = i + 1 < words ? x[i + 1] : 0u;
    const uint32_t from_left = ((a << 1) | (l >> 31)) & notfirst[i];   // bit p: pixel p - 1, where p is not in column 0
    const uint32_t from_right = ((a >> 1) | (r << 31)) & notlast[i];   // bit p: pixel p + 1, where p is not in column L - 1
    tmp[i] = DILATE ? (a | from_left | from_right) : (a & from_left & from_right);
  }
  __syncthreads();
  for (int i = threadIdx.x; i < words; i += NT) {
    const int j = i - q, k = i + q;
    const uint32_t a = tmp[i];
    const uint64_t above = ((uint64_t)(j >= 0 ? tmp[j] : 0u) << 32) | (j >= 1 ? tmp[j - 1] : 0u);
    const uint64_t below = ((uint64_t)(k + 1 < words ? tmp[k + 1] : 0u) << 32) | (k < words ? tmp[k] : 0u);
    const uint32_t from_above = (uint32_t)(above >> (32 - s));  // bit p: pixel p - L (none in row 0: zeros come in)
    const uint32_t from_below = (uint32_t)(below >> s);         // bit p: pixel p + L (bits from n on are clear)
    x[i] = DILATE ? ((a | from_above | from_below) & keep[i]) : (a & from_above & from_below);
  }
  __syncthreads();
}

__device__ __forceinline__ int block_popcount(const uint32_t* plane, int words) {
  int c = 0;
  for (int i = threadIdx.x; i < words; i += NT) c += __popc(plane[i]);
  return mg_block_fold(c, [](int a, int b) { return a + b; });
}

// bit plane -> 0 / 1 bytes, every byte of out[0 .. n) written once; four pixels a thread where `out` is 4-byte aligned
__device__ __forceinline__ void unpack_bits(const uint32_t* plane, int n, uint8_t* __restrict__ out) {
  if ((reinterpret_cast<uintptr_t>(out) & 3) == 0) {
    for (int p = 4 * threadIdx.x; p < n; p += 4 * NT) {
      const uint32_t b = (plane[p >> 5] >> (p & 31)) & 0xFu;  // (p is a multiple of 4: the four bits lie in one word)
      const uint32_t bytes = (b & 1u) | ((b & 2u) << 7) | ((b & 4u) << 14) | ((b & 8u) << 21);
      if (p + 4 <= n) {
        *reinterpret_cast<uint32_t*>(out + p) = bytes;
      } else {
        for (int e = 0; p + e < n; ++e) out[p + e] = (uint8_t)((bytes >> (8 * e)) & 1u);
      }
    }
  } else {
    for (int p = threadIdx.x; p < n; p += NT) out[p] = (uint8_t)((plane[p >> 5] >> (p & 31)) & 1u);
  }
}

template <typename T>
__global__ __launch_bounds__(NT) void k_threshold_masks(SegArgs a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char s_dyn[];
  __shared__ int hist[256 * HIST_COPIES];  // bin b of copy c at [HIST_COPIES * b + c]
  __shared__ int s_k;
  const int L = a.len, n = L * L, chunks = (n + 63) / 64, words = 2 * chunks;
  uint32_t* planes = reinterpret_cast<uint32_t*>(s_dyn);
  uint8_t* bins = s_dyn + (size_t)N_PLANES * words * 4;  // n bytes
  auto plane = [&](int which) { return planes + which * words; };
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int64_t window = blockIdx.x;
  const int g = (int)(window / a.n_t), t = (int)(window % a.n_t);
  const T* v = static_cast<const T*>(a.roi) + g * a.stride_m + t * a.stride_t;

  // the drawn masks, once
  const uint8_t* const fg0 = a.fg0.at(g, t);
  const uint8_t* const bg0 = a.bg0.at(g, t);
  if (a.allowed.p) {  // block-uniform
    const uint8_t* const src[3] = {fg0, bg0, a.allowed.at(g, t)};
    uint32_t* const dst[3] = {plane(P_FG0), plane(P_BG0), plane(P_ALLOWED)};
    pack_bytes<3>(src, n, chunks, dst);
  } else {
    const uint8_t* const src[2] = {fg0, bg0};
    uint32_t* const dst[2] = {plane(P_FG0), plane(P_BG0)};
    pack_bytes<2>(src, n, chunks, dst);
  }
#pragma unroll
  for (int e = 0; e < HIST_COPIES; ++e) hist[HIST_COPIES * threadIdx.x + e] = 0;
  static_assert(NT == 256, "one histogram bin a thread");

  // 1. range of the non-NaN pixels, in the pixels' own type (every value of it is a float64)
  double tlo = INFINITY, thi = -INFINITY;
  if constexpr (std::is_integral<T>::value) {
    uint32_t ilo = 0xFFFFFFFFu, ihi = 0u;
    for_each_pixel(v, n, [&](int, T px) {
      const uint32_t x = px;
      ilo = x < ilo ? x : ilo, ihi = x > ihi ? x : ihi;
    });
    if (ilo <= ihi) tlo = (double)ilo, thi = (double)ihi;
  } else {
    T flo = INFINITY, fhi = -INFINITY;
    for_each_pixel(v, n, [&](int, T x) {
      if (x == x) flo = x < flo ? x : flo, fhi = x > fhi ? x : fhi;
    });
    tlo = (double)flo, thi = (double)fhi;
  }
  // (mg_block_fold synchronises: the planes above and the cleared histogram are in place after the first)
  const double lo = mg_block_fold(tlo, [](double x, double y) { return x < y ? x : y; });
  const double hi = mg_block_fold(thi, [](double x, double y) { return x > y ? x : y; });
  const double range = hi - lo;
  const bool flat = !(range > 0.0) || !(range < INFINITY);  // no pixels: -inf; an infinity among them: inf or NaN

  bool segmented = false;
  double thr = MG_QNAN;
  if (!flat) {  // block-uniform
    // 2. bins (to_uint8's order of operations), as bytes; with a numeric threshold the "bin" is the comparison itself
    // (the histogram in HIST_COPIES interleaved copies, a lane's copy by its number: a background that fills a few
    // bins meets in fewer lanes per address)
    int* const my_hist = hist + (lane & (HIST_COPIES - 1));
    if (!a.use_otsu) {
      for_each_pixel(v, n, [&](int p, T px) {
        const double x = (double)px;
        bins[p] = (uint8_t)(x > a.threshold ? 1 : 0);  // (NaN: off)
      });
    } else if constexpr (std::is_integral<T>::value) {
      // Integer pixels: 255 (v - lo) < 2^24 and hi - lo < 2^16 are exact, and a quotient that is no integer lies at least
      // 1 / (hi - lo) from one -- far beyond float64 rounding -- so the bin is the integer quotient: float32 estimate,
      // corrected by the remainder.
      const uint32_t ilo = (uint32_t)lo, irange = (uint32_t)range;
      const float inv = 1.0f / (float)irange;
      for_each_pixel(v, n, [&](int p, T px) {
        const uint32_t num = 255u * ((uint32_t)px - ilo);
        uint32_t b = (uint32_t)((float)num * inv);
        const int rem = (int)num - (int)(b * irange);
        b = rem < 0 ? b - 1u : rem >= (int)irange ? b + 1u : b;
        atomicAdd(&my_hist[HIST_COPIES * b], 1);
        bins[p] = (uint8_t)b;
      });
    } else {
      for_each_pixel(v, n, [&](int p, T px) {
        const double x = (double)px;
        int b = 0;
        if (x == x) {
          const double u = (255.0 * (x - lo)) / range;
          b = u >= 255.0 ? 255 : (int)u;  // (u >= 0: truncation is floor)
          atomicAdd(&my_hist[HIST_COPIES * b], 1);
        }
        bins[p] = (uint8_t)b;
      });
    }
    __syncthreads();
    // 3. Otsu: one wave, four bins a lane
    int kstar = 0;
    if (a.use_otsu) {
      if (wave == 0) {
        int h[4], cnt = 0, sum = 0;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          h[e] = 0;
#pragma unroll
          for (int c = 0; c < HIST_COPIES; ++c) h[e] += hist[HIST_COPIES * (4 * lane + e) + c];
          cnt += h[e], sum += (4 * lane + e) * h[e];
        }
        const int cnt_incl = mg_wave_scan_incl_i32(cnt), sum_incl = mg_wave_scan_incl_i32(sum);
        const int64_t total = __builtin_amdgcn_readlane(cnt_incl, 63), stot = __builtin_amdgcn_readlane(sum_incl, 63);
        int w0 = cnt_incl - cnt, s0 = sum_incl - sum, best_k = 255;
        double best = -1.0;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const int k = 4 * lane + e;
          w0 += h[e], s0 += k * h[e];
          const int64_t w1 = total - w0;
          if (k <= 254 && w0 > 0 && w1 > 0) {
            const double d = (double)(stot * (int64_t)w0 - total * (int64_t)s0);
            const double value = (d * d) / (double)((int64_t)w0 * w1);
            if (value > best) best = value, best_k = k;  // (k ascending: the smaller k keeps a tie)
          }
        }
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) {
          const double ov = __shfl_xor(best, off);
          const int ok = __shfl_xor(best_k, off);
          if (ov > best || (ov == best && ok < best_k)) best = ov, best_k = ok;
        }
        if (lane == 0) s_k = best_k;
      }
      __syncthreads();
      kstar = s_k;
      thr = lo + ((double)(kstar + 1) * range) / 255.0;
    } else {
      thr = a.threshold;
    }
    // on = b > k*, the column masks and the window's extent as planes
    {
      uint64_t* on = reinterpret_cast<uint64_t*>(plane(P_ON));
      uint64_t* open = reinterpret_cast<uint64_t*>(plane(P_OPEN));
      uint64_t* notfirst = reinterpret_cast<uint64_t*>(plane(P_NOTFIRST));
      uint64_t* notlast = reinterpret_cast<uint64_t*>(plane(P_NOTLAST));
      uint64_t* valid = reinterpret_cast<uint64_t*>(plane(P_VALID));
      // p / L by a multiplication: p < 2^14 and L <= 2^7, so ceil(2^32 / L) gives the exact quotient
      const uint32_t magic = L > 1 ? 0xFFFFFFFFu / (uint32_t)L + 1u : 0u;
      for (int c = wave; c < chunks; c += WV) {
        const int p = c * 64 + lane, col = L > 1 ? p - (int)__umulhi((uint32_t)p, magic) * L : 0;
        const bool in = p < n;
        const uint64_t b_on = __ballot(in && (int)bins[in ? p : 0] > kstar);
        const uint64_t b_nf = __ballot(in && col != 0), b_nl = __ballot(in && col != L - 1), b_in = __ballot(in);
        if (lane == 0) on[c] = b_on, open[c] = b_on, notfirst[c] = b_nf, notlast[c] = b_nl, valid[c] = b_in;
      }
    }
    __syncthreads();
    const int q = L >> 5, s = L & 31;
    // 4. opening, then the allowed pixels; 5. the drawn foreground's part of it, grown inside it
    for (int r = 0; r < a.open_radius; ++r)
      morph<false>(plane(P_OPEN), plane(P_TMP), plane(P_NOTFIRST), plane(P_NOTLAST), nullptr, words, q, s);
    for (int r = 0; r < a.open_radius; ++r)
      morph<true>(plane(P_OPEN), plane(P_TMP), plane(P_NOTFIRST), plane(P_NOTLAST), plane(P_VALID), words, q, s);
    for (int i = threadIdx.x; i < words; i += NT) {
      uint32_t o = plane(P_OPEN)[i];
      if (a.allowed.p) o &= plane(P_ALLOWED)[i];
      plane(P_OPEN)[i] = o;
      plane(P_FG)[i] = o & plane(P_FG0)[i];
    }
    __syncthreads();
    for (int r = 0; r < a.max_grow; ++r)
      morph<true>(plane(P_FG), plane(P_TMP), plane(P_NOTFIRST), plane(P_NOTLAST), plane(P_OPEN), words, q, s);
    // 6. too little left: the drawn masks stay
    const int area = block_popcount(plane(P_FG), words);
    segmented = area >= (a.min_area > 1 ? a.min_area : 1);
    if (segmented) {
      // 7. background: the drawn one without a guard band around everything bright
      for (int i = threadIdx.x; i < words; i += NT) plane(P_ON)[i] |= plane(P_FG)[i];
      __syncthreads();
      for (int r = 0; r < a.bg_guard; ++r)
        morph<true>(plane(P_ON), plane(P_TMP), plane(P_NOTFIRST), plane(P_NOTLAST), plane(P_VALID), words, q, s);
      for (int i = threadIdx.x; i < words; i += NT) plane(P_BG0)[i] &= ~plane(P_ON)[i];
      __syncthreads();
    }
  }

  // 8. outputs
  const uint32_t* fg = plane(segmented ? P_FG : P_FG0);
  const uint32_t* bg = plane(P_BG0);
  const int n_fg = block_popcount(fg, words), n_bg = block_popcount(bg, words);
  unpack_bits(fg, n, a.fg + window * n);
  unpack_bits(bg, n, a.bg + window * n);
  if (threadIdx.x == 0) {
    a.thr[window] = thr;
    a.counts[2 * window] = n_fg, a.counts[2 * window + 1] = n_bg;
    a.segmented[window] = segmented ? 1 : 0;
  }
}

}  // namespace

extern "C" int mg_roi_threshold_masks(const void* d_roi, int dtype, int64_t stride_m, int64_t stride_t,
                                      const uint8_t* d_fg0, int64_t fg_stride_m, int64_t fg_stride_t,
                                      const uint8_t* d_bg0, int64_t bg_stride_m, int64_t bg_stride_t,
                                      const uint8_t* d_allowed, int64_t al_stride_m, int64_t al_stride_t, int m, int n_t,
                                      int roi_len, int use_otsu, double threshold, int open_radius, int max_grow,
                                      int bg_guard, int min_area, uint8_t* d_fg, uint8_t* d_bg, double* d_threshold,
                                      int32_t* d_counts, uint8_t* d_segmented, void* stream) {
  const MgMaskView fg0 = {d_fg0, fg_stride_m, fg_stride_t}, bg0 = {d_bg0, bg_stride_m, bg_stride_t};
  const MgMaskView allowed = {d_allowed, al_stride_m, al_stride_t};  // (no pointer: no such mask; its strides still count)
  if (!d_roi || !mg_mask_view_ok(fg0) || !mg_mask_view_ok(bg0) || !d_fg || !d_bg || !d_threshold || !d_counts || !d_segmented)
    return MG_EINVAL;
  if (!mg_windows_check(m, 1, n_t, roi_len, MG_SEGMENT_MAX_LEN, {stride_m, stride_t, al_stride_m, al_stride_t}))
    return MG_EINVAL;
  if (open_radius < 0 || open_radius > MG_SEGMENT_MAX_OPEN || max_grow < 0 || max_grow > MG_SEGMENT_MAX_GROW ||
      bg_guard < 0 || bg_guard > MG_SEGMENT_MAX_GUARD || min_area < 0)
    return MG_EINVAL;
  if (!use_otsu && threshold != threshold) return MG_EINVAL;
  SegArgs a = {d_roi,     stride_m,    stride_t, fg0,      bg0,      allowed, n_t,  roi_len,     use_otsu ? 1 : 0,
               threshold, open_radius, max_grow, bg_guard, min_area, d_fg,    d_bg, d_threshold, d_counts,
               d_segmented};
  const int n = roi_len * roi_len, words = 2 * ((n + 63) / 64);
  const size_t lds = (size_t)N_PLANES * words * 4 + (size_t)n;
  hipStream_t s = mg_stream(stream);
  return mg_windows_launch(dtype, m, n_t, [&](auto t, dim3 grid, dim3 block) {
    hipLaunchKernelGGL((k_threshold_masks<decltype(t)>), grid, block, lds, s, a);
  });
}
