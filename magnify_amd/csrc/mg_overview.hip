// plot.overview ("plot.overview: a picture of the result, made on the device"): the label map of the
// foreground masks in image coordinates and the composite of the (C, T, H, W) image -- block means at 2^level,
// contrast limits, one additive colour per channel, the label overlay -- as an RGB picture.  tests/plot_ref.py restates
// both in NumPy; the kernels are held to it bit for bit.  s = 2^level, hk = ceil(h / s), wk = ceil(w / s).
//
// k_image_labels: one thread per four pixels of a mask row (one 4-byte load where they are an aligned word).  A set
// pixel (ry, rx) of fg[i, t] claims label pixel ((top + ry) >> level, (left + rx) >> level) of plane t with
// atomicMax(i + 1): the largest marker index wins, whatever the order of the work -- at level 0 the reference's
// sequential overwrite (plot/image.py:160-166).  Claims outside the image are dropped (a window larger than the image).
//
// k_overview: a streaming pass over the image, every pixel read once, 3 / s^2 bytes written per pixel and channel
// block.  A thread owns a run of OC output pixels of one output row: CH = OC s input columns, a whole number of
// 16-byte vectors (8-byte ones for one-byte pixels at level 0: RunShape), over s rows.  Where the run lies inside the
// image, its first byte is vector-aligned and so is the row pitch, its vectors are read in batches of up to eight
// independent loads; otherwise row by row, with vector loads where that row's start is aligned and element by element
// where it is not, and in the ragged last run of a row.  Block sums: uint32 for u8 / u16 (64^2 * 65535 < 2^32, exact), float64 for float pixels, the block's rows
// from the top, each from the left, on every path.  The channels of an output pixel are accumulated in the same
// thread -- mean, (mean - lo) / (hi - lo), clamp, acc += u * colour, min(acc, 1), all float64, one operation at a time
// -- then the overlay is applied from the label map and the three bytes are written once.  No LDS, no atomics.
#include "mg_composite.h"

namespace {

// ---- label map ------------------------------------------------------------------------------------------------------

__global__ __launch_bounds__(256) void k_image_labels(MgMaskView fg, const int32_t* __restrict__ origin, int n_t, int L,
                                                      int qpr, int level, int h, int w, int hk, int wk, int64_t total,
                                                      int32_t* __restrict__ labels) {
  const bool small = total <= 0x7FFFFFFFLL;  // (uniform) 32-bit index arithmetic
  const int64_t stride = (int64_t)gridDim.x * 256;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += stride) {
    int64_t mt, g;  // i = (((marker g) * n_t + t) * L + ry) * qpr + word of the row
    int rx0, ry, t;
    if (small) {
      const uint32_t u = (uint32_t)i, row = u / (uint32_t)qpr, a = row / (uint32_t)L, b = a / (uint32_t)n_t;
      rx0 = (int)(u - row * (uint32_t)qpr) * 4, ry = (int)(row - a * (uint32_t)L), t = (int)(a - b * (uint32_t)n_t), mt = a, g = b;
    } else {
      const int64_t row = i / qpr;
      rx0 = (int)(i - row * qpr) * 4, mt = row / L, ry = (int)(row - mt * L), g = mt / n_t, t = (int)(mt - g * n_t);
    }
    const uint8_t* q = fg.at(g, t) + (int64_t)ry * L;
    const int y = origin[2 * mt] + ry, left = origin[2 * mt + 1];
    if (y < 0 || y >= h) continue;
    int32_t* out = labels + ((int64_t)t * hk + (y >> level)) * wk;
    uint32_t four = 0;  // the thread's four mask bytes: one load where they are a whole, aligned word
    if (rx0 + 4 <= L && (reinterpret_cast<uintptr_t>(q + rx0) & 3) == 0) {
      four = *reinterpret_cast<const uint32_t*>(q + rx0);
    } else {
      for (int k = 0; k < 4 && rx0 + k < L; ++k) four |= (uint32_t)(q[rx0 + k] != 0) << (8 * k);
    }
    if (!four) continue;
    int last = -1;
    for (int k = 0; k < 4; ++k) {
      const int rx = rx0 + k, x = left + rx;
      if (x < 0 || x >= w || !((four >> (8 * k)) & 0xFFu)) continue;
      const int X = x >> level;
      // one claim per label pixel of this thread's four; above level 0, where up to 4^level mask pixels of a marker meet
      // in a label pixel, look first (past the non-coherent L1: the map only grows, a value seen is a lower bound)
      if (X != last && (level == 0 || __hip_atomic_load(out + X, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) < (int32_t)(g + 1)))
        atomicMax(out + X, (int32_t)(g + 1));
      last = X;
    }
  }
}

// ---- composite ------------------------------------------------------------------------------------------------------

template <typename T, int S>
struct RunShape {
  // bytes of a vector load: 16, but 8 for one-byte pixels at level 0 -- 16 output pixels with three float64 accumulators
  // each leave one wave per SIMD (256 VGPRs), 8 leave three
  static constexpr int VB = (sizeof(T) == 1 && S == 1) ? 8 : 16;
  using Vec = std::conditional_t<VB == 8, uint2, uint4>;
  static constexpr int N = VB / (int)sizeof(T);                                           // elements per vector
  static constexpr int VPR = S > N ? S / N : 1;                                           // vectors per row of a run
  static constexpr int CH = VPR * N, OC = CH / S;                                         // input / output columns of a run
  static constexpr int B = S * VPR < 8 ? S * VPR : 8;                                     // vector loads of a batch
};

// sum[j] += the in-image pixels of block j of the run at p (row pitch w): rows [0, nrows), nj blocks, block j columns
// [j S, j S + min(S, cols_left - j S)).  One order of additions per block on every path: rows from the top, each from
// the left.
template <typename T, int S, typename Acc>
__device__ __forceinline__ void block_sums(const T* __restrict__ p, int w, int nrows, int nj, int cols_left,
                                           Acc (&sum)[RunShape<T, S>::OC]) {
  using Sh = RunShape<T, S>;
  using Vec = typename Sh::Vec;
  constexpr int N = Sh::N, VPR = Sh::VPR, CH = Sh::CH, OC = Sh::OC, B = Sh::B, VB = Sh::VB;
  const bool full = cols_left >= CH;  // every column of the run is in the image
  if (full && (reinterpret_cast<uintptr_t>(p) & (VB - 1)) == 0 && (((int64_t)w * (int64_t)sizeof(T)) & (VB - 1)) == 0) {
    const int nk = nrows * VPR;  // vector k of the run: row k / VPR, vector k % VPR of that row
    for (int k0 = 0; k0 < nk; k0 += B) {
      Vec bits[B];
#pragma unroll
      for (int b = 0; b < B; ++b) {
        const int k = k0 + b;
        if (k < nk) bits[b] = *reinterpret_cast<const Vec*>(p + (int64_t)(k / VPR) * w + (k % VPR) * N);
      }
#pragma unroll
      for (int b = 0; b < B; ++b) {
        if (k0 + b < nk) {
          T x[N];
          __builtin_memcpy(x, &bits[b], VB);
#pragma unroll
          for (int e = 0; e < N; ++e) sum[OC == 1 ? 0 : ((b % VPR) * N + e) / S] += (Acc)x[e];  // (B % VPR == 0 where OC > 1)
        }
      }
    }
    return;
  }
  for (int r = 0; r < nrows; ++r) {
    const T* q = p + (int64_t)r * w;
    if (full && (reinterpret_cast<uintptr_t>(q) & (VB - 1)) == 0) {
      for (int v0 = 0; v0 < VPR; v0 += B) {  // (B % VPR == 0 where OC > 1: one round)
        Vec bits[B];
#pragma unroll
        for (int b = 0; b < B; ++b)
          if (b < VPR) bits[b] = *reinterpret_cast<const Vec*>(q + (v0 + b) * N);
#pragma unroll
        for (int b = 0; b < B; ++b)
          if (b < VPR) {
            T x[N];
            __builtin_memcpy(x, &bits[b], VB);
#pragma unroll
            for (int e = 0; e < N; ++e) sum[OC == 1 ? 0 : (b * N + e) / S] += (Acc)x[e];
          }
      }
    } else {
#pragma unroll
      for (int j = 0; j < OC; ++j)
        if (j < nj) {
          const int nc = min(S, cols_left - j * S);
          for (int k = 0; k < nc; ++k) sum[j] += (Acc)q[j * S + k];
        }
    }
  }
}

// v[j] = p[j] for j < n, 0 beyond: 16-byte loads for a whole, aligned run
template <int OC>
__device__ __forceinline__ void run_labels(const int32_t* __restrict__ p, int n, int (&v)[OC]) {
  if (OC % 4 == 0 && n == OC && (reinterpret_cast<uintptr_t>(p) & 15) == 0) {
#pragma unroll
    for (int q = 0; q < OC / 4; ++q) {
      const int4 x = *reinterpret_cast<const int4*>(p + 4 * q);
      v[4 * q] = x.x, v[4 * q + 1] = x.y, v[4 * q + 2] = x.z, v[4 * q + 3] = x.w;
    }
  } else {
#pragma unroll
    for (int j = 0; j < OC; ++j) v[j] = j < n ? p[j] : 0;
  }
}

// grid-stride over (t * hk + output row, run of the row)
template <typename T, int S>
__global__ __launch_bounds__(256) void k_overview(const T* __restrict__ image, int64_t chan_stride, int64_t time_stride,
                                                  int n_c, int n_t, int h, int w, int hk, int wk, int cpr, int64_t total,
                                                  MgChannels ch, const int32_t* __restrict__ labels,
                                                  const uint8_t* __restrict__ table, int n_marks, int overlay, double alpha,
                                                  uint8_t* __restrict__ out) {
  using Sh = RunShape<T, S>;
  using Acc = mg_block_acc_t<T>;
  constexpr int OC = Sh::OC;
  const bool small = total <= 0x7FFFFFFFLL;  // (uniform) 32-bit index arithmetic
  const int64_t stride = (int64_t)gridDim.x * 256;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += stride) {
    const MgIndex3 at = mg_split3(i, small, hk, cpr);  // i = (t * hk + Y) * cpr + run of the row
    const int64_t ri = at.row;
    const int t = at.a, Y = at.b, c = at.c;
    const int j0 = c * OC, nj = min(OC, wk - j0);
    const int nrows = min(S, h - Y * S), cols_left = w - j0 * S;
    double acc[OC][3];
#pragma unroll
    for (int j = 0; j < OC; ++j) acc[j][0] = acc[j][1] = acc[j][2] = 0.0;
    for (int k = 0; k < n_c; ++k) {
      const T* p = image + (int64_t)k * chan_stride + (int64_t)t * time_stride + (int64_t)Y * S * w + (int64_t)j0 * S;
      Acc sum[OC];
#pragma unroll
      for (int j = 0; j < OC; ++j) sum[j] = (Acc)0;
      block_sums<T, S, Acc>(p, w, nrows, nj, cols_left, sum);
      const MgChannel c = mg_channel(ch, k);
#pragma unroll
      for (int j = 0; j < OC; ++j)
        if (j < nj) mg_composite_add(c, sum[j], nrows * min(S, cols_left - j * S), acc[j]);
    }
    if (overlay != MG_OVERLAY_NONE) {
      const int32_t* lrow = labels + ri * wk + j0;  // the run's labels; its neighbours only where it holds one
      int lab[OC];
      run_labels<OC>(lrow, nj, lab);
      bool any = false;
#pragma unroll
      for (int j = 0; j < OC; ++j) any |= lab[j] > 0 && lab[j] <= n_marks;
      if (any) {
        int up[OC], down[OC], lf = 0, rt = 0;
        if (overlay == MG_OVERLAY_OUTLINE) {  // (0 outside the picture)
          run_labels<OC>(lrow - wk, Y > 0 ? nj : 0, up);
          run_labels<OC>(lrow + wk, Y + 1 < hk ? nj : 0, down);
          lf = j0 > 0 ? lrow[-1] : 0, rt = j0 + nj < wk ? lrow[nj] : 0;
        }
#pragma unroll
        for (int j = 0; j < OC; ++j)
          if (j < nj && lab[j] > 0 && lab[j] <= n_marks) {
            bool on = true;
            if (overlay == MG_OVERLAY_OUTLINE) {  // an edge of its region: a 4-neighbour with another label
              const int left = j > 0 ? lab[j > 0 ? j - 1 : 0] : lf, right = j + 1 < nj ? lab[j + 1 < OC ? j + 1 : 0] : rt;
              on = up[j] != lab[j] || down[j] != lab[j] || left != lab[j] || right != lab[j];
            }
            if (on) {
              const uint8_t* col = table + ((int64_t)(lab[j] - 1) * n_t + t) * 3;
              mg_overlay_blend(overlay == MG_OVERLAY_FILL ? alpha : 1.0, (double)col[0], (double)col[1], (double)col[2], acc[j]);
            }
          }
      }
    }
    uint8_t* o = out + (ri * wk + j0) * 3;
    uint8_t by[OC * 3];
#pragma unroll
    for (int j = 0; j < OC; ++j)
#pragma unroll
      for (int e = 0; e < 3; ++e) by[3 * j + e] = mg_composite_byte(acc[j][e]);
    if (OC % 4 == 0 && nj == OC && (reinterpret_cast<uintptr_t>(o) & 3) == 0) {  // whole words, as wide as they come
      uint32_t wd[OC % 4 == 0 ? OC * 3 / 4 : 1];
#pragma unroll
      for (int q = 0; q < OC * 3 / 4; ++q)
        wd[q] = (uint32_t)by[4 * q] | ((uint32_t)by[4 * q + 1] << 8) | ((uint32_t)by[4 * q + 2] << 16) |
                ((uint32_t)by[4 * q + 3] << 24);
      if (OC % 8 == 0 && (reinterpret_cast<uintptr_t>(o) & 7) == 0) {
#pragma unroll
        for (int q = 0; q < OC * 3 / 8; ++q) reinterpret_cast<uint2*>(o)[q] = make_uint2(wd[2 * q], wd[2 * q + 1]);
      } else {
#pragma unroll
        for (int q = 0; q < OC * 3 / 4; ++q) reinterpret_cast<uint32_t*>(o)[q] = wd[q];
      }
    } else {
#pragma unroll
      for (int j = 0; j < OC; ++j)
        if (j < nj) o[3 * j] = by[3 * j], o[3 * j + 1] = by[3 * j + 1], o[3 * j + 2] = by[3 * j + 2];
    }
  }
}

template <typename T, int S>
int launch_overview(const void* d_image, int64_t chan_stride, int64_t time_stride, int n_c, int n_t, int h, int w,
                    const MgChannels& ch, const int32_t* d_labels, const uint8_t* d_table, int n_marks, int overlay,
                    double alpha, uint8_t* d_out, hipStream_t s) {
  const int hk = (h + S - 1) / S, wk = (w + S - 1) / S, oc = RunShape<T, S>::OC;
  const int cpr = (wk + oc - 1) / oc;
  const int64_t total = (int64_t)n_t * hk * cpr;
  const int blocks = (int)std::min<int64_t>((total + 255) / 256, MG_OVERVIEW_WALK);
  hipLaunchKernelGGL((k_overview<T, S>), dim3(blocks), dim3(256), 0, s, (const T*)d_image, chan_stride, time_stride, n_c, n_t,
                     h, w, hk, wk, cpr, total, ch, d_labels, d_table, n_marks, overlay, alpha, d_out);
  MG_CHECK_LAUNCH();
  return MG_OK;
}

}  // namespace

extern "C" int mg_roi_image_labels(const uint8_t* d_fg, int64_t mask_stride_m, int64_t mask_stride_t,
                                   const int32_t* d_origin, int m, int n_t, int roi_len, int level, int h, int w,
                                   int32_t* d_labels, void* stream) {
  const MgMaskView fg = {d_fg, mask_stride_m, mask_stride_t};
  if (m < 0 || n_t < 1 || roi_len < 1 || level < 0 || level > MG_OVERVIEW_MAX_LEVEL || h < 1 || w < 1 || !d_labels ||
      fg.stride_m < 0 || fg.stride_t < 0)
    return MG_EINVAL;
  if (m == 0) return MG_OK;  // (no markers: the mask need not exist)
  if (!mg_mask_view_ok(fg) || !d_origin) return MG_EINVAL;
  const int s = 1 << level, hk = (h + s - 1) / s, wk = (w + s - 1) / s, qpr = (roi_len + 3) / 4;
  const int64_t total = (int64_t)m * n_t * roi_len * qpr;
  const int blocks = (int)std::min<int64_t>((total + 255) / 256, MG_IMAGE_LABELS_WALK);
  hipLaunchKernelGGL(k_image_labels, dim3(blocks), dim3(256), 0, mg_stream(stream), fg, d_origin, n_t, roi_len, qpr,
                     level, h, w, hk, wk, total, d_labels);
  MG_CHECK_LAUNCH();
  return MG_OK;
}

extern "C" int mg_render_overview(const void* d_image, int dtype, int64_t chan_stride, int64_t time_stride, int n_c, int n_t,
                                  int h, int w, int level, const double* limits, const double* colors,
                                  const int32_t* d_labels, const uint8_t* d_table, int n_marks, int overlay, double alpha,
                                  uint8_t* d_out, void* stream) {
  if (!d_image || !d_out || !limits || !colors || n_c < 1 || n_c > MG_OVERVIEW_MAX_CHANNELS || n_t < 1 || h < 1 || w < 1 ||
      level < 0 || level > MG_OVERVIEW_MAX_LEVEL || chan_stride < 0 || time_stride < 0 ||
      !mg_overlay_ok(overlay, alpha))
    return MG_EINVAL;
  if (overlay != MG_OVERLAY_NONE && (!d_labels || !d_table || n_marks < 1)) return MG_EINVAL;
  MgChannels ch;
  if (mg_fill_channels(limits, colors, n_c, &ch) != MG_OK) return MG_EINVAL;
  hipStream_t s = mg_stream(stream);
  return mg_dispatch_pixel(dtype, [&](auto t) {
    using T = decltype(t);
#define MG_OV_LEVEL(K)                                                                                                  \
  case K:                                                                                                               \
    return launch_overview<T, (1 << K)>(d_image, chan_stride, time_stride, n_c, n_t, h, w, ch, d_labels, d_table, n_marks, \
                                        overlay, alpha, d_out, s)
    switch (level) {
      MG_OV_LEVEL(0);
      MG_OV_LEVEL(1);
      MG_OV_LEVEL(2);
      MG_OV_LEVEL(3);
      MG_OV_LEVEL(4);
      MG_OV_LEVEL(5);
      MG_OV_LEVEL(6);
    }
#undef MG_OV_LEVEL
    return MG_EINVAL;
  });
}
