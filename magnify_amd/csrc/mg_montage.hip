// plot.roishow ("roishow and percentile contrast limits"): every marker's ROI window side by side as one
// RGB picture per timepoint, the bg mask in red and the fg mask in green on top.  tests/roishow_ref.py restates it in
// NumPy; the kernel is held to it bit for bit.  s = 2^level, lk = ceil(L / s): the side of a cell.
//
// k_roi_montage: one thread per output pixel.  The pixel lies in cell (Y / lk, X / lk) of the layout table, which
// names the marker shown there (-1: an empty cell, written as 0), at block (Y % lk, X % lk) of its window.  Per
// channel the block's in-window pixels are summed -- uint32 for u8 / u16 (64^2 * 65535 < 2^32, exact), float64 for
// float pixels, rows from the top, each from the left -- then mean, (mean - lo) / (hi - lo), clamp, acc += u * colour,
// min(acc, 1): mg_composite_add (mg_composite.h), what mg_render_overview does, on a window.  A row of a block
// starts anywhere (a u16 window row of L = 100 is 200 bytes): elements up to the next 16-byte boundary, whole vectors,
// elements again -- left to right on every path.  Then the masks: a block is on where any mask byte in it is set;
// "outline" keeps the on-blocks with an off 4-neighbour in the cell.  The three bytes are written once.  No LDS.
#include "mg_composite.h"

namespace {

template <typename T, typename Acc>
__device__ __forceinline__ Acc row_sum(const T* __restrict__ q, int nc, Acc sum) {
  constexpr int N = 16 / (int)sizeof(T);
  int k = 0;
  if (nc >= N) {
    const int mis = (int)((reinterpret_cast<uintptr_t>(q) & 15) / sizeof(T));
    const int head = mis ? N - mis : 0;  // (< N <= nc)
    for (; k < head; ++k) sum += (Acc)q[k];
    for (; k + N <= nc; k += N) {
      const uint4 v = *reinterpret_cast<const uint4*>(q + k);
      T x[N];
      __builtin_memcpy(x, &v, 16);
#pragma unroll
      for (int e = 0; e < N; ++e) sum += (Acc)x[e];
    }
  }
  for (; k < nc; ++k) sum += (Acc)q[k];
  return sum;
}

// any byte set in block (by, bx) of the L x L mask at m; a block outside the cell is off.  A row of the block starts
// anywhere: eight bytes, four bytes, then single bytes per load (unaligned loads; the order does not matter to an OR).
__device__ __forceinline__ bool block_on(const uint8_t* __restrict__ m, int L, int lk, int s, int by, int bx) {
  if (by < 0 || bx < 0 || by >= lk || bx >= lk) return false;
  const int y1 = min(L, by * s + s), x0 = bx * s, nc = min(L, x0 + s) - x0;
  for (int y = by * s; y < y1; ++y) {
    const uint8_t* q = m + y * L + x0;
    uint64_t any = 0;
    int k = 0;
    for (; k + 8 <= nc; k += 8) any |= reinterpret_cast<const MgUnaligned64*>(q + k)->v;
    if (k + 4 <= nc) any |= reinterpret_cast<const MgUnaligned32*>(q + k)->v, k += 4;
    for (; k < nc; ++k) any |= q[k];
    if (any) return true;
  }
  return false;
}

template <typename T>
__global__ __launch_bounds__(256) void k_roi_montage(const T* __restrict__ roi, int64_t stride_m, int64_t stride_c,
                                                     int64_t stride_t, int n_marks, int n_c, int L, int level,
                                                     int lk, const int32_t* __restrict__ layout, int cols, int hp, int wp,
                                                     int64_t total, MgChannels ch, MgMaskView bg, MgMaskView fg,
                                                     int overlay, double alpha, uint8_t* __restrict__ out) {
  using Acc = mg_block_acc_t<T>;
  const int s = 1 << level;
  const bool small = total <= 0x7FFFFFFFLL;  // (uniform) 32-bit index arithmetic
  const int64_t stride = (int64_t)gridDim.x * 256;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += stride) {
    const MgIndex3 at = mg_split3(i, small, hp, wp);  // i = (t * hp + Y) * wp + X
    const int t = at.a, Y = at.b, X = at.c;
    const int cr = Y / lk, cc = X / lk, by = Y - cr * lk, bx = X - cc * lk;
    const int g = layout[cr * cols + cc];
    uint8_t* o = out + i * 3;
    if (g < 0 || g >= n_marks) {  // an empty cell (and a table entry that names no marker)
      o[0] = o[1] = o[2] = 0;
      continue;
    }
    const int y0 = by * s, x0 = bx * s, nr = min(s, L - y0), nc = min(s, L - x0), n = nr * nc;
    double acc[3] = {0.0, 0.0, 0.0};
    for (int k = 0; k < n_c; ++k) {
      const T* p = roi + (int64_t)g * stride_m + (int64_t)k * stride_c + (int64_t)t * stride_t + y0 * L + x0;
      Acc sum = (Acc)0;
      for (int r = 0; r < nr; ++r) sum = row_sum<T, Acc>(p + r * L, nc, sum);
      mg_composite_add(mg_channel(ch, k), sum, n, acc);
    }
    if (overlay != MG_OVERLAY_NONE) {
#pragma unroll
      for (int which = 0; which < 2; ++which) {  // bg in red, then fg in green on top
        // (a copy, not a reference: at() through a reference schedules the whole kernel another way; no pointer: no mask)
        const MgMaskView mk = which ? fg : bg;
        if (!mk.p) continue;
        const uint8_t* m = mk.at(g, t);
        bool on = block_on(m, L, lk, s, by, bx);
        if (on && overlay == MG_OVERLAY_OUTLINE)
          on = !(block_on(m, L, lk, s, by - 1, bx) && block_on(m, L, lk, s, by + 1, bx) &&
                 block_on(m, L, lk, s, by, bx - 1) && block_on(m, L, lk, s, by, bx + 1));
        if (on) mg_overlay_blend(overlay == MG_OVERLAY_FILL ? alpha : 1.0, which ? 0.0 : 255.0, which ? 255.0 : 0.0, 0.0, acc);
      }
    }
#pragma unroll
    for (int e = 0; e < 3; ++e) o[e] = mg_composite_byte(acc[e]);
  }
}

}  // namespace

extern "C" int mg_render_roi_montage(const void* d_roi, int dtype, int64_t stride_m, int64_t stride_c, int64_t stride_t,
                                     int n_marks, int n_c, int n_t, int roi_len, int level, const int32_t* d_layout,
                                     int rows, int cols, const double* limits, const double* colors, const uint8_t* d_bg,
                                     int64_t bg_stride_m, int64_t bg_stride_t, const uint8_t* d_fg, int64_t fg_stride_m,
                                     int64_t fg_stride_t, int overlay, double alpha, uint8_t* d_out, void* stream) {
  if (!limits || !colors || n_marks < 0 || n_c < 1 || n_c > MG_OVERVIEW_MAX_CHANNELS || n_t < 1 || roi_len < 1 ||
      roi_len > 32767 || level < 0 || level > MG_OVERVIEW_MAX_LEVEL || rows < 0 || cols < 0 || stride_m < 0 || stride_c < 0 ||
      stride_t < 0 || bg_stride_m < 0 || bg_stride_t < 0 || fg_stride_m < 0 || fg_stride_t < 0 ||
      !mg_overlay_ok(overlay, alpha))
    return MG_EINVAL;
  MgChannels ch;
  if (mg_fill_channels(limits, colors, n_c, &ch) != MG_OK) return MG_EINVAL;
  const int s = 1 << level, lk = (roi_len + s - 1) / s;
  const int64_t hp = (int64_t)rows * lk, wp = (int64_t)cols * lk;
  if (hp > 0x7FFFFFFFLL || wp > 0x7FFFFFFFLL) return MG_EINVAL;
  const int64_t total = (int64_t)n_t * hp * wp;
  if (total == 0) return MG_OK;  // no cells: an empty picture
  if (!d_roi || !d_layout || !d_out || n_marks < 1) return MG_EINVAL;
  const MgMaskView bg = {d_bg, bg_stride_m, bg_stride_t}, fg = {d_fg, fg_stride_m, fg_stride_t};
  const int blocks = (int)std::min<int64_t>((total + 255) / 256, MG_MONTAGE_WALK);
  hipStream_t st = mg_stream(stream);
  return mg_dispatch_pixel(dtype, [&](auto t) {
    using T = decltype(t);
    hipLaunchKernelGGL((k_roi_montage<T>), dim3(blocks), dim3(256), 0, st, (const T*)d_roi, stride_m, stride_c, stride_t, n_marks,
                       n_c, roi_len, level, lk, d_layout, cols, (int)hp, (int)wp, total, ch, bg, fg, overlay, alpha, d_out);
    MG_CHECK_LAUNCH();
    return MG_OK;
  });
}
