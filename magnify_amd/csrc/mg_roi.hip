// A12-A15, A18: ownership labels (utils.py:380-395), ROI windows (utils.py:60-80), fg/bg masks
// and ROI gather (find.py:561-602), masked reductions (README.md:21-22, identify.py:76-80).
//
// Roofline: HBM.  Per marker: L*L*(4 label read + 2 mask write) + C*T*L*L*(2 read + 2 write)
// bytes (u16); the reductions ride along in registers (wavefront shuffles), 0 extra bytes.
#include <math.h>

#include "mg_common.h"
#include "mg_flatcorr.h"

namespace {

constexpr int NT = 256;

// ---- circle_labels as a coverage count -------------------------------------------------------
__global__ __launch_bounds__(NT) void k_circle_labels(const int32_t* __restrict__ d_beads, int64_t bead_cap,
                                                      const int32_t* __restrict__ d_num_beads, int h, int w,
                                                      const int32_t* __restrict__ d_halfwidths, int max_r,
                                                      int32_t* __restrict__ d_labels) {
  const int plane = blockIdx.y;
  const int i = blockIdx.x;
  if (i >= d_num_beads[plane]) return;
  const int32_t* b = d_beads + ((int64_t)plane * bead_cap + i) * 3;
  const int row = b[0], col = b[1], r = b[2];
  if (r < 2 || r > max_r) return;  // undefined in the reference (utils.py:398-430 indexes out of bounds)
  const int32_t* hw = d_halfwidths + (int64_t)r * (2 * max_r + 1);
  int32_t* lab = d_labels + (int64_t)plane * h * w;
  const int side = 2 * r + 1;
  for (int p = threadIdx.x; p < side * side; p += NT) {
    const int dy = p / side - r, dx = p % side - r;
    if (abs(dx) > hw[dy + r]) continue;
    const int y = row + dy, x = col + dx;
    if (y < 0 || y >= h || x < 0 || x >= w) continue;
    int32_t* cell = &lab[(int64_t)y * w + x];
    const int old = atomicCAS(cell, -1, i);
    if (old != -1 && old != i) *cell = -2;  // a second owner: contested
  }
}

// ---- ROI gather + masks + sums ------------------------------------------------------------------
__device__ __forceinline__ void window(int c, int len, int size, int& lo) {
  // utils.py:64-79 with an integer centre.  Whatever the table holds, the window stays inside the image: a centre
  // beyond +-2^28 (nothing an image can hold; what a NaN turns into when it is cast) is pulled in before the sums below
  // could wrap.
  c = min(max(c, -(1 << 28)), 1 << 28);
  int a = c - len / 2, b = c + (len - len / 2);
  if (a < 0) {
    b -= a;
    a = 0;
  }
  if (b > size) a -= b - size;
  lo = a;
}

// fg/bg segmentation straight from the bead table, without the label map: a window pixel is
//   foreground  <=> it lies in this marker's disk and in no other disk   (labels == i,  find.py:580)
//   background  <=> it lies in no disk at all                            (labels == -1, find.py:582)
// which is what circle_labels' "exactly one owner / contested" rule (utils.py:380-395) yields.
// Row bit masks of the window in LDS: any (covered), multi (covered twice or more), own.
struct DiskMasks {
  uint32_t* any;
  uint32_t* multi;
  uint32_t* own;
  int wpr;  // words per window row
  __device__ __forceinline__ void flags(int ry, int rx, uint32_t& f, uint32_t& b) const {
    const int i = ry * wpr + (rx >> 5), sh = rx & 31;
    f = ((own[i] & ~multi[i]) >> sh) & 1u;
    b = (~any[i] >> sh) & 1u;
  }
};

// OR one row span of a disk into the masks (LDS atomics; any thread, any order).
__device__ __forceinline__ void mask_row(const DiskMasks& m, int ry, int xa, int xb, bool is_own) {
  for (int wd = xa >> 5; wd <= (xb >> 5); ++wd) {
    const int lo = max(xa, 32 * wd) - 32 * wd, hi = min(xb, 32 * wd + 31) - 32 * wd;
    const uint32_t bits = (hi - lo == 31) ? 0xFFFFFFFFu : (((1u << (hi - lo + 1)) - 1u) << lo);
    const uint32_t old = atomicOr(&m.any[ry * m.wpr + wd], bits);
    if (old & bits) atomicOr(&m.multi[ry * m.wpr + wd], old & bits);
    if (is_own) atomicOr(&m.own[ry * m.wpr + wd], bits);
  }
}
// Row ry of the window under the disk (yj, xj, rj), if it intersects the window.
__device__ __forceinline__ void mask_disk_row(const DiskMasks& m, int ry, int len, int top, int left, int yj, int xj,
                                              int rj, bool is_own, const int32_t* __restrict__ hwtab, int max_r) {
  const int dy = top + ry - yj;
  if (dy < -rj || dy > rj) return;
  const int hwid = hwtab[(int64_t)rj * (2 * max_r + 1) + dy + rj];
  if (hwid < 0) return;
  const int xa = max(xj - hwid, left) - left, xb = min(xj + hwid, left + len - 1) - left;
  if (xa <= xb) mask_row(m, ry, xa, xb, is_own);
}

constexpr int NBR_CAP = 96;  // disks overlapping one window that are handled row-parallel

__device__ __forceinline__ DiskMasks build_disk_masks(uint32_t* base, int len, int top, int left,
                                                      const int32_t* __restrict__ beads, int nb, int local,
                                                      const int32_t* __restrict__ hwtab, int max_r) {
  __shared__ int s_nn;
  __shared__ int s_nbr[NBR_CAP][3];
  DiskMasks m;
  m.wpr = (len + 31) >> 5;
  const int words = len * m.wpr;
  m.any = base;
  m.multi = base + words;
  m.own = base + 2 * words;
  for (int i = threadIdx.x; i < 3 * words; i += NT) base[i] = 0u;
  if (threadIdx.x == 0) s_nn = 0;
  __syncthreads();
  // 1. scan the assay's bead table for disks that reach into the window (loads issued in batches:
  //    one memory latency per 8 * NT beads); collect them in LDS
  constexpr int UB = 8;
  for (int b0 = 0; b0 < nb; b0 += NT * UB) {
    int yy[UB], xx[UB], rr[UB];
#pragma unroll
    for (int u = 0; u < UB; ++u) {
      const int j = b0 + u * NT + (int)threadIdx.x;
      rr[u] = 0;
      if (j < nb) {
        yy[u] = beads[3 * j];
        xx[u] = beads[3 * j + 1];
        rr[u] = beads[3 * j + 2];
      }
    }
#pragma unroll
    for (int u = 0; u < UB; ++u) {
      const int j = b0 + u * NT + (int)threadIdx.x;
      const int yj = yy[u], xj = xx[u], rj = rr[u];
      if (rj < 2 || rj > max_r) continue;  // undefined in the reference, no coverage (as k_circle_labels)
      if (yj + rj < top || yj - rj >= top + len || xj + rj < left || xj - rj >= left + len) continue;
      const int k = atomicAdd(&s_nn, 1);
      if (k < NBR_CAP) {
        s_nbr[k][0] = yj;
        s_nbr[k][1] = xj;
        s_nbr[k][2] = rj | (j == local ? 0x10000 : 0);
      } else {  // an extremely crowded window: this thread draws the whole disk itself
        for (int ry = max(yj - rj, top) - top; ry <= min(yj + rj, top + len - 1) - top; ++ry)
          mask_disk_row(m, ry, len, top, left, yj, xj, rj, j == local, hwtab, max_r);
      }
    }
  }
  __syncthreads();
  // 2. one (disk, row) pair per thread
  const int nn = min(s_nn, NBR_CAP), side = 2 * max_r + 1;
  for (int p = threadIdx.x; p < nn * side; p += NT) {
    const int k = p / side, dyi = p - k * side - max_r;
    const int yj = s_nbr[k][0], xj = s_nbr[k][1], rj = s_nbr[k][2] & 0xFFFF;
    const int ry = yj + dyi - top;
    if (dyi < -rj || dyi > rj || ry < 0 || ry >= len) continue;
    mask_disk_row(m, ry, len, top, left, yj, xj, rj, (s_nbr[k][2] & 0x10000) != 0, hwtab, max_r);
  }
  __syncthreads();
  return m;
}

inline __host__ __device__ int mask_words(int len) { return 3 * len * ((len + 31) >> 5); }
inline size_t roi_lds_bytes(int len, bool disks) {
  const size_t fl = ((size_t)len * len + 3) & ~(size_t)3;
  return fl + (disks ? (size_t)3 * len * ((len + 31) >> 5) * 4 : 0);
}

// The assay of marker g in the assays' concatenated tables = the last one that starts at or before it (empty assays
// have empty ranges).
__device__ __forceinline__ int roi_assay_of(const int32_t* __restrict__ d_assay_offsets, int n_assays, int g) {
  int lo = 0, hi = n_assays;
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (d_assay_offsets[mid] <= g) lo = mid;
    else hi = mid;
  }
  return lo;
}

// The marker a workgroup of the window kernels takes: of a flat list with per-marker assay / local index (label mode),
// or of the assays' concatenated bead tables (disk mode).
struct RoiMarker {
  int g, assay, first, local;  // marker (row of the outputs), its assay, the assay's first marker, index in the assay
  int64_t bead0, gb;           // the assay's first bead / this marker's bead in d_beads
};
// false: nothing to do for this workgroup
__device__ __forceinline__ bool roi_marker(const int32_t* __restrict__ d_assay_offsets, int n_assays, int64_t bead_stride,
                                           const int32_t* __restrict__ d_order,
                                           const int32_t* __restrict__ d_marker_assay,
                                           const int32_t* __restrict__ d_marker_local, RoiMarker& mk) {
  int g = blockIdx.x;
  mk.first = 0;
  mk.bead0 = 0;
  mk.gb = g;
  if (d_assay_offsets) {
    // flat grid over the markers of all assays (the launch may be sized by an upper bound: the rest leaves at once)
    if (g >= d_assay_offsets[n_assays]) return false;
    if (d_order) g = d_order[g];  // the order the windows are visited in (mg_roi_window_order); outputs stay in place
    mk.assay = roi_assay_of(d_assay_offsets, n_assays, g);
    mk.first = d_assay_offsets[mk.assay];
    mk.local = g - mk.first;
    // bead table: compact (markers and beads share the index) or one padded row per assay
    mk.bead0 = bead_stride ? (int64_t)mk.assay * bead_stride : mk.first;
    mk.gb = mk.bead0 + mk.local;
  } else {
    mk.assay = d_marker_assay ? d_marker_assay[g] : 0;
    mk.local = d_marker_local ? d_marker_local[g] : g;
  }
  mk.g = g;
  return true;
}

// The window's fg / bg pixel counts: per-thread counts -> d_counts[g] (a workgroup of four waves).  Ends behind a
// barrier: what the workgroup wrote to LDS before the call is complete, too.
__device__ __forceinline__ void roi_store_counts(int cf, int cb, int (&s_cnt)[2][NT / 64], int g,
                                                 int32_t* __restrict__ d_counts) {
  cf = mg_wave_sum_i32(cf);
  cb = mg_wave_sum_i32(cb);
  if ((threadIdx.x & 63) == 0) {
    s_cnt[0][threadIdx.x >> 6] = cf;
    s_cnt[1][threadIdx.x >> 6] = cb;
  }
  __syncthreads();
  if (threadIdx.x == 0 && d_counts) {
    d_counts[2 * (int64_t)g] = s_cnt[0][0] + s_cnt[0][1] + s_cnt[0][2] + s_cnt[0][3];
    d_counts[2 * (int64_t)g + 1] = s_cnt[1][0] + s_cnt[1][1] + s_cnt[1][2] + s_cnt[1][3];
  }
}

template <typename T, typename ACC>
__global__ __launch_bounds__(NT) void k_roi(const T* __restrict__ d_image, int64_t assay_stride, int n_c, int n_t, int h,
                                            int w, const int32_t* __restrict__ d_beads,
                                            const int32_t* __restrict__ d_marker_assay,
                                            const int32_t* __restrict__ d_marker_local, int len,
                                            const int32_t* __restrict__ d_labels,
                                            const int32_t* __restrict__ d_assay_offsets, int n_assays, int64_t bead_stride, int time_major,
                                            const int32_t* __restrict__ d_order,
                                            const int32_t* __restrict__ d_halfwidths, int max_r, T* __restrict__ d_roi,
                                            uint8_t* __restrict__ d_fg, uint8_t* __restrict__ d_bg,
                                            double* __restrict__ d_sums, int32_t* __restrict__ d_counts) {
  extern __shared__ __attribute__((aligned(4))) uint8_t flags[];
  __shared__ ACC s_red[2][NT / 64];
  __shared__ int s_cnt[2][NT / 64];
  RoiMarker mk;  // one block per marker
  if (!roi_marker(d_assay_offsets, n_assays, bead_stride, d_order, d_marker_assay, d_marker_local, mk)) return;
  const int g = mk.g, assay = mk.assay, first = mk.first, local = mk.local;
  const int64_t bead0 = mk.bead0, gb = mk.gb;
  const int cy = d_beads[3 * gb], cx = d_beads[3 * gb + 1];
  int top, left;
  window(cy, len, h, top);
  window(cx, len, w, left);
  const int n = len * len;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  // masks from the label map (find.py:580-584) or straight from the assay's bead table
  const int32_t* lab = d_labels ? d_labels + (int64_t)assay * h * w : nullptr;
  DiskMasks dm{};
  if (d_halfwidths)
    dm = build_disk_masks(reinterpret_cast<uint32_t*>(flags + ((n + 3) & ~3)), len, top, left,
                          d_beads + 3 * bead0, d_assay_offsets[assay + 1] - first, local, d_halfwidths, max_r);
  int cf = 0, cb = 0;
  for (int p = threadIdx.x; p < n; p += NT) {
    const int ry = p / len, rx = p - ry * len;
    uint8_t f = 0, b = 0;
    if (d_halfwidths) {
      uint32_t ff, bb;
      dm.flags(ry, rx, ff, bb);
      f = (uint8_t)ff;
      b = (uint8_t)bb;
    } else if (lab) {
      const int v = lab[(int64_t)(top + ry) * w + (left + rx)];
      f = v == local;
      b = v == -1;
    }
    flags[p] = f | (b << 1);
    if (d_fg) d_fg[(int64_t)g * n + p] = f;
    if (d_bg) d_bg[(int64_t)g * n + p] = b;
    cf += f;
    cb += b;
  }
  roi_store_counts(cf, cb, s_cnt, g, d_counts);
  // gather every (channel, time) window (find.py:589-602) and reduce under the masks
  const T* img = d_image + (int64_t)assay * assay_stride;
  for (int ct = 0; ct < n_c * n_t; ++ct) {
    // outputs are (channel, time)-ordered; the image block may be stored time-major (t, c, h, w)
    const T* plane = img + (int64_t)(time_major ? (ct % n_t) * n_c + ct / n_t : ct) * h * w;
    T* out = d_roi ? d_roi + ((int64_t)g * n_c * n_t + ct) * n : nullptr;
    ACC sf = 0, sb = 0;
    for (int p = threadIdx.x; p < n; p += NT) {
      const int ry = p / len, rx = p - ry * len;
      const T v = plane[(int64_t)(top + ry) * w + (left + rx)];
      if (out) out[p] = v;
      const uint8_t fl = flags[p];
      if (fl & 1) sf += (ACC)v;
      if (fl & 2) sb += (ACC)v;
    }
    if (d_sums) {
#pragma unroll
      for (int off = 32; off > 0; off >>= 1) {
        sf += __shfl_xor(sf, off);
        sb += __shfl_xor(sb, off);
      }
      __syncthreads();
      if (lane == 0) {
        s_red[0][wave] = sf;
        s_red[1][wave] = sb;
      }
      __syncthreads();
      if (threadIdx.x == 0) {
        double* o = d_sums + ((int64_t)g * n_c * n_t + ct) * 2;
        o[0] = (double)(s_red[0][0] + s_red[0][1] + s_red[0][2] + s_red[0][3]);
        o[1] = (double)(s_red[1][0] + s_red[1][1] + s_red[1][2] + s_red[1][3]);
      }
    }
  }
}

// ---- fast path: uint16 image, even window length <= 126, even image width -------------------------
// One wave per window row, one dword (2 pixels) per lane: aligned 4-byte loads (odd source offsets are funnel-shifted
// from the neighbouring lane's dword, fetched by a whole-wave DPP shift), 4-byte roi stores, 2-byte mask stores.
// The masks live in LDS as two BIT rows per window row (fg, bg); a lane turns its two bits into the 0/1 halves of a
// packed-u16 multiplier once per row and applies it to CTB (channel, time) planes at a time: one v_dot2_u32_u16 per
// dword and mask.  All sums fit 32 bits (126^2 pixels x 65535 < 2^32) up to the final conversion.
// (Before: byte flags in LDS and four conditional 64-bit adds per dword -- 53 wave-instructions per row and plane,
// the VALU 85 % busy at the HBM ceiling.)
typedef unsigned short roi_us2 __attribute__((ext_vector_type(2)));

__device__ __forceinline__ uint32_t roi_dot2(uint32_t v, uint32_t m, uint32_t acc) {
  return __builtin_amdgcn_udot2(__builtin_bit_cast(roi_us2, v), __builtin_bit_cast(roi_us2, m), acc, false);
}
// bits 0, 1 of b -> the 0/1 halves of a packed pair
__device__ __forceinline__ uint32_t roi_pair(uint32_t b) { return (b & 1u) | ((b & 2u) << 15); }

// FUSE (mg_roi_segment_reduce_raw): the channels of `rw.chan_mask` have no corrected copy in the image block -- their
// dwords come from the raw stack at the same coordinates and are flat-field corrected here, with the functions the
// correction pass itself uses (mg_flatcorr.h), before they are shifted, stored and summed; the other channels are read
// from the image block as they are.  The flat pair of a lane's dword is loaded once per window row (beside the pixel
// loads, so it rides in the same software pipeline) and its factors rk = rcp(flat) * (M1 / M2) are made once per row
// for all raw channels: the planes of an assay share one group of maxima.  FUSE 1: an integer-valued scalar dark
// (subtracted in the integer domain, two pixels per instruction), 2: any scalar dark.
struct RoiRaw {
  const uint16_t* raw;   // the uncorrected stack, laid out as the image block (same assay stride)
  const float* flat;     // float32 flat image (h, w), or nullptr: the scalar flat_s
  const double* max2;    // double[groups][2], the maxima of the correction's pass 1
  double flat_s, dark;
  int planes_per_group;  // a multiple of n_c * n_t: the planes of an assay share one group
  uint32_t chan_mask;    // bit c: channel c is gathered from the raw stack
};

// the two pixels of a dword through the correction
template <bool INT_DARK>
__device__ __forceinline__ uint32_t roi_correct_dword(uint32_t d, uint32_t dark_i, double dark, const double (&fl)[2],
                                                      const double (&rk)[2], bool rk_bad,
                                                      const double* __restrict__ d_max2, int group) {
  const uint16_t x[2] = {(uint16_t)(d & 0xFFFFu), (uint16_t)(d >> 16)};
  const double dk[2] = {dark, dark};
  uint16_t o[2];
  correct_chunk_rk<uint16_t, 2, INT_DARK>(x, dark_i, dk, fl, rk, rk_bad, d_max2, group, 1, o);
  return (uint32_t)o[0] | ((uint32_t)o[1] << 16);
}

// Registers: 62 VGPRs / 8 waves per SIMD without FUSE; the float64 correction brings the fused variants to 97 (4 waves)
// when the compiler is left alone, 89 without scratch when asked for 5 -- asked for 6 it spills 11 registers.  The
// hint leaves the plain variant's code as it was.
template <int FUSE>
__global__ __launch_bounds__(NT) __attribute__((amdgpu_waves_per_eu(5, 8))) void k_roi_u16_even(const uint16_t* __restrict__ d_image, int64_t assay_stride,
                                                     int n_c, int n_t, int h, int w,
                                                     const int32_t* __restrict__ d_beads,
                                                     const int32_t* __restrict__ d_marker_assay,
                                                     const int32_t* __restrict__ d_marker_local, int len,
                                                     const int32_t* __restrict__ d_labels,
                                                     const int32_t* __restrict__ d_assay_offsets, int n_assays, int64_t bead_stride, int time_major,
                                                     const int32_t* __restrict__ d_order,
                                                     const int32_t* __restrict__ d_halfwidths, int max_r,
                                                     uint16_t* __restrict__ d_roi, uint8_t* __restrict__ d_fg,
                                                     uint8_t* __restrict__ d_bg, double* __restrict__ d_sums,
                                                     int32_t* __restrict__ d_counts, RoiRaw rw) {
  extern __shared__ __attribute__((aligned(4))) uint8_t smem[];  // three bit-row arrays of len x wpr words
  constexpr int WV = NT / 64;
  constexpr int U = 2, CTB = 4;  // window rows per wave and (channel, time) planes per trip (alternatives: roi_dispatch)
  __shared__ uint32_t s_red[2][CTB][WV];
  __shared__ int s_cnt[2][WV];
  RoiMarker mk;  // one block per marker
  if (!roi_marker(d_assay_offsets, n_assays, bead_stride, d_order, d_marker_assay, d_marker_local, mk)) return;
  const int g = mk.g, assay = mk.assay, first = mk.first, local = mk.local;
  const int64_t bead0 = mk.bead0, gb = mk.gb;
  int top, left;
  window(d_beads[3 * gb], len, h, top);
  window(d_beads[3 * gb + 1], len, w, left);
  const int n = len * len, half = len >> 1;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int x = 2 * lane;
  const bool act = lane < half;
  const int wpr = (len + 31) >> 5, words = len * wpr;
  uint32_t* base = reinterpret_cast<uint32_t*>(smem);
  uint32_t* fgw = base + 2 * words;  // (disk mode: `own`, narrowed in place)
  uint32_t* bgw = base;              // (disk mode: `any`, complemented in place)
  int cf = 0, cb = 0;
  if (d_halfwidths) {
    const DiskMasks dm = build_disk_masks(base, len, top, left, d_beads + 3 * bead0, d_assay_offsets[assay + 1] - first,
                                          local, d_halfwidths, max_r);
    // fg = own and not contested, bg = covered by nobody (the bits of a row's last word beyond the window stay 0)
    for (int i = threadIdx.x; i < words; i += NT) {
      const int wd = i % wpr;
      const uint32_t valid = (len - 32 * wd >= 32) ? 0xFFFFFFFFu : ((1u << (len - 32 * wd)) - 1u);
      const uint32_t f = dm.own[i] & ~dm.multi[i], b = ~dm.any[i] & valid;
      fgw[i] = f;
      bgw[i] = b;
      cf += __popc(f);
      cb += __popc(b);
    }
  } else {
    for (int i = threadIdx.x; i < 3 * words; i += NT) base[i] = 0u;
    __syncthreads();
    if (d_labels) {
      const int32_t* lab = d_labels + (int64_t)assay * h * w;
      for (int ry = wave; ry < len; ry += WV) {
        if (!act) continue;
        const int32_t* lp = lab + (int64_t)(top + ry) * w + left + x;
        const int v0 = lp[0], v1 = lp[1];
        const uint32_t f = (uint32_t)(v0 == local) | ((uint32_t)(v1 == local) << 1);
        const uint32_t b = (uint32_t)(v0 == -1) | ((uint32_t)(v1 == -1) << 1);
        if (f) atomicOr(&fgw[ry * wpr + (x >> 5)], f << (x & 31));
        if (b) atomicOr(&bgw[ry * wpr + (x >> 5)], b << (x & 31));
        cf += __popc(f);
        cb += __popc(b);
      }
    }
  }
  roi_store_counts(cf, cb, s_cnt, g, d_counts);  // (its barrier completes the bit rows)
  const int mword = x >> 5, msh = x & 31;  // this lane's two bits inside a bit row
  if (d_fg || d_bg) {
    for (int ry = wave; ry < len; ry += WV) {
      if (!act) continue;
      const uint32_t f = (fgw[ry * wpr + mword] >> msh) & 3u, b = (bgw[ry * wpr + mword] >> msh) & 3u;
      if (d_fg) *reinterpret_cast<uint16_t*>(&d_fg[(int64_t)g * n + ry * len + x]) = (uint16_t)((f & 1u) | ((f & 2u) << 7));
      if (d_bg) *reinterpret_cast<uint16_t*>(&d_bg[(int64_t)g * n + ry * len + x]) = (uint16_t)((b & 1u) | ((b & 2u) << 7));
    }
  }
  const uint16_t* img = d_image + (int64_t)assay * assay_stride;
  const int nct = n_c * n_t;
  // w is even: every row of the window starts at the same parity.  An odd start is read from one element before
  // (aligned dwords) and funnel-shifted; its last dword then ends one element behind the window -- inside the image
  // row, because left + len == w would make left even.
  const int odd = left & 1;
  const uint32_t shift = odd ? 16u : 0u;
  const uint32_t lidx = (uint32_t)min(lane, half - 1 + odd);  // idle lanes repeat the last dword: no branch around a load
  const int64_t plane_elems = (int64_t)h * w;
  // FUSE: the assay's group of maxima, its quotient and whether the fast path holds for it (uniform, once)
  const int group = FUSE ? (int)(((int64_t)assay * nct) / rw.planes_per_group) : 0;
  double kk = 1.0;
  bool group_ok = false;
  if (FUSE) {
    group_ok = group_quotient(rw.max2[2 * group], rw.max2[2 * group + 1], kk);
    kk = uniform_f64(kk);
  }
  const uint32_t dark_i = FUSE == 1 ? (uint32_t)rw.dark : 0u;
  const uint16_t* rawimg = FUSE ? rw.raw + (int64_t)assay * assay_stride : nullptr;
  for (int ct0 = 0; ct0 < nct; ct0 += CTB) {
    // outputs are (channel, time)-ordered; the image block may be stored time-major (t, c, h, w)
    const uint32_t* plane[CTB];
    uint32_t* out[CTB];
    uint32_t raw_c = 0u;  // FUSE: which of this trip's planes are raw (the launcher refuses time_major)
#pragma unroll
    for (int c = 0; c < CTB; ++c) {
      const int ct = min(ct0 + c, nct - 1);
      const bool is_raw = FUSE && ((rw.chan_mask >> (ct / n_t)) & 1u);
      raw_c |= is_raw ? (1u << c) : 0u;
      plane[c] = reinterpret_cast<const uint32_t*>((is_raw ? rawimg : img) + (int64_t)(time_major ? (ct % n_t) * n_c + ct / n_t : ct) * plane_elems);
      out[c] = d_roi ? reinterpret_cast<uint32_t*>(d_roi + ((int64_t)g * nct + ct) * n) : nullptr;
    }
    uint32_t sf[CTB], sb[CTB];
#pragma unroll
    for (int c = 0; c < CTB; ++c) sf[c] = 0u, sb[c] = 0u;
    // U rows x CTB planes per trip and wave, software-pipelined: the loads of the NEXT trip are issued before this
    // trip's dwords are shifted, stored and summed (the gather is latency-bound otherwise: a wave would sit out a
    // full load round trip, and the write acknowledgements of its stores, between two batches of requests)
    // (FUSE: ff = the flat values of the dword's two pixels -- the pair before the funnel shift, 8-byte aligned)
    auto load_rows = [&](int r0, uint32_t (&dd)[U][CTB], float2 (&ff)[U]) {
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const int ry = min(r0 + u * WV, len - 1);
        const uint32_t di = (uint32_t)(((top + ry) * w + left - odd) >> 1) + lidx;  // dword index in the plane (h w < 2^31)
#pragma unroll
        for (int c = 0; c < CTB; ++c) dd[u][c] = plane[c][di];
        if (FUSE && rw.flat) ff[u] = reinterpret_cast<const float2*>(rw.flat)[di];
      }
    };
    uint32_t dd[U][CTB], dn[U][CTB];
    float2 ff[U], fn[U];
    load_rows(wave, dd, ff);
    for (int r0 = wave; r0 < len; r0 += WV * U) {
      load_rows(r0 + WV * U, dn, fn);  // (rows beyond the window repeat its last row: no branch)
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const int ry = r0 + u * WV;
        if (ry >= len) break;  // wave-uniform
        const uint32_t mf = roi_pair((fgw[ry * wpr + mword] >> msh) & 3u), mb = roi_pair((bgw[ry * wpr + mword] >> msh) & 3u);
        const uint32_t oi = (uint32_t)(ry * half + lane);
        double fl[2], rk[2];
        bool rk_bad = false;
        if (FUSE && raw_c) {  // the row's factors, shared by its raw planes
          fl[0] = rw.flat ? (double)ff[u].x : rw.flat_s;
          fl[1] = rw.flat ? (double)ff[u].y : rw.flat_s;
          const double rr[2] = {refined_rcp(fl[0]), refined_rcp(fl[1])};
          const bool rk_large = chunk_factors<2>(rr, kk, rk);
          rk_bad = rk_large || rr[0] == 0.0 || rr[1] == 0.0 || !group_ok;
        }
#pragma unroll
        for (int c = 0; c < CTB; ++c) {
          if (ct0 + c >= nct) break;  // uniform
          uint32_t d = dd[u][c];
          if (FUSE && ((raw_c >> c) & 1u))  // (uniform; every lane, idle ones too: the shift below reads lane + 1)
            d = roi_correct_dword<FUSE == 1>(d, dark_i, rw.dark, fl, rk, rk_bad, rw.max2, group);
          const uint32_t nx = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)d, 0x130, 0xF, 0xF, false);  // lane + 1
          const uint32_t v = __builtin_amdgcn_alignbit(nx, d, shift);
          if (act) {
            if (out[c]) out[c][oi] = v;
            sf[c] = roi_dot2(v, mf, sf[c]);
            sb[c] = roi_dot2(v, mb, sb[c]);
          }
        }
      }
#pragma unroll
      for (int u = 0; u < U; ++u)
#pragma unroll
        for (int c = 0; c < CTB; ++c) dd[u][c] = dn[u][c];
      if (FUSE) {
#pragma unroll
        for (int u = 0; u < U; ++u) ff[u] = fn[u];
      }
    }
    if (d_sums) {
#pragma unroll
      for (int c = 0; c < CTB; ++c) {
        const uint32_t a = (uint32_t)mg_wave_scan_incl_i32((int)sf[c]), b = (uint32_t)mg_wave_scan_incl_i32((int)sb[c]);
        if (lane == 63) {
          s_red[0][c][wave] = a;
          s_red[1][c][wave] = b;
        }
      }
      __syncthreads();
      if ((int)threadIdx.x < 2 * CTB) {
        const int k = threadIdx.x & 1, c = threadIdx.x >> 1;
        if (ct0 + c < nct) {
          uint32_t tot = 0;
#pragma unroll
          for (int q = 0; q < WV; ++q) tot += s_red[k][c][q];
          d_sums[((int64_t)g * nct + ct0 + c) * 2 + k] = (double)tot;
        }
      }
      __syncthreads();
    }
  }
}

// ---- host side of the ROI pass ---------------------------------------------------------------------------------------
// What one call of the pass is given: the entry points fill it, roi_dispatch chooses the kernel.
struct RoiCall {
  const void* d_image;
  int dtype;
  int64_t assay_stride;
  int n_c, n_t, h, w;
  const int32_t* d_beads;
  int64_t bead_stride;
  const int32_t *d_marker_assay, *d_marker_local;  // label mode: per-marker assay / index in the assay
  int m, len;
  const int32_t* d_labels;
  const int32_t* d_assay_offsets;  // disk mode: where every assay's markers start
  int n_assays, time_major;
  const int32_t *d_order, *d_halfwidths;
  int max_r;
  void* d_roi;
  uint8_t *d_fg, *d_bg;
  double* d_sums;
  int32_t* d_counts;
  hipStream_t stream;
};

// The window kernels' parameter list (k_roi<T, ACC> and k_roi_u16_even<...> share it; `raw` = the RoiRaw of the
// latter), one workgroup per marker.
template <typename T, typename K, typename... Raw>
int roi_launch(K kernel, size_t lds, const RoiCall& c, Raw... raw) {
  hipLaunchKernelGGL(kernel, dim3(c.m), dim3(NT), lds, c.stream, (const T*)c.d_image, c.assay_stride, c.n_c, c.n_t, c.h,
                     c.w, c.d_beads, c.d_marker_assay, c.d_marker_local, c.len, c.d_labels, c.d_assay_offsets, c.n_assays,
                     c.bead_stride, c.time_major, c.d_order, c.d_halfwidths, c.max_r, (T*)c.d_roi, c.d_fg, c.d_bg, c.d_sums,
                     c.d_counts, raw...);
  MG_CHECK_LAUNCH();
  return MG_OK;
}

inline bool aligned(const void* p, uintptr_t bytes) { return (reinterpret_cast<uintptr_t>(p) & (bytes - 1)) == 0; }

// Can the uint16 even-window kernels take this call?  A lane works on dwords: uint16, an even window of at most 126
// (a row's dwords fit one wave), dword indices below 2^31, dword stores to d_roi and 2-byte stores to the masks.  What
// differs between the branches:
//   fast   (k_roi_u16_even)        image_align 4,  w_div 2, stride_div 2: every plane and row starts on a dword
//   fused  (k_roi_u16_even, FUSE)  image_align 16, w_div 2, stride_div 8: every assay starts on 16 bytes, in the image
//                                  block and in the raw stack alike (its other bases: roi_dispatch)
bool roi_u16_even_ok(const RoiCall& c, int image_align, int w_div, int stride_div) {
  return c.dtype == MG_U16 && (c.len & 1) == 0 && c.len <= 126 && (c.w & (w_div - 1)) == 0 &&
         (c.assay_stride & (stride_div - 1)) == 0 && (int64_t)c.h * c.w < (1LL << 31) && aligned(c.d_image, image_align) &&
         aligned(c.d_roi, 4) && aligned(c.d_fg, 2) && aligned(c.d_bg, 2);
}

// Argument checks, then the first branch that takes the call: fused (`fuse` given: it or a refusal), fast, generic.
int roi_dispatch(const RoiCall& c, const RoiRaw* fuse = nullptr) {
  if (!c.d_image || !c.d_beads || c.m < 0 || c.len <= 0 || c.n_c <= 0 || c.n_t <= 0) return MG_EINVAL;
  // (the LDS bound is the generic kernel's; windows beyond it are refused whichever kernel would run)
  if (c.len > c.h || c.len > c.w || roi_lds_bytes(c.len, c.d_halfwidths != nullptr) > 60000) return MG_EINVAL;
  if (c.m == 0) return MG_OK;
  const size_t bit_rows = (size_t)mask_words(c.len) * 4;  // LDS of k_roi_u16_even
  if (fuse) {
    // one geometry for the raw stack and the image block; anything the kernel does not take is refused (the caller
    // corrects the channels with the correction pass and gathers as usual)
    if (!roi_u16_even_ok(c, 16, 2, 8) || c.time_major || !fuse->raw || !fuse->max2 || c.n_c > 31 ||
        (fuse->chan_mask >> c.n_c) || fuse->planes_per_group <= 0 || fuse->planes_per_group % (c.n_c * c.n_t) ||
        !aligned(fuse->raw, 16) || !aligned(fuse->flat, 16) || !aligned(fuse->max2, 8))
      return MG_EINVAL;
    if (dark_is_int(nullptr, fuse->dark)) return roi_launch<uint16_t>(k_roi_u16_even<1>, bit_rows, c, *fuse);
    return roi_launch<uint16_t>(k_roi_u16_even<2>, bit_rows, c, *fuse);
  }
  // 2 rows x 4 planes per trip, next trip's loads in flight while this one is worked on (measured at 16 x 4 x 4096^2:
  // 1.14 ms; without the pipelining 1.22, one row per trip 1.22, 4 rows x 2 planes 1.20, 4 x 4 unpipelined 1.24)
  if (roi_u16_even_ok(c, 4, 2, 2)) return roi_launch<uint16_t>(k_roi_u16_even<0>, bit_rows, c, RoiRaw{});
  return mg_dispatch_pixel(c.dtype, [&](auto t) {
    using T = decltype(t);
    return roi_launch<T>(k_roi<T, mg_acc_t<T>>, roi_lds_bytes(c.len, c.d_halfwidths != nullptr), c);
  });
}

}  // namespace

extern "C" int mg_circle_labels(const int32_t* d_beads, int64_t bead_cap, const int32_t* d_num_beads, int n_planes,
                                int h, int w, const int32_t* d_halfwidths, int max_r, int32_t* d_labels,
                                void* stream) {
  if (!d_beads || !d_num_beads || !d_halfwidths || !d_labels || n_planes < 0 || n_planes > 65535 || bead_cap < 0 ||
      max_r < 0)
    return MG_EINVAL;
  if (n_planes == 0 || bead_cap == 0) return MG_OK;
  hipLaunchKernelGGL(k_circle_labels, dim3((unsigned)bead_cap, n_planes), dim3(NT), 0, mg_stream(stream), d_beads,
                     bead_cap, d_num_beads, h, w, d_halfwidths, max_r, d_labels);
  MG_CHECK_LAUNCH();
  return MG_OK;
}

namespace {
// d_offsets[0 .. n] = exclusive prefix of min(d_counts[i], cap): where every assay's markers start in the compact
// outputs of mg_roi_segment_reduce -- on the device, so that the pass can be queued before the host has seen the counts.
__global__ __launch_bounds__(1024) void k_counts_to_offsets(const int32_t* __restrict__ d_counts, int n, int cap,
                                                            int32_t* __restrict__ d_offsets) {
  int carry = 0;
  for (int i0 = 0; i0 < n; i0 += 1024) {  // block-uniform trip count
    const int i = i0 + (int)threadIdx.x;
    const int v = i < n ? min(max(d_counts[i], 0), cap) : 0;
    int total;
    const int ex = mg_block_exscan(v, &total);
    if (i < n) d_offsets[i] = carry + ex;
    carry += total;
  }
  if (threadIdx.x == 0) d_offsets[n] = carry;
}
}  // namespace

extern "C" int mg_counts_to_offsets(const int32_t* d_counts, int n, int cap, int32_t* d_offsets, void* stream) {
  if (!d_counts || !d_offsets || n < 0 || cap < 0) return MG_EINVAL;
  hipLaunchKernelGGL(k_counts_to_offsets, dim3(1), dim3(1024), 0, mg_stream(stream), d_counts, n, cap, d_offsets);
  MG_CHECK_LAUNCH();
  return MG_OK;
}

namespace {
// One row per marker: [assay, row, col, r, fg_count, bg_count, fg_sum[C], bg_sum[C]] (float64: exact for these
// integers) from the bead tables and the ROI pass's counts / sums where they are -- what a rank contributes to the
// all-gather of the marker table (collective 3).
__global__ __launch_bounds__(256) void k_marker_table(const int32_t* __restrict__ d_beads, int64_t bead_stride,
                                                      const int32_t* __restrict__ d_assay_offsets, int n_assays,
                                                      int assay_offset, const int32_t* __restrict__ d_counts,
                                                      const double* __restrict__ d_sums, int n_c, int n_t, int t_index,
                                                      double* __restrict__ d_table) {
  const int total = d_assay_offsets[n_assays];
  const int width = 6 + 2 * n_c;
  for (int g = blockIdx.x * blockDim.x + threadIdx.x; g < total; g += gridDim.x * blockDim.x) {
    const int lo = roi_assay_of(d_assay_offsets, n_assays, g);
    const int local = g - d_assay_offsets[lo];
    const int32_t* b = bead_stride > 0 ? d_beads + ((int64_t)lo * bead_stride + local) * 3 : d_beads + (int64_t)g * 3;
    double* row = d_table + (int64_t)g * width;
    row[0] = (double)(assay_offset + lo);
    row[1] = (double)b[0], row[2] = (double)b[1], row[3] = (double)b[2];
    row[4] = (double)d_counts[2 * g], row[5] = (double)d_counts[2 * g + 1];
    for (int c = 0; c < n_c; ++c) {
      const double* sm = d_sums + (((int64_t)g * n_c + c) * n_t + t_index) * 2;
      row[6 + c] = sm[0];
      row[6 + n_c + c] = sm[1];
    }
  }
}
}  // namespace

extern "C" int mg_marker_table(const int32_t* d_beads, int64_t bead_stride, const int32_t* d_assay_offsets, int n_assays,
                               int m, int assay_offset, const int32_t* d_counts, const double* d_sums, int n_c, int n_t,
                               int t_index, double* d_table, void* stream) {
  if (!d_assay_offsets || n_assays <= 0 || n_assays > 65535 || m < 0 || bead_stride < 0 || n_c <= 0 || n_t <= 0 ||
      t_index < 0 || t_index >= n_t)
    return MG_EINVAL;
  if (m == 0) return MG_OK;
  if (!d_beads || !d_counts || !d_sums || !d_table) return MG_EINVAL;
  hipLaunchKernelGGL(k_marker_table, dim3((unsigned)std::min((m + 255) / 256, MG_MARKER_TABLE_WALK)), dim3(256), 0, mg_stream(stream),
                     d_beads, bead_stride, d_assay_offsets, n_assays, assay_offset, d_counts, d_sums, n_c, n_t, t_index,
                     d_table);
  MG_CHECK_LAUNCH();
  return MG_OK;
}

extern "C" int mg_roi_gather_reduce_batched(const void* d_image, int dtype, int64_t assay_stride, int n_c, int n_t,
                                            int h, int w, const int32_t* d_beads, const int32_t* d_marker_assay,
                                            const int32_t* d_marker_local, int m, int roi_len,
                                            const int32_t* d_labels, void* d_roi, uint8_t* d_fg, uint8_t* d_bg,
                                            double* d_sums, int32_t* d_counts, void* stream) {
  // label mode: no assay offsets, window order or half-width table
  return roi_dispatch(RoiCall{.d_image = d_image, .dtype = dtype, .assay_stride = assay_stride, .n_c = n_c, .n_t = n_t,
                              .h = h, .w = w, .d_beads = d_beads, .d_marker_assay = d_marker_assay,
                              .d_marker_local = d_marker_local, .m = m, .len = roi_len, .d_labels = d_labels, .d_roi = d_roi,
                              .d_fg = d_fg, .d_bg = d_bg, .d_sums = d_sums, .d_counts = d_counts,
                              .stream = mg_stream(stream)});
}

namespace {
// ---- the order the windows of an assay are visited in ---------------------------------------------------------
// The beads of an assay arrive in suppression (score) order, spatially random: two windows that share image lines
// (200-byte rows at arbitrary alignment touch 2.56 lines of 128 B; neighbouring windows overlap) are then worked on
// long after each other and every one fetches its lines from HBM again.  Visited band by band (64 rows) and left to
// right inside a band, neighbours are in flight together and meet in the L2s: 4.73 instead of 5.17 ms at C4 in
// tools/roi_order_probe.py.  d_order[g] = the marker the g-th workgroup takes; only the ORDER of the work changes,
// every marker's outputs stay where they were.  ORDER_PARTS workgroups per assay hold the assay's keys in LDS and rank
// slices of 256 markers each: rank = keys before the marker that are <= its key + keys after it that are < (equal
// keys keep their table order) -- two instructions per key except in the few chunks around the wave's own markers.
// (One workgroup of 1024 per assay took 180 us at C4: 2 000^2 compares on one CU.)  An assay with more beads than
// ORDER_CAP keeps its order.
constexpr int ORDER_CAP = 8192;
constexpr int ORDER_BAND = 6;  // log2 of the band height
constexpr int ORDER_PARTS = 8;

__global__ __launch_bounds__(NT) void k_window_order(const int32_t* __restrict__ d_beads, int64_t bead_stride,
                                                     const int32_t* __restrict__ d_assay_offsets, int m,
                                                     int32_t* __restrict__ d_order) {
  __shared__ __attribute__((aligned(16))) uint32_t keys[ORDER_CAP];
  const int assay = blockIdx.x;
  const int first = d_assay_offsets[assay];
  const int n = min(d_assay_offsets[assay + 1], m) - first;  // (markers beyond the launch's bound m are not worked on)
  if (n <= 0) return;
  if (n > ORDER_CAP) {
    for (int i = blockIdx.y * NT + threadIdx.x; i < n; i += ORDER_PARTS * NT) d_order[first + i] = first + i;
    return;
  }
  const int32_t* b = d_beads + 3 * (bead_stride ? (int64_t)assay * bead_stride : (int64_t)first);
  const int n4 = (n + 3) & ~3, nq = n4 >> 2;
  for (int i = threadIdx.x; i < n4; i += NT) {
    uint32_t k = 0xFFFFFFFFu;  // (padding: after every marker, above every key)
    if (i < n) {
      const int row = min(max(b[3 * i], 0), (1 << 20) - 1), col = min(max(b[3 * i + 1], 0), (1 << 17) - 1);
      k = ((uint32_t)(row >> ORDER_BAND) << 17) | (uint32_t)col;
    }
    keys[i] = k;
  }
  __syncthreads();
  const uint4* k4 = reinterpret_cast<const uint4*>(keys);
  for (int i0 = blockIdx.y * NT; i0 < n; i0 += ORDER_PARTS * NT) {
    const int i = i0 + threadIdx.x;
    const int w0 = __builtin_amdgcn_readfirstlane(i0 + (int)(threadIdx.x & ~63u));  // the wave's first marker
    const int q_lo = min(w0 >> 2, nq), q_hi = min((w0 + 63) >> 2, nq - 1);
    const uint32_t ki = keys[min(i, n - 1)];
    int rank = 0;
    for (int q = 0; q < q_lo; ++q) {  // before every marker of the wave
      const uint4 v = k4[q];
      rank += (v.x <= ki) + (v.y <= ki) + (v.z <= ki) + (v.w <= ki);
    }
    for (int q = q_lo; q <= q_hi; ++q) {  // around them
      const uint4 v = k4[q];
      const int j = 4 * q;
      rank += (v.x < ki || (v.x == ki && j < i)) + (v.y < ki || (v.y == ki && j + 1 < i)) +
              (v.z < ki || (v.z == ki && j + 2 < i)) + (v.w < ki || (v.w == ki && j + 3 < i));
    }
    for (int q = q_hi + 1; q < nq; ++q) {  // after
      const uint4 v = k4[q];
      rank += (v.x < ki) + (v.y < ki) + (v.z < ki) + (v.w < ki);
    }
    if (i < n) d_order[first + rank] = first + i;
  }
}
}  // namespace

extern "C" int mg_roi_window_order(const int32_t* d_beads, int64_t bead_stride, const int32_t* d_assay_offsets,
                                   int n_assays, int m, int32_t* d_order, void* stream) {
  if (!d_beads || !d_assay_offsets || !d_order || n_assays <= 0 || n_assays > 65535 || m < 0 || bead_stride < 0)
    return MG_EINVAL;
  if (m == 0) return MG_OK;
  hipLaunchKernelGGL(k_window_order, dim3(n_assays, ORDER_PARTS), dim3(NT), 0, mg_stream(stream), d_beads, bead_stride,
                     d_assay_offsets, m, d_order);
  MG_CHECK_LAUNCH();
  return MG_OK;
}

extern "C" int mg_roi_segment_reduce(const void* d_image, int dtype, int64_t assay_stride, int n_c, int n_t, int h,
                                     int w, int time_major, const int32_t* d_beads, int64_t bead_stride,
                                     const int32_t* d_assay_offsets, int n_assays, int m, const int32_t* d_order,
                                     int roi_len, const int32_t* d_halfwidths, int max_r, void* d_roi, uint8_t* d_fg,
                                     uint8_t* d_bg, double* d_sums, int32_t* d_counts, void* stream) {
  if (!d_assay_offsets || !d_halfwidths || n_assays <= 0 || n_assays > 65535 || max_r < 0 || bead_stride < 0)
    return MG_EINVAL;
  return roi_dispatch(RoiCall{.d_image = d_image, .dtype = dtype, .assay_stride = assay_stride, .n_c = n_c, .n_t = n_t,
                              .h = h, .w = w, .d_beads = d_beads, .bead_stride = bead_stride, .m = m, .len = roi_len,
                              .d_assay_offsets = d_assay_offsets, .n_assays = n_assays, .time_major = time_major,
                              .d_order = d_order, .d_halfwidths = d_halfwidths, .max_r = max_r, .d_roi = d_roi,
                              .d_fg = d_fg, .d_bg = d_bg, .d_sums = d_sums, .d_counts = d_counts,
                              .stream = mg_stream(stream)});
}

extern "C" int mg_roi_segment_reduce_raw(const void* d_image, const void* d_raw, int dtype, int64_t assay_stride, int n_c,
                                         int n_t, int h, int w, int time_major, int raw_channel_mask, double dark,
                                         double flat, const float* d_flat, const double* d_max2, int planes_per_group,
                                         const int32_t* d_beads, int64_t bead_stride, const int32_t* d_assay_offsets,
                                         int n_assays, int m, const int32_t* d_order, int roi_len,
                                         const int32_t* d_halfwidths, int max_r, void* d_roi, uint8_t* d_fg, uint8_t* d_bg,
                                         double* d_sums, int32_t* d_counts, void* stream) {
  if (!d_assay_offsets || !d_halfwidths || n_assays <= 0 || n_assays > 65535 || max_r < 0 || bead_stride < 0 ||
      raw_channel_mask < 0)
    return MG_EINVAL;
  const RoiRaw rw{(const uint16_t*)d_raw, d_flat, d_max2, flat, dark, planes_per_group, (uint32_t)raw_channel_mask};
  return roi_dispatch(RoiCall{.d_image = d_image, .dtype = dtype, .assay_stride = assay_stride, .n_c = n_c, .n_t = n_t,
                              .h = h, .w = w, .d_beads = d_beads, .bead_stride = bead_stride, .m = m, .len = roi_len,
                              .d_assay_offsets = d_assay_offsets, .n_assays = n_assays, .time_major = time_major,
                              .d_order = d_order, .d_halfwidths = d_halfwidths, .max_r = max_r, .d_roi = d_roi,
                              .d_fg = d_fg, .d_bg = d_bg, .d_sums = d_sums, .d_counts = d_counts,
                              .stream = mg_stream(stream)},
                      &rw);
}
