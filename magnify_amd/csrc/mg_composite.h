// The composite contract of plot.overview and plot.roishow (sections 18 and 19), once: k_overview
// (mg_overview.hip) and k_roi_montage (mg_montage.hip) gather their block sums and find their overlay each in their own
// way and call these for everything between a block's sum and its three bytes.  All float64, one operation at a time
// (-ffp-contract=off): tests/plot_ref.py and tests/roishow_ref.py restate the sequence and hold both kernels to it bit
// for bit.
#pragma once
#include "mg_common.h"

// (an unnamed namespace: every file that includes this gets copies of its own, as if it had written them)
namespace {

constexpr int MG_OVERLAY_NONE = 0, MG_OVERLAY_OUTLINE = 1, MG_OVERLAY_FILL = 2;
inline bool mg_overlay_ok(int overlay, double alpha) {
  return (overlay == MG_OVERLAY_NONE || overlay == MG_OVERLAY_OUTLINE || overlay == MG_OVERLAY_FILL) &&
         alpha >= 0.0 && alpha <= 1.0;  // (NaN fails both)
}

struct MgChannels {  // by value: what every thread needs of every channel
  double lo[MG_OVERVIEW_MAX_CHANNELS], hi[MG_OVERVIEW_MAX_CHANNELS], rgb[MG_OVERVIEW_MAX_CHANNELS][3];
};

// limits (n_c, 2) and colors (n_c, 3) on the host into the record, the unused slots zero; MG_EINVAL for a colour outside
// [0, 1] (NaN included).  1 <= n_c <= MG_OVERVIEW_MAX_CHANNELS is the caller's check.
inline int mg_fill_channels(const double* limits, const double* colors, int n_c, MgChannels* ch) {
  for (int k = 0; k < MG_OVERVIEW_MAX_CHANNELS; ++k) {
    const bool used = k < n_c;
    ch->lo[k] = used ? limits[2 * k] : 0.0, ch->hi[k] = used ? limits[2 * k + 1] : 0.0;
    for (int e = 0; e < 3; ++e) {
      ch->rgb[k][e] = used ? colors[3 * k + e] : 0.0;
      if (!(ch->rgb[k][e] >= 0.0 && ch->rgb[k][e] <= 1.0)) return MG_EINVAL;
    }
  }
  return MG_OK;
}

// Block sums: uint32 for u8 / u16 (64^2 * 65535 < 2^32, exact), float64 for float pixels.
template <typename T>
using mg_block_acc_t = std::conditional_t<std::is_integral<T>::value, uint32_t, double>;

// What the composite step needs of channel k, read once for all the blocks a thread owns.
struct MgChannel {
  double lo, range, r, g, b;
  bool flat;
};
__device__ __forceinline__ MgChannel mg_channel(const MgChannels& ch, int k) {
  return {ch.lo[k], ch.hi[k] - ch.lo[k], ch.rgb[k][0], ch.rgb[k][1], ch.rgb[k][2], !(ch.hi[k] > ch.lo[k])};
}

// The composite step.  A block of n pixels of channel c that sum to `sum`, added to the pixel: mean,
// (mean - lo) / (hi - lo), clamp, acc = min(acc + u * colour, 1).
template <typename Acc>
__device__ __forceinline__ void mg_composite_add(const MgChannel& c, Acc sum, int n, double (&acc)[3]) {
  double mean = (double)sum;
  if (n != 1) mean = mean / (double)n;  // (x / 1 is x)
  double u = (mean - c.lo) / c.range;
  if (c.flat || !(u >= 0.0)) u = 0.0;  // hi <= lo, NaN, u < 0
  if (u > 1.0) u = 1.0;
  acc[0] = fmin(acc[0] + u * c.r, 1.0);
  acc[1] = fmin(acc[1] + u * c.g, 1.0);
  acc[2] = fmin(acc[2] + u * c.b, 1.0);
}

// The overlay on a pixel: colour rgb (0 .. 255 per component) with weight a.
__device__ __forceinline__ void mg_overlay_blend(double a, double r, double g, double b, double (&acc)[3]) {
  const double keep = 1.0 - a, rgb[3] = {r, g, b};
#pragma unroll
  for (int e = 0; e < 3; ++e) acc[e] = keep * acc[e] + (a * rgb[e]) / 255.0;
}

__device__ __forceinline__ uint8_t mg_composite_byte(double x) { return (uint8_t)floor(255.0 * x + 0.5); }

}  // namespace
