// Binned planes for find_beads(track="ncc", stage_drift=D) ("find_beads: following a stage that moved"):
// the coarse view on which a handful of large anchor patches are tracked to find the offset every bead of a timepoint
// shares.  out[t, i, j] = the sum of the bin x bin block at (bin i, bin j) of plane t, as float32; hb = h / bin,
// wb = w / bin, the trailing h % bin rows and w % bin columns are not read.
//
// Exactness.  u8 / u16: a block's sum is at most 64 * 65535 < 2^24, summed in uint32 and exact in float32.  f32 / f64:
// summed in float64 -- the block's rows from the top, each from the left -- and rounded to float32 once; the order does
// not depend on the launch, the alignment or the path taken: the same bits on every call.  No atomics.
//
// k_bin: a streaming pass (every pixel read once, 4 / bin^2 bytes written per pixel).  A thread owns a run of OC output
// columns of one output row: CH = OC bin input columns, a whole number of 16-byte vectors, over bin rows -- at least
// four 16-byte loads per item, all independent.  A row of the run is read with 16-byte loads where its first byte is
// 16-byte aligned (the run starts a whole number of vectors into the row, so that is a property of the row), element
// by element otherwise; the last, partial run of a row is read element by element too.  Sums are kept in registers
// and written as float32, consecutive lanes to consecutive addresses (16- or 8-byte stores where the run is aligned).
// Items are dealt to a grid of at most MG_BIN_WALK workgroups in a grid-stride loop.  No LDS.
#include "mg_common.h"

namespace {

template <typename T, int BIN>
struct BinShape {
  static constexpr int N = 16 / (int)sizeof(T);                              // elements per 16-byte vector
  static constexpr int VPR = (BIN > N ? BIN / N : 1) * (BIN == 2 ? 2 : 1);  // vectors per row of a run
  static constexpr int CH = VPR * N, OC = CH / BIN;                         // input / output columns of a run
};

// grid-stride over (plane * hb + output row, run of the row)
template <typename T, int BIN>
__global__ __launch_bounds__(256) void k_bin(const T* __restrict__ planes, int64_t plane_stride, int w, int hb, int wb,
                                             int cpr, int64_t total, float* __restrict__ out) {
  using Sh = BinShape<T, BIN>;
  using Acc = std::conditional_t<std::is_integral<T>::value, uint32_t, double>;
  constexpr int N = Sh::N, VPR = Sh::VPR, CH = Sh::CH, OC = Sh::OC;
  const bool small = total <= 0x7FFFFFFFLL;  // (uniform) 32-bit index arithmetic
  const int64_t stride = (int64_t)gridDim.x * 256;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += stride) {
    int64_t ri, t;
    int c, row;
    if (small) {
      const uint32_t u = (uint32_t)i, r = u / (uint32_t)cpr, tt = r / (uint32_t)hb;
      c = (int)(u - r * (uint32_t)cpr), row = (int)(r - tt * (uint32_t)hb), ri = r, t = tt;
    } else {
      ri = i / cpr, c = (int)(i - ri * cpr), t = ri / hb, row = (int)(ri - t * hb);
    }
    const int j0 = c * OC, nj = min(OC, wb - j0);
    const T* p = planes + t * plane_stride + (int64_t)row * BIN * w + (int64_t)j0 * BIN;
    Acc acc[OC];
#pragma unroll
    for (int j = 0; j < OC; ++j) acc[j] = (Acc)0;
    if (nj == OC) {
#pragma unroll
      for (int r = 0; r < BIN; ++r) {
        const T* q = p + (int64_t)r * w;
        T x[CH];
        if ((reinterpret_cast<uintptr_t>(q) & 15) == 0) {
#pragma unroll
          for (int v = 0; v < VPR; ++v) {
            const uint4 bits = *reinterpret_cast<const uint4*>(q + v * N);
            __builtin_memcpy(&x[v * N], &bits, 16);
          }
        } else {
#pragma unroll
          for (int k = 0; k < CH; ++k) x[k] = q[k];
        }
#pragma unroll
        for (int k = 0; k < CH; ++k) acc[k / BIN] += (Acc)x[k];
      }
    } else {
      for (int r = 0; r < BIN; ++r) {
        const T* q = p + (int64_t)r * w;
#pragma unroll
        for (int j = 0; j < OC; ++j)
          if (j < nj) {
#pragma unroll
            for (int k = 0; k < BIN; ++k) acc[j] += (Acc)q[j * BIN + k];
          }
      }
    }
    float* o = out + ri * wb + j0;
    float f[OC];
#pragma unroll
    for (int j = 0; j < OC; ++j) f[j] = (float)acc[j];
    if (OC % 4 == 0 && nj == OC && (reinterpret_cast<uintptr_t>(o) & 15) == 0) {
#pragma unroll
      for (int j = 0; j + 4 <= OC; j += 4) *reinterpret_cast<float4*>(o + j) = make_float4(f[j], f[j + 1], f[j + 2], f[j + 3]);
    } else if (OC % 2 == 0 && nj == OC && (reinterpret_cast<uintptr_t>(o) & 7) == 0) {
#pragma unroll
      for (int j = 0; j + 2 <= OC; j += 2) *reinterpret_cast<float2*>(o + j) = make_float2(f[j], f[j + 1]);
    } else {
#pragma unroll
      for (int j = 0; j < OC; ++j)
        if (j < nj) o[j] = f[j];
    }
  }
}

template <typename T, int BIN>
int launch_bin(const void* d_planes, int n_t, int64_t plane_stride, int h, int w, float* d_out, hipStream_t s) {
  const int hb = h / BIN, wb = w / BIN, oc = BinShape<T, BIN>::OC;
  const int cpr = (wb + oc - 1) / oc;
  const int64_t total = (int64_t)n_t * hb * cpr;
  const int blocks = (int)std::min<int64_t>((total + 255) / 256, MG_BIN_WALK);
  hipLaunchKernelGGL((k_bin<T, BIN>), dim3(blocks), dim3(256), 0, s, (const T*)d_planes, plane_stride, w, hb, wb, cpr, total,
                     d_out);
  MG_CHECK_LAUNCH();
  return MG_OK;
}

}  // namespace

extern "C" int mg_bin_planes(const void* d_planes, int dtype, int n_t, int64_t plane_stride, int h, int w, int bin,
                             float* d_out, void* stream) {
  if (!(bin == 2 || bin == 4 || bin == 8) || h < bin || w < bin || n_t < 1 || plane_stride < 0 || !d_planes || !d_out)
    return MG_EINVAL;
  hipStream_t s = mg_stream(stream);
  return mg_dispatch_pixel(dtype, [&](auto t) {
    using T = decltype(t);
    if (bin == 2) return launch_bin<T, 2>(d_planes, n_t, plane_stride, h, w, d_out, s);
    if (bin == 4) return launch_bin<T, 4>(d_planes, n_t, plane_stride, h, w, d_out, s);
    return launch_bin<T, 8>(d_planes, n_t, plane_stride, h, w, d_out, s);
  });
}
