// What the kernels over already gathered ROI windows share (mg_roistats.hip, mg_unmix.hip, mg_profile.hip,
// mg_segment.hip, mg_refine.hip; DESIGN.md, "Window kernels: what they share"): the workgroup of MG_WINDOW_THREADS
// threads a window, the host check and the launch frame of their entries, the copy of a table of fractions, and the
// walk of the kernels that stream a whole window -- chunks of 16 bytes of pixels, dealt to the waves in runs, the
// loads of IN_FLIGHT steps issued before the first is worked on.  The order statistics are mg_select.h's.
#pragma once
#include <initializer_list>

#include "mg_select.h"

// (an unnamed namespace: every file that includes this gets copies of its own, as if it had written them)
namespace {

constexpr int MG_WINDOW_THREADS = MG_SELECT_THREADS, MG_WINDOW_WAVES = MG_WINDOW_THREADS / 64;
static_assert(MG_WINDOW_WAVES == MG_FOLD_WAVES, "mg_block_fold folds four waves, and the kernels add out four partials");

// ---- the entry frame --------------------------------------------------------------------------------------------------

// What every entry refuses: fewer than no markers, no channel, no timepoint, a window side outside 1 .. max_len, more
// than 2^31 - 1 windows (one workgroup a window, or a channel's share of one), a negative stride.  An entry without a
// channel axis passes n_c = 1.  Pointers, a mask that has to be there and the entry's own arguments are its own rules.
inline bool mg_windows_check(int m, int n_c, int n_t, int roi_len, int max_len, std::initializer_list<int64_t> strides) {
  if (m < 0 || n_c <= 0 || n_t <= 0 || roi_len <= 0 || roi_len > max_len) return false;
  if ((int64_t)m * n_c * n_t > INT32_MAX) return false;
  for (const int64_t s : strides)
    if (s < 0) return false;
  return true;
}

// n_q fractions (0 .. max_q of them, each in [0, 1]) checked and copied to dst; false for what is refused.
inline bool mg_fractions(const double* q, int n_q, int max_q, double* dst) {
  if (n_q < 0 || n_q > max_q || (n_q > 0 && !q)) return false;
  for (int j = 0; j < n_q; ++j) {
    if (!(q[j] >= 0.0 && q[j] <= 1.0)) return false;  // (NaN fails both)
    dst[j] = q[j];
  }
  return true;
}

// launch(T{}, grid, block) with T the element type of `dtype` and m * per_marker workgroups of MG_WINDOW_THREADS:
// MG_EINVAL for any other dtype code, with or without markers; no markers is MG_OK for a valid one, nothing launched.
template <class Launch>
inline int mg_windows_launch(int dtype, int m, int per_marker, Launch&& launch) {
  return mg_dispatch_pixel(dtype, [&](auto t) {
    if (m == 0) return (int)MG_OK;
    launch(t, dim3((unsigned)((int64_t)m * per_marker)), dim3(MG_WINDOW_THREADS));
    MG_CHECK_LAUNCH();
    return (int)MG_OK;
  });
}

// ---- the chunk walk ---------------------------------------------------------------------------------------------------

// A chunk as it comes from memory: VW pixels (16 bytes of them, or one) and their mask bytes, byte j in mw[j / 4].
// Pixels beyond the window have mask byte 0.  MASKED = false: there is no mask to read, every pixel of the window has
// byte 1.
template <typename T, int VW>
struct RawChunk {
  T px[VW];
  uint32_t mw[4];
  __device__ __forceinline__ bool under_mask(int j) const { return ((mw[j >> 2] >> (8 * (j & 3))) & 0xFFu) != 0u; }
};
// VW (2, 4, 8 or 16) bytes from p, which is aligned to VW, as one load: byte j in w[j / 4].
template <int VW>
__device__ __forceinline__ void load_bytes(const uint8_t* p, uint32_t* w) {
  if constexpr (VW == 16) {
    const uint4 t = *reinterpret_cast<const uint4*>(p);
    w[0] = t.x, w[1] = t.y, w[2] = t.z, w[3] = t.w;
  } else if constexpr (VW == 8) {
    const uint2 t = *reinterpret_cast<const uint2*>(p);
    w[0] = t.x, w[1] = t.y;
  } else if constexpr (VW == 4) {
    w[0] = *reinterpret_cast<const uint32_t*>(p);
  } else {
    w[0] = *reinterpret_cast<const uint16_t*>(p);
  }
}
template <typename T, int VW, bool MASKED = true>
__device__ __forceinline__ RawChunk<T, VW> fetch(const T* __restrict__ v, const uint8_t* __restrict__ mask, int n, int c,
                                                 int end) {
  RawChunk<T, VW> r = {};
  if (c >= end) return r;
  if (VW > 1 && (c + 1) * VW <= n) {
    const uint4 bits = *reinterpret_cast<const uint4*>(v + (int64_t)c * VW);
    __builtin_memcpy(r.px, &bits, 16);
    const uint8_t* mp = mask + (int64_t)c * VW;
    if constexpr (!MASKED) {
#pragma unroll
      for (int j = 0; j < VW; j += 4) r.mw[j >> 2] = VW >= 4 ? 0x01010101u : 0x0101u;
    } else {
      load_bytes<VW>(mp, r.mw);
    }
  } else {  // VW = 1, or the window's last, partial chunk
#pragma unroll
    for (int j = 0; j < VW; ++j) {
      const int p = c * VW + j;
      if (p < n) r.px[j] = v[p], r.mw[j >> 2] |= (uint32_t)(MASKED ? mask[p] : (uint8_t)1) << (8 * (j & 3));
    }
  }
  return r;
}

// The run of chunks that wave `wave` walks of a window of n pixels cut into chunks of vw: the chunks dealt to the
// MG_WINDOW_WAVES waves in equal runs [begin, end), the last ones shorter or empty.
struct WaveRun {
  int chunks, per_wave, begin, end;
};
__device__ __forceinline__ WaveRun wave_run(int n, int vw, int wave) {
  const int chunks = (n + vw - 1) / vw, per_wave = (chunks + MG_WINDOW_WAVES - 1) / MG_WINDOW_WAVES;
  const int begin = min(wave * per_wave, chunks);
  return {chunks, per_wave, begin, min(begin + per_wave, chunks)};
}

// The pass over a window: every wave walks its run, its lanes 64 chunks at a time, the loads of IN_FLIGHT such steps
// issued before the first is worked on.  body(raw, c, run) gets, for every step that has a chunk below run.end, the
// lane's chunk as it came from memory and its index c -- which may lie at or beyond run.end: those are another wave's
// pixels or none, `raw` is all zero, and the lane still takes part in whatever the body does across the wave.  The
// trip counts are wave-uniform.  MASKED = false: `mask` is not read.
constexpr int IN_FLIGHT = 4;
template <typename T, int VW, bool MASKED = true, class Body>
__device__ __forceinline__ void walk_chunks(const T* __restrict__ v, const uint8_t* __restrict__ mask, int n, Body&& body) {
  const int lane = threadIdx.x & 63;
  const WaveRun run = wave_run(n, VW, threadIdx.x >> 6);
  for (int c0 = run.begin; c0 < run.end; c0 += 64 * IN_FLIGHT) {
    RawChunk<T, VW> raw[IN_FLIGHT];
#pragma unroll
    for (int u = 0; u < IN_FLIGHT; ++u) raw[u] = fetch<T, VW, MASKED>(v, mask, n, c0 + 64 * u + lane, run.end);
#pragma unroll
    for (int u = 0; u < IN_FLIGHT; ++u) {
      if (c0 + 64 * u >= run.end) break;
      body(raw[u], c0 + 64 * u + lane, run);
    }
  }
}

// The chunk width of a window: 16 bytes of pixels where the window starts on 16 bytes and its mask on as many bytes as
// a chunk has pixels (no mask: a null pointer, which is aligned) -- one 16-byte load per lane and chunk; 1 otherwise.
// with_chunk_width hands f the width as a std::integral_constant and returns what f returns.
template <typename T>
constexpr int wide_chunk = 16 / (int)sizeof(T);
template <typename T>
__device__ __forceinline__ bool window_is_wide(const T* v, const uint8_t* mask) {
  return (reinterpret_cast<uintptr_t>(v) & 15) == 0 && (reinterpret_cast<uintptr_t>(mask) & (wide_chunk<T> - 1)) == 0;
}
template <typename T, class F>
__device__ __forceinline__ auto with_chunk_width(bool wide, F&& f) {
  if (wide) return f(std::integral_constant<int, wide_chunk<T>>{});
  return f(std::integral_constant<int, 1>{});
}

}  // namespace
