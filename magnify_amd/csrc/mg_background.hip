// Background (the `subtract_background` component): the grey opening of every plane of a contiguous block (N, H, W) with
// a (2R + 1)^2 window -- the minimum over the window, then the maximum over the window of that -- and the plane minus
// it (mg_background_planes).  Minimum and maximum over a square are separable, so the opening is four 1-D passes
// (min-x, min-y, max-y, max-x) in three launches: the two vertical ones are one kernel.  Every 1-D pass is van Herk /
// Gil-Werman: the line is cut into blocks of 2R + 1, G is the running extremum from a block's start, H the one from
// its end, and the extremum of the window i - R .. i + R is op(H[i - R], G[i + R]) -- three compares per pixel at
// any R.  Oracle: tests/background_ref.py.
#include <algorithm>
#include <limits>

#include "mg_planes.h"

namespace {

constexpr int BG_THREADS = 256;
constexpr int BG_LDS_BUDGET = 80 * 1024;  // two workgroups on a CU
constexpr int BG_LDS_WISH = 40 * 1024;    // four, where that leaves BG_WISH_LINES lines or more
constexpr int BG_MIN_LINES = 8, BG_WISH_LINES = 32;
constexpr int BG_BATCH = 16;              // global loads a thread has in flight when a tile is filled
constexpr int BG_SCAN = 8;                // values a thread reads from LDS at a time as it walks a block

// What a position that takes no part holds: NaN for floats (fmin / fmax return the other operand, and NaN when both
// are -- "a window with nothing left is NaN"), the far end of the range for integers (every window of a pixel in the
// plane holds that pixel, so the value never comes out).
template <class T>
__device__ __forceinline__ T bg_ident(bool is_max) {
  if constexpr (std::is_integral<T>::value) return is_max ? (T)0 : std::numeric_limits<T>::max();
  else return std::numeric_limits<T>::quiet_NaN();
}
template <class T, bool MAX>
__device__ __forceinline__ T bg_op(T a, T b) {
  if constexpr (std::is_same<T, float>::value) return MAX ? fmaxf(a, b) : fminf(a, b);
  else if constexpr (std::is_same<T, double>::value) return MAX ? fmax(a, b) : fmin(a, b);
  else return MAX ? (a > b ? a : b) : (a < b ? a : b);
}

// The elements of a tile, dealt to the threads so that the lanes of a wave run along the direction that is contiguous
// in memory: f(pos, line) for pos < n_pos, line < nl.  VERT: lines are columns (nl of them side by side, a power of two),
// else rows (64 lanes along a row).
template <bool VERT, class F>
__device__ __forceinline__ void bg_each(int n_pos, int nl, int nl_log2, F&& f) {
  const int t = threadIdx.x;
  if (VERT) {
    for (int pos = t >> nl_log2; pos < n_pos; pos += BG_THREADS >> nl_log2) f(pos, t & (nl - 1));
  } else {
    for (int line = t >> 6; line < nl; line += BG_THREADS / 64)
      for (int pos = t & 63; pos < n_pos; pos += 64) f(pos, line);
  }
}

// The same walk for an element that starts with a read of global memory: `load` of BG_BATCH elements is issued before
// `use` takes the first (one load at a time leaves a workgroup waiting on memory latency between any two).
template <bool VERT, class T, class L, class U>
__device__ __forceinline__ void bg_each_loaded(int n_pos, int nl, int nl_log2, L&& load, U&& use) {
  const int t = threadIdx.x;
  if (VERT) {
    const int line = t & (nl - 1), step = BG_THREADS >> nl_log2;
    for (int first = t >> nl_log2; first < n_pos; first += BG_BATCH * step) {
      T v[BG_BATCH];
#pragma unroll
      for (int j = 0; j < BG_BATCH; ++j) v[j] = load(min(first + j * step, n_pos - 1), line);
#pragma unroll
      for (int j = 0; j < BG_BATCH; ++j)
        if (first + j * step < n_pos) use(first + j * step, line, v[j]);
    }
  } else {
    constexpr int ACROSS = BG_BATCH / 2;  // two lines at a time, ACROSS positions of each
    for (int line = t >> 6; line < nl; line += 2 * (BG_THREADS / 64))
      for (int first = t & 63; first < n_pos; first += ACROSS * 64) {
        T v[2][ACROSS];
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
          for (int j = 0; j < ACROSS; ++j)
            v[i][j] = load(min(first + j * 64, n_pos - 1), min(line + i * (BG_THREADS / 64), nl - 1));
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
          for (int j = 0; j < ACROSS; ++j)
            if (first + j * 64 < n_pos && line + i * (BG_THREADS / 64) < nl) use(first + j * 64, line + i * (BG_THREADS / 64), v[i][j]);
      }
  }
}

// G and H of every block of every line: a thread owns one line of one block at a time (lanes along the lines: the
// walk is free of bank conflicts whatever the pitch).  G goes to its own array, H takes the place of the values.  The
// values are read BG_SCAN at a time (the rest of a block one by one): the running extremum is the only chain, the reads
// of LDS do not wait for it.
template <class T, bool MAX>
__device__ __forceinline__ void bg_scan(T* __restrict__ a, T* __restrict__ g, int len, int win, int pitch, int nl, int nl_log2) {
  const int line = threadIdx.x & (nl - 1), n_blocks = (len + win - 1) / win;
  for (int b = threadIdx.x >> nl_log2; b < n_blocks; b += BG_THREADS >> nl_log2) {
    const int j0 = b * win, j1 = min(j0 + win, len);
    T run = a[j0 * pitch + line];  // (op(x, x) = x: the first value may be taken in twice)
    int j = j0;
    for (; j + BG_SCAN <= j1; j += BG_SCAN) {
      T v[BG_SCAN];
#pragma unroll
      for (int u = 0; u < BG_SCAN; ++u) v[u] = a[(j + u) * pitch + line];
#pragma unroll
      for (int u = 0; u < BG_SCAN; ++u) {
        run = bg_op<T, MAX>(run, v[u]);
        g[(j + u) * pitch + line] = run;
      }
    }
    for (; j < j1; ++j) {
      run = bg_op<T, MAX>(run, a[j * pitch + line]);
      g[j * pitch + line] = run;
    }
    run = a[(j1 - 1) * pitch + line];
    for (j = j1 - 1; j - BG_SCAN >= j0 - 1; j -= BG_SCAN) {
      T v[BG_SCAN];
#pragma unroll
      for (int u = 0; u < BG_SCAN; ++u) v[u] = a[(j - u) * pitch + line];
#pragma unroll
      for (int u = 0; u < BG_SCAN; ++u) {
        run = bg_op<T, MAX>(run, v[u]);
        a[(j - u) * pitch + line] = run;
      }
    }
    for (; j >= j0; --j) {
      run = bg_op<T, MAX>(run, a[j * pitch + line]);
      a[j * pitch + line] = run;
    }
  }
}

// One launch: STAGES 1-D passes along one direction (VERT: along y) over every plane; stage 0 is a maximum if
// FIRST_MAX, else a minimum, stage 1 the other one.  A workgroup takes `nl` neighbouring lines and a run of `run`
// output positions at a time, with STAGES * R more positions on either side: L = run + 2 STAGES R positions x nl
// lines in LDS, twice (values / H, and G).  Positions outside the plane hold the stage's bg_ident.  After a stage,
// output k (the window centred on input k + R) lies where input k lay.  SUBTRACT: the last stage's result B does
// not go out itself but orig - B where orig > B, else 0, NaN where either is.  Work items (plane, group of lines, run)
// are dealt to a 1-D grid: no count is bounded by a grid dimension.
template <class T, bool VERT, int STAGES, bool FIRST_MAX, bool SUBTRACT>
__global__ __launch_bounds__(BG_THREADS) void k_bg_pass(const T* __restrict__ src, const T* __restrict__ orig, T* __restrict__ dst,
                                                        int h, int w, int radius, int nl, int nl_log2, int run, int pitch,
                                                        int64_t n_groups, int64_t n_runs, int64_t total) {
  extern __shared__ __attribute__((aligned(16))) unsigned char bg_lds[];
  const int win = 2 * radius + 1, len0 = run + 2 * STAGES * radius;
  T* a = reinterpret_cast<T*>(bg_lds);
  T* g = a + (size_t)len0 * pitch;
  const int extent = VERT ? h : w, n_lines = VERT ? w : h;
  const int64_t plane = (int64_t)h * w;
  for (int64_t item = blockIdx.x; item < total; item += gridDim.x) {
    const int64_t pi = item / (n_groups * n_runs), rest = item - pi * (n_groups * n_runs);
    const int64_t gi = rest / n_runs;
    const int64_t pos0 = (rest - gi * n_runs) * run, line0 = gi * nl;  // (below 2^30: a row or a column of the plane)
    const int64_t base = pi * plane;
    auto offset = [&](int64_t gp, int64_t gl) { return base + (VERT ? gp * w + gl : gl * w + gp); };
    bg_each_loaded<VERT, T>(
        len0, nl, nl_log2,
        [&](int pos, int line) {
          const int64_t gp = pos0 - STAGES * radius + pos, gl = line0 + line;
          return gp >= 0 && gp < extent && gl < n_lines ? src[offset(gp, gl)] : bg_ident<T>(FIRST_MAX);
        },
        [&](int pos, int line, T v) { a[pos * pitch + line] = v; });
    __syncthreads();
#pragma unroll
    for (int stage = 0; stage < STAGES; ++stage) {
      const bool is_max = FIRST_MAX != (stage == 1);  // (a constant once the loop is unrolled)
      const int len = len0 - 2 * radius * stage;
      if (is_max) bg_scan<T, true>(a, g, len, win, pitch, nl, nl_log2);
      else bg_scan<T, false>(a, g, len, win, pitch, nl, nl_log2);
      __syncthreads();
      const int64_t first = pos0 - (STAGES - 1 - stage) * radius;  // the plane position of output 0
      auto combine = [&](int k, int line) {
        const T hv = a[k * pitch + line], gv = g[(k + 2 * radius) * pitch + line];
        return is_max ? bg_op<T, true>(hv, gv) : bg_op<T, false>(hv, gv);
      };
      auto inside = [&](int k, int line) { return first + k >= 0 && first + k < extent && line0 + line < n_lines; };
      if (stage + 1 < STAGES) {
        bg_each<VERT>(len - 2 * radius, nl, nl_log2, [&](int k, int line) {
          a[k * pitch + line] = first + k >= 0 && first + k < extent ? combine(k, line) : bg_ident<T>(!is_max);
        });
      } else if constexpr (SUBTRACT) {
        bg_each_loaded<VERT, T>(
            len - 2 * radius, nl, nl_log2,
            [&](int k, int line) { return inside(k, line) ? orig[offset(first + k, line0 + line)] : (T)0; },
            [&](int k, int line, T p) {
              if (!inside(k, line)) return;
              const T v = combine(k, line);
              T d;
              if constexpr (std::is_integral<T>::value) d = p > v ? (T)(p - v) : (T)0;
              else d = (p != p || v != v) ? std::numeric_limits<T>::quiet_NaN() : p > v ? p - v : (T)0;
              dst[offset(first + k, line0 + line)] = d;
            });
      } else {
        bg_each<VERT>(len - 2 * radius, nl, nl_log2, [&](int k, int line) {
          if (inside(k, line)) dst[offset(first + k, line0 + line)] = combine(k, line);
        });
      }
      __syncthreads();  // (also: nobody fills the next tile while another thread reads this one)
    }
  }
}

// The lines of a workgroup, a power of two: max_lines, or half of them down to BG_WISH_LINES, if that fits BG_LDS_WISH;
// else as many as BG_LDS_BUDGET allows, down to BG_MIN_LINES.  The pitch of a line group, in elements: the group
// itself where the lanes of the fill run along it (VERT); else 4 * odd bytes, so that the fill, whose lanes run along
// the positions, spreads over the banks.
struct BgShape {
  int nl, nl_log2, pitch;
  size_t lds;
};
static BgShape bg_shape(bool vert, int esize, int len0, int max_lines) {
  BgShape s{};
  auto with = [&](int nl) {
    s.nl = nl;
    s.pitch = vert ? nl : nl + std::max(1, 4 / esize);
    s.lds = (size_t)2 * len0 * s.pitch * esize;
    return s.lds;
  };
  int nl = max_lines;
  while (nl > BG_WISH_LINES && with(nl) > (size_t)BG_LDS_WISH) nl /= 2;
  if (with(nl) > (size_t)BG_LDS_WISH)
    for (nl = max_lines; nl > BG_MIN_LINES && with(nl) > (size_t)BG_LDS_BUDGET;) nl /= 2;
  with(nl);
  for (s.nl_log2 = 0; (1 << s.nl_log2) < s.nl; ++s.nl_log2) {}
  return s;
}
static_assert(2 * (MG_BACKGROUND_ROWS + 4 * MG_BACKGROUND_MAX_RADIUS) * BG_MIN_LINES * 8 <= BG_LDS_BUDGET,
              "the vertical pair of passes, float64 at the largest radius, on the narrowest group of columns");
static_assert(2 * (MG_BACKGROUND_SPAN + 2 * MG_BACKGROUND_MAX_RADIUS) * (BG_MIN_LINES + 1) * 8 <= BG_LDS_BUDGET,
              "a horizontal pass, float64 at the largest radius, on the fewest rows");
static_assert(MG_BACKGROUND_COLS == 64 && BG_THREADS % MG_BACKGROUND_COLS == 0, "a wave along x in the vertical passes");

template <class T, bool VERT, int STAGES, bool FIRST_MAX, bool SUBTRACT>
int launch_bg_pass(const T* src, const T* orig, T* dst, int64_t n, int h, int w, int radius, hipStream_t s) {
  const int run = VERT ? MG_BACKGROUND_ROWS : MG_BACKGROUND_SPAN;
  const BgShape shape = bg_shape(VERT, (int)sizeof(T), run + 2 * STAGES * radius, MG_BACKGROUND_COLS);
  const int extent = VERT ? h : w, n_lines = VERT ? w : h;
  const int64_t n_runs = ((int64_t)extent + run - 1) / run, n_groups = ((int64_t)n_lines + shape.nl - 1) / shape.nl;
  const int64_t total = n * n_groups * n_runs;  // (n h w fits 63 bits with room to spare: the entry checked)
  static bool attr_set = false;
  if (!attr_set) {
    if (hipFuncSetAttribute(reinterpret_cast<const void*>(k_bg_pass<T, VERT, STAGES, FIRST_MAX, SUBTRACT>),
                            hipFuncAttributeMaxDynamicSharedMemorySize, BG_LDS_BUDGET) != hipSuccess)
      return MG_ELAUNCH;
    attr_set = true;
  }
  const unsigned blocks = (unsigned)std::min<int64_t>(total, MG_BACKGROUND_WALK);
  hipLaunchKernelGGL((k_bg_pass<T, VERT, STAGES, FIRST_MAX, SUBTRACT>), dim3(blocks), dim3(BG_THREADS), shape.lds, s, src, orig,
                     dst, h, w, radius, shape.nl, shape.nl_log2, run, shape.pitch, n_groups, n_runs, total);
  MG_CHECK_LAUNCH();
  return MG_OK;
}

// Bytes of two blocks (n, h, w), or -1 where the sizes or one of `pixels` (mg_planes_check) are refused.
static int64_t bg_scratch_bytes(int dtype, int64_t n, int h, int w, int radius, std::initializer_list<const void*> pixels) {
  if (mg_planes_check(dtype, n, h, w, pixels) == MG_PLANES_REFUSED) return -1;
  if (radius < 1 || radius > MG_BACKGROUND_MAX_RADIUS) return -1;
  const int64_t per_plane = 2 * (int64_t)h * w * mg_elem_size(dtype);  // at most 2^54
  if (per_plane && n > (INT64_MAX / 2) / per_plane) return -1;
  return n * per_plane;
}

}  // namespace

extern "C" int64_t mg_background_scratch_bytes(int dtype, int64_t n, int h, int w, int radius) {
  return bg_scratch_bytes(dtype, n, h, w, radius, {});
}

extern "C" int mg_background_planes(const void* d_src, const void* d_filtered, void* d_dst, int dtype, int64_t n, int h, int w,
                                    int radius, int mode, void* d_scratch, int64_t scratch_bytes, void* stream) {
  const int64_t need = bg_scratch_bytes(dtype, n, h, w, radius, {d_src, d_filtered, d_dst, d_scratch});
  if (need < 0 || (mode != MG_BACKGROUND_ESTIMATE && mode != MG_BACKGROUND_SUBTRACT)) return MG_EINVAL;
  if (!d_src || !d_dst || d_dst == d_src || d_dst == d_filtered || scratch_bytes < need) return MG_EINVAL;
  if (need && (!d_scratch || d_scratch == d_src || d_scratch == d_dst || d_scratch == d_filtered)) return MG_EINVAL;
  if (need == 0) return MG_OK;  // (n, h or w is 0)
  hipStream_t s = mg_stream(stream);
  return mg_dispatch_pixel(dtype, [&](auto t) {
    using T = decltype(t);
    const T* p = static_cast<const T*>(d_src);
    const T* f = d_filtered ? static_cast<const T*>(d_filtered) : p;
    T* one = static_cast<T*>(d_scratch);
    T* two = one + n * (int64_t)h * w;
    T* out = static_cast<T*>(d_dst);
    int rc = launch_bg_pass<T, false, 1, false, false>(f, nullptr, one, n, h, w, radius, s);                      // min-x
    if (rc == MG_OK) rc = launch_bg_pass<T, true, 2, false, false>(one, nullptr, two, n, h, w, radius, s);        // min-y, max-y
    if (rc != MG_OK) return rc;
    return mode == MG_BACKGROUND_SUBTRACT ? launch_bg_pass<T, false, 1, true, true>(two, p, out, n, h, w, radius, s)  // max-x
                                          : launch_bg_pass<T, false, 1, true, false>(two, nullptr, out, n, h, w, radius, s);
  });
}
