// plot.percentile_limits ("roishow and percentile contrast limits"): exact order statistics of a resident
// stack by radix selection on an order-preserving integer key, coarse to fine.  The key of a value: the value itself
// for u8 (8 bits) and u16 (16 bits); for float32 -- and float64 rounded to float32 first, which is monotone -- the 32
// key of median_key<float> (mg_select.h: the sign flipped for positive, all bits flipped for negative values), -0
// counted as +0.  NaN has no key and is not counted.
//
// k_key_hist is one read-once pass: every value whose key bits above `prefix_shift` equal one of up to
// MG_PERCENTILE_MAX_PREFIXES selected prefixes (the first pass has none: every value takes part) is counted in the
// table of that prefix, in bin (key >> shift) & (2^bits - 1).  The host reads the small tables, picks the bin that
// holds each rank, and asks for the next pass inside it (hotpath.percentiles) -- the split of mg_edge_thresholds*.
// Passes: u8 one (8 bits), u16 two (11 + 5), float three (11 + 11 + 10).
//
// Tables live in LDS, one uint32 per bin and workgroup (at most 4 x 2048 x 4 B = 32 KiB), and are added to the uint64
// tables in global memory once per workgroup, non-empty bins only.  A real image puts most pixels into a few bins: a
// wave's 64 keys of one round would then hit one LDS address and be served one after the other.  So equal keys are
// gathered before the atomic, twice.  In the lane: a run of equal bins among the 2 .. 16 neighbouring pixels of its
// vector is one count (on a narrow histogram a lane mostly has one run).  In the wave, for the last run of every
// lane: the first active lane's (bin, count) is broadcast, the lanes that hold the same pair are counted with a
// ballot and that lane adds count * lanes once; two such rounds, and what is left (on a narrow histogram: next to
// nothing; on white noise: nearly all, on distinct addresses) goes through a plain LDS atomic.
//
// Work: a unit is `unit_len` contiguous elements (a plane, a window) at d + i0 * stride0 + i1 * stride1; a chunk is
// up to 256 * R vectors of 16 bytes of one unit, a workgroup strides over the chunks.  16-byte loads where the vector
// lies whole in the unit and its address is aligned, element loads otherwise.
#include "mg_select.h"

namespace {

constexpr int PC_MAX_BITS = MG_PERCENTILE_MAX_BITS;
constexpr uint32_t PC_NONE = 0xFFFFFFFFu;

struct PcPrefixes {
  uint32_t v[MG_PERCENTILE_MAX_PREFIXES];
};

template <typename T>
__device__ __forceinline__ bool pc_key(T x, uint32_t& key) {
  if constexpr (std::is_integral<T>::value) {
    key = (uint32_t)x;
    return true;
  } else {
    float f = (float)x;  // (float64: round to nearest even, the order statistic commutes with it)
    if (f != f) return false;
    if (f == 0.0f) f = 0.0f;  // -0 is +0
    return median_key<float>::key(f, &key);  // (true: f is no NaN)
  }
}

// `run` counts at s_hist[addr] for every lane with ok.  Lanes of the wave that hold the same (addr, run) are gathered
// first: the first active lane's pair is broadcast, the lanes with that pair are counted by a ballot and that lane adds
// count * run once; two such rounds, then a plain atomic for what is left.
__device__ __forceinline__ void pc_count_wave(uint32_t* s_hist, uint32_t addr, uint32_t run, bool ok, int lane) {
  const uint32_t code = addr | (run << 16);  // (addr < 2^13, run <= 16)
  unsigned long long act = __ballot(ok);
#pragma unroll
  for (int r = 0; r < 2; ++r) {
    if (!act) return;  // (uniform)
    const int leader = __builtin_amdgcn_readfirstlane(__ffsll((long long)act) - 1);
    const uint32_t c0 = (uint32_t)__builtin_amdgcn_readlane((int)code, leader);
    const unsigned long long same = __ballot(ok && code == c0);
    if (lane == leader) atomicAdd(&s_hist[c0 & 0xFFFFu], (uint32_t)__popcll(same) * (c0 >> 16));
    ok = ok && code != c0;
    act &= ~same;
  }
  if (ok) atomicAdd(&s_hist[addr], run);
}

template <typename T>
__global__ __launch_bounds__(256) void k_key_hist(const T* __restrict__ base, int n1, int64_t stride0, int64_t stride1,
                                                  int64_t unit_len, int64_t chunk_elems, int64_t chunks_per_unit,
                                                  int64_t total_chunks, int shift, int bits, int prefix_shift,
                                                  PcPrefixes pre, int n_pre, unsigned long long* __restrict__ hist) {
  extern __shared__ uint32_t s_hist[];
  constexpr int N = 16 / (int)sizeof(T);
  const int nbins = 1 << bits, n_tab = n_pre > 0 ? n_pre : 1, lane = threadIdx.x & 63;
  const uint32_t mask = (uint32_t)nbins - 1u;
  for (int b = threadIdx.x; b < n_tab * nbins; b += 256) s_hist[b] = 0u;
  __syncthreads();
  for (int64_t c = blockIdx.x; c < total_chunks; c += gridDim.x) {  // (everything about the chunk is uniform)
    const int64_t u = c / chunks_per_unit, e0 = (c - u * chunks_per_unit) * chunk_elems;
    const int64_t i0 = u / n1, i1 = u - i0 * n1;
    const T* p = base + i0 * stride0 + i1 * stride1;
    const int64_t left = min(chunk_elems, unit_len - e0);
    const int rounds = (int)((left + 256 * N - 1) / (256 * N));
    for (int r = 0; r < rounds; ++r) {
      const int64_t e = e0 + ((int64_t)r * 256 + threadIdx.x) * N;
      const int nv = (int)max((int64_t)0, min((int64_t)N, unit_len - e));
      T x[N];
      if (nv == N && (reinterpret_cast<uintptr_t>(p + e) & 15) == 0) {
        const uint4 v = *reinterpret_cast<const uint4*>(p + e);
        __builtin_memcpy(x, &v, 16);
      } else {
#pragma unroll
        for (int j = 0; j < N; ++j) x[j] = j < nv ? p[e + j] : (T)0;
      }
      uint32_t addr[N];  // the table slot of every element; PC_NONE: not counted
#pragma unroll
      for (int j = 0; j < N; ++j) {
        uint32_t key = 0u;
        bool ok = pc_key<T>(x[j], key) && j < nv;
        uint32_t a = (key >> shift) & mask;
        if (n_pre > 0) {  // (uniform) a refinement: only inside a selected prefix, in that prefix's table
          const uint32_t hi = key >> prefix_shift;
          int t = -1;
#pragma unroll
          for (int q = 0; q < MG_PERCENTILE_MAX_PREFIXES; ++q)
            if (q < n_pre && hi == pre.v[q]) t = q;
          ok = ok && t >= 0;
          a += (uint32_t)(t < 0 ? 0 : t) * (uint32_t)nbins;
        }
        addr[j] = ok ? a : PC_NONE;
      }
      // runs of equal slots among the lane's neighbouring elements are counted in the lane; a run that ends inside the
      // vector is added at once (few lanes at a time), the last one through the wave's gather
      uint32_t run = 0u;
#pragma unroll
      for (int j = 0; j < N; ++j) {
        run += addr[j] != PC_NONE;
        if (j + 1 < N) {
          if (run && addr[j + 1] != addr[j]) {
            atomicAdd(&s_hist[addr[j]], run);
            run = 0u;
          }
        } else {
          pc_count_wave(s_hist, addr[j], run, run != 0u, lane);
        }
      }
    }
  }
  __syncthreads();
  for (int b = threadIdx.x; b < n_tab * nbins; b += 256) {
    const uint32_t n = s_hist[b];
    if (n) atomicAdd(&hist[b], (unsigned long long)n);
  }
}

}  // namespace

extern "C" int mg_percentile_histogram(const void* d_data, int dtype, int n0, int64_t stride0, int n1, int64_t stride1,
                                       int64_t unit_len, int shift, int bits, int prefix_shift, const uint32_t* prefixes,
                                       int n_prefixes, uint64_t* d_hist, void* stream) {
  const int key_bits = dtype == MG_U8 ? 8 : dtype == MG_U16 ? 16 : (dtype == MG_F32 || dtype == MG_F64) ? 32 : 0;
  if (!key_bits || !d_hist || n0 < 0 || n1 < 0 || unit_len < 0 || stride0 < 0 || stride1 < 0 || bits < 1 ||
      bits > PC_MAX_BITS || shift < 0 || shift + bits > key_bits || n_prefixes < 0 || n_prefixes > MG_PERCENTILE_MAX_PREFIXES)
    return MG_EINVAL;
  PcPrefixes pre = {};
  if (n_prefixes == 0) {
    if (shift + bits != key_bits) return MG_EINVAL;  // the first pass counts the leading bits
    prefix_shift = 0;
  } else {
    if (!prefixes || prefix_shift != shift + bits || prefix_shift >= key_bits) return MG_EINVAL;
    for (int q = 0; q < n_prefixes; ++q) {
      if ((uint64_t)prefixes[q] >> (key_bits - prefix_shift)) return MG_EINVAL;
      for (int k = 0; k < q; ++k)
        if (prefixes[k] == prefixes[q]) return MG_EINVAL;
      pre.v[q] = prefixes[q];
    }
  }
  if (n0 == 0 || n1 == 0 || unit_len == 0) return MG_OK;
  if (!d_data) return MG_EINVAL;
  const int64_t units = (int64_t)n0 * n1, vec = 16 / mg_elem_size(dtype), vpu = (unit_len + vec - 1) / vec;
  const int64_t rounds = std::min<int64_t>(8, (vpu + 255) / 256), chunk_elems = 256 * rounds * vec;
  const int64_t cpu = (unit_len + chunk_elems - 1) / chunk_elems;
  if (cpu > INT64_MAX / units) return MG_EINVAL;
  const int64_t total = units * cpu;
  const int blocks = (int)std::min<int64_t>(total, MG_PERCENTILE_WALK);
  // a workgroup's uint32 bins hold what it counts: at most ceil(total / blocks) chunks
  if ((total + blocks - 1) / blocks > (int64_t)0xFFFFFFFFLL / chunk_elems) return MG_EINVAL;
  const size_t lds = (size_t)(n_prefixes > 0 ? n_prefixes : 1) * ((size_t)1 << bits) * sizeof(uint32_t);
  hipStream_t s = mg_stream(stream);
  return mg_dispatch_pixel(dtype, [&](auto t) {
    using T = decltype(t);
    hipLaunchKernelGGL((k_key_hist<T>), dim3(blocks), dim3(256), lds, s, (const T*)d_data, n1, stride0, stride1, unit_len,
                       chunk_elems, cpu, total, shift, bits, prefix_shift, pre, n_prefixes,
                       reinterpret_cast<unsigned long long*>(d_hist));
    MG_CHECK_LAUNCH();
    return MG_OK;
  });
}
