// Blobs: connected-component labelling of a thresholded plane, selection by area / border, hole filling
// (include/magnify_hip.h "Blobs"; tests/blobs_ref.py restates every rule).
//
// mg_blob_labels is seven launches on one stream, none of which waits for another workgroup:
//   k_blob_clear     d_num, d_status = 0
//   k_blob_tiles     a 32 x 64 tile per workgroup: threshold while loading, rows bit-packed, union-find in LDS;
//                    d_labels[i] = linear index of the smallest pixel of i's component inside the tile (-1: off)
//   k_blob_seams     unions across the tile borders on that parent array: agent-scope atomics only
//   k_blob_compress  every on pixel points at its root; roots counted per block of 1024 pixels
//   k_blob_scan      one workgroup: exclusive scan of the block counts, K, overflow
//   k_blob_number    root r <- -(number) - 3 in place, its statistics row initialised
//   k_blob_flatten   every on pixel takes its root's number; statistics summed per block in LDS, then integer atomics
// The invariant all of them keep: a parent word of an on pixel i holds an index p <= i of the same component.
#include "mg_common.h"

namespace {

constexpr int TH = MG_BLOB_TILE_H, TW = MG_BLOB_TILE_W, TPX = TH * TW;
constexpr int NT = 256, PPT = 8;   // tile pass: 8 consecutive pixels of one row per thread
constexpr int CHUNK = 4 * NT;      // counting / numbering: pixels per block, as 4 rounds of 256 consecutive ones
static_assert(TW == 64 && TPX == NT * PPT, "a tile row is one 64-bit word; 256 threads x 8 pixels cover the tile");

template <class T>
__device__ __forceinline__ bool blob_on(T v, double thr, int below) {
  const double d = (double)v;
  return below ? d < thr : d > thr;  // NaN: false both ways
}

template <class T>
struct alignas(sizeof(T) * PPT > 16 ? 16 : sizeof(T) * PPT) BlobVec {
  T v[PPT];
};

// Start of the run of set bits of `row` that holds bit x (which is set).
__device__ __forceinline__ int run_start(uint64_t row, int x) {
  const uint64_t z = ~row & ((1ull << x) - 1ull);
  return z ? 64 - __clzll((long long)z) : 0;
}

// ---- union-find in LDS (coherent inside the workgroup).  A find path strictly descends, so it has fewer than TPX
// steps; a union's larger operand strictly descends from one trip to the next, so it has fewer than 2 TPX trips.
__device__ __forceinline__ uint32_t lds_find(uint32_t* lab, uint32_t a, bool& bad) {
  for (int it = 0; it < TPX; ++it) {
    const uint32_t p = __hip_atomic_load(&lab[a], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    if (p == a) return a;
    a = p;
  }
  bad = true;
  return a;
}
__device__ __forceinline__ void lds_unite(uint32_t* lab, uint32_t a, uint32_t b, bool& bad) {
  for (int it = 0; it < 2 * TPX; ++it) {
    a = lds_find(lab, a, bad);
    b = lds_find(lab, b, bad);
    if (a == b || bad) return;
    if (a < b) {
      const uint32_t t = a;
      a = b, b = t;
    }
    const uint32_t old = __hip_atomic_fetch_min(&lab[a], b, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    if (old == a) return;  // a was a root and now hangs under b
    a = old;               // a had a parent already: what is left is union(that parent, b)
  }
  bad = true;
}

__global__ void k_blob_clear(int32_t* d_num, int32_t* d_status) {
  *d_num = 0;
  *d_status = 0;
}

// LDS: 2048 labels x 4 B (a tile row = 64 dwords = one bank row: the lanes of a wave read consecutive banks, also
// for the row above) + 33 row words = 8456 B a workgroup.
template <class T>
__global__ __launch_bounds__(NT) void k_blob_tiles(const T* __restrict__ img, int h, int w, double thr, int below,
                                                   int conn8, int tiles_x, int32_t* __restrict__ labels,
                                                   int32_t* d_status) {
  __shared__ uint64_t s_row[TH + 1];  // [0]: the (empty) row above the tile
  __shared__ uint32_t s_lab[TPX];
  const int t = threadIdx.x, ly = t >> 3, lx0 = (t & 7) * PPT;
  const int ty = blockIdx.x / tiles_x, tx = blockIdx.x - ty * tiles_x;
  const int gy = ty * TH + ly, gx0 = tx * TW + lx0;
  uint32_t m = 0;
  if (gy < h && gx0 < w) {
    const T* p = img + (int64_t)gy * w + gx0;
    if (gx0 + PPT <= w && (reinterpret_cast<uintptr_t>(p) & (alignof(BlobVec<T>) - 1)) == 0) {
      const BlobVec<T> v = *reinterpret_cast<const BlobVec<T>*>(p);
#pragma unroll
      for (int j = 0; j < PPT; ++j) m |= (uint32_t)blob_on(v.v[j], thr, below) << j;
    } else {
      for (int j = 0; j < PPT && gx0 + j < w; ++j) m |= (uint32_t)blob_on(p[j], thr, below) << j;
    }
  }
  unsigned long long rb = (unsigned long long)m << lx0;  // the eight threads of a row are eight consecutive lanes
  rb |= __shfl_xor(rb, 1);
  rb |= __shfl_xor(rb, 2);
  rb |= __shfl_xor(rb, 4);
  if ((t & 7) == 0) s_row[ly + 1] = rb;
  if (t == 0) s_row[0] = 0;
  __syncthreads();
  const uint64_t up = s_row[ly];
  // every pixel starts under the first pixel of its horizontal run
#pragma unroll
  for (int j = 0; j < PPT; ++j) {
    const int x = lx0 + j;
    if ((rb >> x) & 1) s_lab[ly * TW + x] = (uint32_t)(ly * TW + run_start(rb, x));
  }
  __syncthreads();
  // vertical contacts, one union per stretch of overlap: a contact is left to the pixel on its left (or right) where
  // that pixel has the same contact
  bool bad = false;
  for (int j = 0; j < PPT; ++j) {
    const int x = lx0 + j;
    if (!((rb >> x) & 1)) continue;
    const bool L = x > 0 && ((rb >> (x - 1)) & 1), R = x < TW - 1 && ((rb >> (x + 1)) & 1);
    const bool U = (up >> x) & 1, UL = x > 0 && ((up >> (x - 1)) & 1), UR = x < TW - 1 && ((up >> (x + 1)) & 1);
    const uint32_t a = (uint32_t)(ly * TW + run_start(rb, x));
    if (U) {
      if (!(L && UL)) lds_unite(s_lab, a, (uint32_t)((ly - 1) * TW + run_start(up, x)), bad);
    } else if (conn8) {
      if (UL && !L) lds_unite(s_lab, a, (uint32_t)((ly - 1) * TW + run_start(up, x - 1)), bad);
      if (UR && !R) lds_unite(s_lab, a, (uint32_t)((ly - 1) * TW + run_start(up, x + 1)), bad);
    }
  }
  __syncthreads();
  if (gy < h) {
    int root = -1, root_start = -1;
    for (int j = 0; j < PPT && gx0 + j < w; ++j) {
      const int x = lx0 + j;
      int32_t out = -1;
      if ((rb >> x) & 1) {
        const int s = run_start(rb, x);
        if (s != root_start) root_start = s, root = (int)lds_find(s_lab, (uint32_t)(ly * TW + s), bad);
        out = (int32_t)((int64_t)(ty * TH + (root >> 6)) * w + tx * TW + (root & 63));
      }
      labels[(int64_t)gy * w + gx0 + j] = out;
    }
  }
  if (bad) atomicOr(d_status, MG_BLOB_EBOUND);
}

// ---- the seam pass.  Every access to a parent word is an agent-scope atomic: the L1s and the per-XCD L2s are not
// coherent inside a launch.  A load may return an older value of the word; every value a word ever held is an index of
// the same (final) component that is >= the current one, so a stale load costs steps, never a link: a link is made
// only by the fetch-min, and whether it was made is read from the value the fetch-min returns.
// Bounds: a find path strictly descends through indices below n, so it has fewer than n steps; from one trip of a
// union to the next its larger operand strictly descends (a' = old < a, b' <= b < a), so it has fewer than 2 n trips.
__device__ __forceinline__ int32_t par_load(int32_t* p) {
  return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ bool par_find(int32_t* par, int32_t& a, int64_t n) {
  for (int64_t it = 0; it < n; ++it) {
    const int32_t p = par_load(par + a);
    if (p == a) return true;
    if (p < 0 || p > a) return false;  // not a parent word of this array
    a = p;
  }
  return false;
}
__device__ __forceinline__ bool par_unite(int32_t* par, int32_t a, int32_t b, int64_t n) {
  for (int64_t it = 0; it < 2 * n; ++it) {
    if (!par_find(par, a, n) || !par_find(par, b, n)) return false;
    if (a == b) return true;
    if (a < b) {
      const int32_t t = a;
      a = b, b = t;
    }
    const int32_t old = __hip_atomic_fetch_min(par + a, b, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (old == a) return true;  // a was a root: linked
    a = old;                    // it was not (the load was stale, or another lane was faster): union(old, b) is left
  }
  return false;
}

// Items: the pixels of every row y = 32 k + 31 with a row below it (n_row_seams * w), then those of every column
// x = 64 k + 63 with a column right of it (n_col_seams * h).  A row item joins (y, x) to (y + 1, x - 1 .. x + 1), a
// column item (y, x) to (y - 1 .. y + 1, x + 1): the diagonal contacts at a tile corner are items of both kinds.  A
// contact is left to the neighbouring item on the same seam line where that one has the same contact.
__global__ __launch_bounds__(NT) void k_blob_seams(int32_t* par, int h, int w, int conn8, int64_t row_items,
                                                   int64_t items, int32_t* d_status) {
  const int64_t idx = (int64_t)blockIdx.x * NT + threadIdx.x;
  if (idx >= items) return;
  const int64_t n = (int64_t)h * w;
  bool ok = true;
  if (idx < row_items) {
    const int k = (int)(idx / w), x = (int)(idx - (int64_t)k * w), y = k * TH + TH - 1;
    int32_t* r0 = par + (int64_t)y * w;
    int32_t* r1 = r0 + w;
    const int32_t p = par_load(r0 + x);
    if (p < 0) return;
    const int32_t d = par_load(r1 + x);
    // (a neighbour on the line stands in only from inside the same tile, where the tile pass has joined it to this
    // pixel already: across a tile corner the row item and the column item would each leave the contact to the other)
    const bool L = x % TW != 0 && par_load(r0 + x - 1) >= 0;
    if (d >= 0) {
      if (!(L && par_load(r1 + x - 1) >= 0)) ok = par_unite(par, p, d, n);
    } else if (conn8) {
      const int32_t dl = x > 0 ? par_load(r1 + x - 1) : -1, dr = x + 1 < w ? par_load(r1 + x + 1) : -1;
      if (dl >= 0 && !L) ok = par_unite(par, p, dl, n);
      if (ok && dr >= 0 && !((x + 1) % TW != 0 && par_load(r0 + x + 1) >= 0)) ok = par_unite(par, p, dr, n);
    }
  } else {
    const int64_t j = idx - row_items;
    const int k = (int)(j / h), y = (int)(j - (int64_t)k * h), x = k * TW + TW - 1;
    int32_t* c0 = par + (int64_t)y * w + x;
    const int32_t p = par_load(c0);
    if (p < 0) return;
    const int32_t r = par_load(c0 + 1);
    const bool U = y % TH != 0 && par_load(c0 - w) >= 0;
    if (r >= 0) {
      if (!(U && par_load(c0 - w + 1) >= 0)) ok = par_unite(par, p, r, n);
    } else if (conn8) {
      const int32_t ur = y > 0 ? par_load(c0 - w + 1) : -1, dr = y + 1 < h ? par_load(c0 + w + 1) : -1;
      if (ur >= 0 && !U) ok = par_unite(par, p, ur, n);
      if (ok && dr >= 0 && !((y + 1) % TH != 0 && par_load(c0 + w) >= 0)) ok = par_unite(par, p, dr, n);
    }
  }
  if (!ok) atomicOr(d_status, MG_BLOB_EBOUND);
}

// ---- after the seam launch the forest is fixed: plain loads.  Lanes of this launch rewrite non-root words with the
// root while others walk through them; either value of such a word is an ancestor, and root words are not written.
__global__ __launch_bounds__(NT) void k_blob_compress(int32_t* par, int64_t n, int32_t* __restrict__ block_counts,
                                                      int32_t* d_status) {
  const int64_t base = (int64_t)blockIdx.x * CHUNK;
  int roots = 0;
  bool bad = false;
  for (int j = 0; j < 4; ++j) {
    const int64_t i = base + j * NT + threadIdx.x;
    if (i >= n) break;
    const int32_t p = par_load(par + i);
    if (p < 0) continue;
    if (p == (int32_t)i) {
      ++roots;
      continue;
    }
    int32_t r = p;
    if (!par_find(par, r, n)) bad = true;  // (a path strictly descends: fewer than n steps)
    if (r != p) par[i] = r;
  }
  const int total = mg_block_fold(roots, [](int a, int b) { return a + b; });
  if (threadIdx.x == 0) block_counts[blockIdx.x] = total;
  if (bad) atomicOr(d_status, MG_BLOB_EBOUND);
}

__global__ __launch_bounds__(1024) void k_blob_scan(int32_t* __restrict__ block_counts, int64_t n_blocks, int64_t cap,
                                                    int32_t* d_num, int32_t* d_status) {
  int64_t carry = 0;
  for (int64_t c0 = 0; c0 < n_blocks; c0 += 1024) {
    const int64_t b = c0 + threadIdx.x;
    const int v = b < n_blocks ? block_counts[b] : 0;
    int total;
    const int ex = mg_block_exscan(v, &total);
    if (b < n_blocks) block_counts[b] = (int32_t)(carry + ex);
    carry += total;
  }
  if (threadIdx.x == 0) {
    *d_num = (int32_t)carry;
    if (carry > cap) atomicOr(d_status, MG_BLOB_OVERFLOW);
  }
}

constexpr int32_t ROOT_CODE = -3;  // root number k is held as ROOT_CODE - k (below the -1 of off and the -2 of select)

__global__ __launch_bounds__(NT) void k_blob_number(int32_t* par, int64_t n, const int32_t* __restrict__ block_prefix,
                                                    int64_t* __restrict__ stats, int64_t cap) {
  const int64_t base = (int64_t)blockIdx.x * CHUNK;
  int run = block_prefix[blockIdx.x];
  for (int j = 0; j < 4; ++j) {  // (uniform: mg_block_exscan synchronises)
    const int64_t i = base + j * NT + threadIdx.x;
    const bool root = i < n && par[i] == (int32_t)i;
    int total;
    const int ex = mg_block_exscan((int)root, &total);
    if (root) {
      const int32_t k = run + ex;
      par[i] = ROOT_CODE - k;
      if (k < cap) {
        int64_t* s = stats + 8 * (int64_t)k;
        s[0] = 0, s[1] = 0, s[2] = 0, s[3] = INT64_MAX, s[4] = INT64_MAX, s[5] = -1, s[6] = -1, s[7] = i;
      }
    }
    run += total;
  }
}

// A lower bound is published only where the word (as last seen: it only descends) is still above it.
__device__ __forceinline__ void stat_min(int64_t* p, int64_t v) {
  if (__hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) > v)
    __hip_atomic_fetch_min(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ void stat_max(int64_t* p, int64_t v) {
  if (__hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) < v)
    __hip_atomic_fetch_max(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

__device__ __forceinline__ void stat_publish(int64_t* s, int64_t area, int64_t sum_y, int64_t sum_x, int64_t y0,
                                             int64_t x0, int64_t y1, int64_t x1) {
  __hip_atomic_fetch_add(s + 0, area, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  __hip_atomic_fetch_add(s + 1, sum_y, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  __hip_atomic_fetch_add(s + 2, sum_x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  stat_min(s + 3, y0);
  stat_min(s + 4, x0);
  stat_max(s + 5, y1);
  stat_max(s + 6, x1);
}

// A non-root word holds its root r (k_blob_compress); the root's word holds ROOT_CODE - k until the root's own lane
// replaces it with k in this launch: a reader takes either form.  Statistics: a wave is 64 consecutive pixels, and the
// first lane of every stretch of one label in one image row adds the stretch -- not to the component's row in memory
// (a component that percolates through the plane has a stretch in nearly every wave: millions of atomics on one
// address) but to the block's table in LDS, FL_SLOTS slots found by the label's hash and linear probing.  A block of
// FL_PX pixels has at most FL_PX stretches, so a label always finds a slot within FL_SLOTS probes; after a barrier
// every slot in use becomes ONE set of atomics on the component's row.  40 bytes a slot: 20 KB a workgroup, which
// leaves the CU its 8 workgroups of 4 waves.
constexpr int FL_PX = 2 * NT, FL_SLOTS = FL_PX;
static_assert(FL_SLOTS == 512, "a slot is found by the top 9 bits of the label's hash and wraps by a mask");
__global__ __launch_bounds__(NT) void k_blob_flatten(int32_t* par, int64_t n, int w, int64_t* stats, int64_t cap) {
  __shared__ int32_t s_key[FL_SLOTS], s_y0[FL_SLOTS], s_x0[FL_SLOTS], s_y1[FL_SLOTS], s_x1[FL_SLOTS];
  __shared__ uint32_t s_area[FL_SLOTS];
  __shared__ unsigned long long s_sy[FL_SLOTS], s_sx[FL_SLOTS];
  for (int s = threadIdx.x; s < FL_SLOTS; s += NT) {
    s_key[s] = -1, s_area[s] = 0, s_sy[s] = 0, s_sx[s] = 0;
    s_y0[s] = INT32_MAX, s_x0[s] = INT32_MAX, s_y1[s] = -1, s_x1[s] = -1;
  }
  __syncthreads();
  const int lane = threadIdx.x & 63;
  for (int j = 0; j < FL_PX / NT; ++j) {  // (uniform: the shuffles and the ballot are the whole wave's)
    const int64_t i = (int64_t)blockIdx.x * FL_PX + j * NT + threadIdx.x;
    int32_t lab = -1;
    if (i < n) {
      const int32_t v = par[i];
      if (v <= ROOT_CODE) {
        lab = ROOT_CODE - v;
      } else if (v >= 0) {
        const int32_t q = par_load(par + v);
        lab = q <= ROOT_CODE ? ROOT_CODE - q : q;
      }
      if (lab >= 0) par[i] = lab;
    }
    const int y = (int)(i / w), x = (int)(i - (int64_t)y * w);
    const int lab_prev = __shfl_up(lab, 1), y_prev = __shfl_up(y, 1);
    const bool head = lane == 0 || lab != lab_prev || y != y_prev;
    const unsigned long long heads = __ballot(head);
    if (head && lab >= 0 && lab < cap) {
      const unsigned long long above = lane == 63 ? 0ull : heads >> (lane + 1);
      const int len = above ? __ffsll((long long)above) : 64 - lane;
      const unsigned long long sum_y = (unsigned long long)len * (unsigned long long)y;
      const unsigned long long sum_x = (unsigned long long)len * (unsigned long long)x + (unsigned long long)(len * (len - 1) / 2);
      int slot = (int)(((uint32_t)lab * 2654435761u) >> 23) & (FL_SLOTS - 1), probes = 0;
      for (; probes < FL_SLOTS; ++probes) {
        const int32_t seen = atomicCAS(&s_key[slot], -1, lab);
        if (seen == -1 || seen == lab) break;
        slot = (slot + 1) & (FL_SLOTS - 1);
      }
      if (probes < FL_SLOTS) {
        atomicAdd(&s_area[slot], (uint32_t)len);
        atomicAdd(&s_sy[slot], sum_y);
        atomicAdd(&s_sx[slot], sum_x);
        atomicMin(&s_y0[slot], y);
        atomicMin(&s_x0[slot], x);
        atomicMax(&s_y1[slot], y);
        atomicMax(&s_x1[slot], x + len - 1);
      } else {  // (not reached: more labels than stretches)
        stat_publish(stats + 8 * (int64_t)lab, len, (int64_t)sum_y, (int64_t)sum_x, y, x, y, x + len - 1);
      }
    }
  }
  __syncthreads();
  for (int s = threadIdx.x; s < FL_SLOTS; s += NT)
    if (s_key[s] >= 0)
      stat_publish(stats + 8 * (int64_t)s_key[s], s_area[s], (int64_t)s_sy[s], (int64_t)s_sx[s], s_y0[s], s_x0[s], s_y1[s],
                   s_x1[s]);
}

// The on mask alone: 1 where on, 0 where off (fill_holes starts from it).
template <class T>
__global__ __launch_bounds__(NT) void k_blob_threshold(const T* __restrict__ img, int64_t n, double thr, int below,
                                                       uint8_t* __restrict__ on) {
  const int64_t i = (int64_t)blockIdx.x * NT + threadIdx.x;
  if (i < n) on[i] = blob_on(img[i], thr, below);
}

// ---- select ----
__device__ __forceinline__ bool blob_inside(const int64_t* s, int h, int w) {
  return s[3] > 0 && s[4] > 0 && s[5] < h - 1 && s[6] < w - 1;
}
// The largest r with 355 (2 r - 1)^2 <= 452 area (area >= 1: r >= 0 qualifies).
__device__ __forceinline__ int32_t blob_radius(int64_t area) {
  int64_t r = (int64_t)(sqrt((double)area * (113.0 / 355.0)) + 0.5);
  while (r > 0 && 355 * (2 * r - 1) * (2 * r - 1) > 452 * area) --r;
  while (355 * (2 * r + 1) * (2 * r + 1) <= 452 * area) ++r;
  return (int32_t)r;
}

__global__ __launch_bounds__(1024) void k_blob_select(const int64_t* __restrict__ stats, const int32_t* d_num,
                                                      int64_t cap, int h, int w, int64_t min_area, int64_t max_area,
                                                      int clear_border, int32_t* d_num_kept,
                                                      int64_t* __restrict__ stats_out, int32_t* __restrict__ table,
                                                      int32_t* __restrict__ remap) {
  const int64_t k_all = *d_num < cap ? *d_num : cap;
  int64_t carry = 0;
  for (int64_t c0 = 0; c0 < k_all; c0 += 1024) {
    const int64_t k = c0 + threadIdx.x;
    bool keep = false;
    const int64_t* s = stats + 8 * k;
    if (k < k_all) {
      const int64_t area = s[0];
      keep = area >= min_area && area >= 1 && (max_area <= 0 || area <= max_area) && (!clear_border || blob_inside(s, h, w));
    }
    int total;
    const int ex = mg_block_exscan((int)keep, &total);
    if (k < k_all) remap[k] = keep ? (int32_t)(carry + ex) : -2;
    if (keep) {
      const int64_t m = carry + ex, area = s[0];
      for (int f = 0; f < 8; ++f) stats_out[8 * m + f] = s[f];
      table[3 * m] = (int32_t)((2 * s[1] + area) / (2 * area));
      table[3 * m + 1] = (int32_t)((2 * s[2] + area) / (2 * area));
      table[3 * m + 2] = blob_radius(area);
    }
    carry += total;
  }
  if (threadIdx.x == 0) *d_num_kept = (int32_t)carry;
}

__global__ __launch_bounds__(NT) void k_blob_remap(int32_t* __restrict__ labels, int64_t n, const int32_t* d_num,
                                                   int64_t cap, const int32_t* __restrict__ remap) {
  const int64_t i = (int64_t)blockIdx.x * NT + threadIdx.x;
  if (i >= n) return;
  const int32_t v = labels[i];
  if (v < 0) return;
  const int64_t k_all = *d_num < cap ? *d_num : cap;
  labels[i] = v < k_all ? remap[v] : -2;
}

__global__ __launch_bounds__(NT) void k_blob_fill(const int32_t* __restrict__ clabels, const int64_t* __restrict__ cstats,
                                                  int64_t cap, int h, int w, int64_t n, uint8_t* __restrict__ on) {
  const int64_t i = (int64_t)blockIdx.x * NT + threadIdx.x;
  if (i >= n) return;
  const int32_t c = clabels[i];
  if (c >= 0 && c < cap && blob_inside(cstats + 8 * (int64_t)c, h, w)) on[i] = 1;
}

struct BlobShape {
  int64_t n, tiles, n_blocks, row_items, items;
  int tiles_x;
};
// false: not a plane this family takes (h * w beyond int32).  No grid of the family reaches a launch limit then: the
// largest (k_blob_threshold, k_blob_remap, k_blob_fill: one workgroup per 256 pixels) stays below 2^23 workgroups of
// 256 threads.
bool blob_shape(int h, int w, BlobShape* s) {
  if (h < 1 || w < 1 || (int64_t)h * w > INT32_MAX) return false;
  s->n = (int64_t)h * w;
  s->tiles_x = (w + TW - 1) / TW;
  s->tiles = (int64_t)((h + TH - 1) / TH) * s->tiles_x;
  s->n_blocks = (s->n + CHUNK - 1) / CHUNK;
  s->row_items = (int64_t)((h - 1) / TH) * w;
  s->items = s->row_items + (int64_t)((w - 1) / TW) * h;
  const int64_t limit = (1ll << 32) / NT;  // blocks x threads stays below 2^32
  return s->tiles < limit && (s->n + NT - 1) / NT < limit && (s->items + NT - 1) / NT < limit;
}

}  // namespace

extern "C" int64_t mg_blob_scratch_bytes(int h, int w, int64_t cap) {
  BlobShape s;
  if (!blob_shape(h, w, &s) || cap < 1) return MG_EINVAL;
  return ((s.n_blocks * 4 + 15) / 16) * 16;
}

extern "C" int mg_blob_labels(const void* d_plane, int dtype, int h, int w, double threshold, int below,
                              int connectivity, int32_t* d_labels, int32_t* d_num, int64_t* d_stats, int64_t cap,
                              int32_t* d_status, void* d_scratch, int64_t scratch_bytes, void* stream) {
  BlobShape s;
  if (!d_plane || !d_labels || !d_num || !d_stats || !d_status || !d_scratch) return MG_EINVAL;
  if (!blob_shape(h, w, &s) || cap < 1 || (connectivity != 4 && connectivity != 8) || threshold != threshold) return MG_EINVAL;
  if (dtype != MG_U8 && dtype != MG_U16 && dtype != MG_F32 && dtype != MG_F64) return MG_EINVAL;
  if (scratch_bytes < mg_blob_scratch_bytes(h, w, cap)) return MG_EINVAL;
  if ((reinterpret_cast<uintptr_t>(d_scratch) & 15) || (reinterpret_cast<uintptr_t>(d_stats) & 7) ||
      (reinterpret_cast<uintptr_t>(d_plane) & (mg_elem_size(dtype) - 1)))
    return MG_EINVAL;
  hipStream_t st = mg_stream(stream);
  int32_t* counts = reinterpret_cast<int32_t*>(d_scratch);
  const int conn8 = connectivity == 8;
  hipLaunchKernelGGL(k_blob_clear, dim3(1), dim3(1), 0, st, d_num, d_status);
  MG_CHECK_LAUNCH();
  const int rc = mg_dispatch_pixel(dtype, [&](auto tag) {
    using T = decltype(tag);
    hipLaunchKernelGGL(k_blob_tiles<T>, dim3((unsigned)s.tiles), dim3(NT), 0, st, reinterpret_cast<const T*>(d_plane), h,
                       w, threshold, below != 0, conn8, s.tiles_x, d_labels, d_status);
    MG_CHECK_LAUNCH();
    return MG_OK;
  });
  if (rc != MG_OK) return rc;
  if (s.items > 0) {
    hipLaunchKernelGGL(k_blob_seams, dim3((unsigned)((s.items + NT - 1) / NT)), dim3(NT), 0, st, d_labels, h, w, conn8,
                       s.row_items, s.items, d_status);
    MG_CHECK_LAUNCH();
  }
  hipLaunchKernelGGL(k_blob_compress, dim3((unsigned)s.n_blocks), dim3(NT), 0, st, d_labels, s.n, counts, d_status);
  MG_CHECK_LAUNCH();
  hipLaunchKernelGGL(k_blob_scan, dim3(1), dim3(1024), 0, st, counts, s.n_blocks, cap, d_num, d_status);
  MG_CHECK_LAUNCH();
  hipLaunchKernelGGL(k_blob_number, dim3((unsigned)s.n_blocks), dim3(NT), 0, st, d_labels, s.n, counts, d_stats, cap);
  MG_CHECK_LAUNCH();
  hipLaunchKernelGGL(k_blob_flatten, dim3((unsigned)((s.n + FL_PX - 1) / FL_PX)), dim3(NT), 0, st, d_labels, s.n, w, d_stats, cap);
  MG_CHECK_LAUNCH();
  return MG_OK;
}

extern "C" int mg_blob_threshold(const void* d_plane, int dtype, int h, int w, double threshold, int below, uint8_t* d_on,
                                 void* stream) {
  BlobShape s;
  if (!d_plane || !d_on || !blob_shape(h, w, &s) || threshold != threshold) return MG_EINVAL;
  if (reinterpret_cast<uintptr_t>(d_plane) & (mg_elem_size(dtype) - 1)) return MG_EINVAL;
  return mg_dispatch_pixel(dtype, [&](auto tag) {
    using T = decltype(tag);
    hipLaunchKernelGGL(k_blob_threshold<T>, dim3((unsigned)((s.n + NT - 1) / NT)), dim3(NT), 0, mg_stream(stream),
                       reinterpret_cast<const T*>(d_plane), s.n, threshold, below != 0, d_on);
    MG_CHECK_LAUNCH();
    return MG_OK;
  });
}

extern "C" int mg_blob_select(int32_t* d_labels, int h, int w, const int64_t* d_stats, const int32_t* d_num, int64_t cap,
                              int64_t min_area, int64_t max_area, int clear_border, int32_t* d_num_kept,
                              int64_t* d_stats_out, int32_t* d_table, int32_t* d_remap, void* stream) {
  BlobShape s;
  if (!d_labels || !d_stats || !d_num || !d_num_kept || !d_stats_out || !d_table || !d_remap) return MG_EINVAL;
  if (!blob_shape(h, w, &s) || cap < 1 || min_area < 0 || max_area < 0 || d_stats_out == d_stats) return MG_EINVAL;
  hipStream_t st = mg_stream(stream);
  hipLaunchKernelGGL(k_blob_select, dim3(1), dim3(1024), 0, st, d_stats, d_num, cap, h, w, min_area, max_area,
                     clear_border != 0, d_num_kept, d_stats_out, d_table, d_remap);
  MG_CHECK_LAUNCH();
  hipLaunchKernelGGL(k_blob_remap, dim3((unsigned)((s.n + NT - 1) / NT)), dim3(NT), 0, st, d_labels, s.n, d_num, cap, d_remap);
  MG_CHECK_LAUNCH();
  return MG_OK;
}

extern "C" int mg_blob_fill_holes(const int32_t* d_clabels, const int64_t* d_cstats, int64_t cap, int h, int w,
                                  uint8_t* d_on, void* stream) {
  BlobShape s;
  if (!d_clabels || !d_cstats || !d_on || !blob_shape(h, w, &s) || cap < 1) return MG_EINVAL;
  hipLaunchKernelGGL(k_blob_fill, dim3((unsigned)((s.n + NT - 1) / NT)), dim3(NT), 0, mg_stream(stream), d_clabels,
                     d_cstats, cap, h, w, s.n, d_on);
  MG_CHECK_LAUNCH();
  return MG_OK;
}
