// A9-A10 on the keyed path: mean_grad / len(perimeter) (utils.py:183-192, 225-251) for the unique circles of
// mg_keys_to_circles, as two kernels.
//
//   k_prefilter  exact rejection of the circles that cannot reach min_roundness -- 99.6 % of them on noisy images.
//                A (persistent, 768-thread) workgroup owns a super-tile of MG_SCORE_SUBY x MG_SCORE_SUBX = 2 x 4 centre
//                tiles (128 x 256 positions); its window of the edge map lives in LDS as
//                ONE BYTE per pixel position: the low nibble is the pixel's gradient-orientation bin (eighths of pi,
//                decided exactly on the integer gradient by mg_canny_nms) or 0xC for "no edge", the high nibble the
//                same for the pixel to its RIGHT (0xC beyond the window's last column or the image).  A lane owns a
//                circle, or two; all circles of a wave have the SAME radius (the keys of a tile are sorted by radius:
//                the block cuts the eight key lists at the radius boundaries and deals tickets of one radius to its
//                waves: 128 consecutive positions, two circles per lane walked together, while a radius has 128 left,
//                then chunks of up to 64; a position finds its key through a per-radius prefix table of the eight
//                sub-tiles, `locate`), so the perimeter walk is straight-line code per radius (template <R>, the midpoint
//                circle evaluated at compile time and matched into read groups, Walk<R>): the offset of a read is the
//                immediate of its ds_read_u8 and the bound tables sit in scalar registers.  Two horizontally adjacent
//                perimeter points come with ONE byte read, at any start column: the horizontal runs of the perimeter
//                cost ceil(L / 2) reads, 15-23 % fewer reads per radius.  Opposite points (p, -p) have the same radial
//                direction mod pi and share a table: the nibbles of a byte and of the byte at the mirrored position
//                form the selector of a v_perm_b32 per table, which looks them up in the 8 signed bytes of the table
//                (0x0C selects the constant 0), and a v_dot4_i32_i8 per table adds the two it owns to the lane's sum.
//                A table byte is an upper bound, in 1/64, of the term a pixel of that bin can contribute to the
//                reference's sum; a circle whose bounds add up to less than min_roundness * P cannot pass (every
//                term <= its bound) and is dropped.  Survivors are appended to a per-plane list.  Bounding roofline:
//                LDS (mg_score_walk_reads(r) byte reads per circle).
//   k_exact      the survivors' reference sum (float64, sequential in perimeter order) in workgroup-level phases over
//                XS = 64 (16 at small batches) survivors: NT / XS lanes per survivor find the edge pixels on its
//                perimeter, a lane lists them in order, all lanes evaluate (survivor, hit) terms -- gradient angles
//                computed on demand from the blurred image exactly as mg_edge_angles does (the dense angle map and
//                its pass are not needed) --, a lane per survivor adds them in order with the reference-exact early
//                exit; score stored float32; circles that pass go to d_alive.
#include <math.h>

#include <algorithm>

#include "mg_common.h"

namespace {

constexpr int NT = 256;
constexpr int NP = 768;  // prefilter block: 12 waves share a window (2 blocks per CU by LDS, up to 63.6 KB each: 24 waves per CU)
constexpr int TS = MG_SCORE_TILE;
constexpr int SUBY = MG_SCORE_SUBY, SUBX = MG_SCORE_SUBX, NSUB = SUBY * SUBX;  // centre tiles per super-tile
constexpr int STY = SUBY * TS, STX = SUBX * TS;
constexpr int WSTR = MG_SCORE_WSTRIDE;
constexpr int MAXR = MG_SCORE_MAX_R;
constexpr int MAXP = MG_SCORE_MAX_PAIRS;
constexpr int BIAS = MAXR * WSTR + MAXR;  // immediates BIAS +- (dr * WSTR + dc) are >= 0
constexpr int WBASE = 8192;               // LDS byte offset of the window (>= BIAS: lane addresses stay >= 0)
constexpr int SEGW = 33;                  // radii + 1 per sub-tile in the segment table
static_assert(WBASE >= BIAS && WBASE % 16 == 0, "window base");
static_assert(STX + 2 * MAXR <= WSTR && (WSTR % 4) == 0 && ((WSTR / 4) & 1) == 1, "window stride");
static_assert(2 * BIAS < 65536, "DS immediates are 16 bits");

// First point (dr, dc) of every pair of opposite perimeter points of radius R, in the order of
// mg_score_pair_table (mg_tables.hip: score_pairs) -- the reference's midpoint walk, utils.py:433-465.
template <int R>
struct Pairs {
  int n;
  int dr[MAXP], dc[MAXP];
  constexpr Pairs() : n(0), dr{}, dc{} {
    put(0, -R);
    put(-R, 0);
    int x = 1, y = -R;
    while (x < -y) {
      put(x, y);
      put(y, x);
      put(-x, y);
      put(-y, x);
      if (x * x + y * y - R * R <= 0) {
        ++x;
      } else {
        ++y;
        ++x;
      }
    }
    if (y == -x) {
      put(x, y);
      put(-x, y);
    }
  }
  constexpr void put(int a, int b) {
    dr[n] = a;
    dc[n] = b;
    ++n;
  }
};

// Read groups of the walk of radius R.  A window byte holds its own pixel's bin in the low nibble and the right
// neighbour's in the high one, so ONE byte read returns two horizontally adjacent perimeter points.  The 2 * P.n points
// (the first points of Pairs<R> and their opposites) are matched row by row: the rows above the centre are cut into
// maximal runs of consecutive columns and a run is paired from its left end; the mirrored run (row -dr) is thereby
// paired from its right end, and the opposite of every pair is a pair.  A group is
//   a quad    the points (dr, dc), (dr, dc + 1) and their opposites: byte reads at (dr, dc) and (-dr, -dc - 1);
//   a single  what a run of odd length leaves over, and (0, -R): the point and its opposite, a byte read each.
// A run may mix first points and opposites (the top run through (-R, 0)): every point carries the index of its pair
// for the bound table.
template <int R>
struct Walk {
  int n;                   // groups: two byte reads each
  int off[MAXP];           // dr * WSTR + dc of the group's (left) point
  int k1[MAXP], k2[MAXP];  // pair index of the left point; of its right neighbour, -1 in a single
  int pts[MAXP];           // perimeter points added up to and including the group
  constexpr Walk() : n(0), off{}, k1{}, k2{}, pts{} {
    const Pairs<R> P{};
    for (int row = -R; row <= 0; ++row) {
      int at[2 * R + 2] = {};  // pair index + 1 of the perimeter point in column c - R of this row
      for (int k = 0; k < P.n; ++k)
        for (int sg = -1; sg <= 1; sg += 2) {
          const int dr = sg * P.dr[k], dc = sg * P.dc[k];
          if (dr == row && (row < 0 || dc < 0)) at[dc + R] = k + 1;
        }
      for (int c = 0; c <= 2 * R;) {
        if (!at[c]) {
          ++c;
          continue;
        }
        const bool quad = at[c + 1] != 0;
        off[n] = row * WSTR + (c - R);
        k1[n] = at[c] - 1;
        k2[n] = quad ? at[c + 1] - 1 : -1;
        ++n;
        c += quad ? 2 : 1;
      }
    }
    // in the order of the tables (a quad: of its lower index), which the scalar loads then fetch in blocks
    for (int i = 1; i < n; ++i)
      for (int j = i; j > 0 && key(j) < key(j - 1); --j) {
        swap(off[j], off[j - 1]);
        swap(k1[j], k1[j - 1]);
        swap(k2[j], k2[j - 1]);
      }
    for (int g = 0; g < n; ++g) pts[g] = (g ? pts[g - 1] : 0) + (k2[g] >= 0 ? 4 : 2);
  }
  constexpr int key(int g) const { return k2[g] >= 0 && k2[g] < k1[g] ? k2[g] : k1[g]; }
  static constexpr void swap(int& a, int& b) {
    const int t = a;
    a = b;
    b = t;
  }
};

typedef unsigned short us2 __attribute__((ext_vector_type(2)));

// Sum of the bounds over the perimeter of the circle whose centre byte sits at lds[va + BIAS]; with TWO, also of a
// second circle of the same radius at vb: the two walks share the scalar table loads and the v_mov that brings a
// table half to the v_perm (one SGPR operand per VOP3), and their LDS reads overlap.
// Per group the two bytes A (at the left point, low half) and B (at the mirrored left point, high half) are split
// into the nibbles [A.lo, A.hi, B.lo, B.hi] = the selector of a v_perm_b32 per table: A.lo and B.hi are the left
// point and its opposite (table k1), A.hi and B.lo the right point and its opposite (table k2); a v_dot4 per table
// adds the two bounds it owns.  A single masks the high nibbles (pixels that are not on the perimeter) away.
// `need`: what the sum has to reach (wave-uniform: a wave's circles share the radius).  A bound is at most 64 per
// point, so a circle with sum + 64 (points not yet added) < need cannot reach it whatever the rest holds; when
// that is true of ALL circles of the wave (both of a lane) -- four checks in the last quarter of the walk: a wave of noise circles
// (81 % of the waves hold no survivor) is out at ~85 % of its perimeter -- the rest is not read.  The sums returned
// then are below `need` like the full ones would be: the same circles are dropped.
template <int R, bool TWO>
__device__ __forceinline__ void score_walk(const uint8_t* lds, int va, int vb, const uint2* __restrict__ tabs, int need, bool valid,
                                           int& sum_a, int& sum_b) {
  constexpr Pairs<R> P{};
  constexpr Walk<R> W{};
  static_assert(P.n <= MAXP, "perimeter too long");
  static_assert(W.pts[W.n - 1] == 2 * P.n, "the perimeter points are distinct and every one is in a group");
  // one group of one circle: two byte reads, the selector, a perm and a dot4 per table
  auto add = [&](int vaddr, int g, const uint2 t1, const uint2 t2, int sum) -> int {
    const bool quad = W.k2[g] >= 0;
    us2 s;
    s.x = lds[vaddr + (BIAS + W.off[g])];
    s.y = lds[vaddr + (BIAS - W.off[g] - (quad ? 1 : 0))];
    const uint32_t v = __builtin_bit_cast(uint32_t, s);
    if (quad) {
      const uint32_t sel = (v | (v << 4)) & 0x0F0F0F0Fu;
      sum = __builtin_amdgcn_sdot4((int)__builtin_amdgcn_perm(t1.y, t1.x, sel), 0x01000001, sum, false);
      return __builtin_amdgcn_sdot4((int)__builtin_amdgcn_perm(t2.y, t2.x, sel), 0x00010100, sum, false);
    }
    const uint32_t q = __builtin_amdgcn_perm(t1.y, t1.x, v & 0x000F000Fu);  // bytes 0 and 2: the two bounds
    return __builtin_amdgcn_sdot4((int)q, 0x00010001, sum, false);
  };
  int sa = 0, sb = 0;
#pragma unroll
  for (int g = 0; g < W.n; ++g) {
    const uint2 t1 = tabs[R * MAXP + W.k1[g]];  // uniform address: scalar loads
    const uint2 t2 = tabs[R * MAXP + (W.k2[g] >= 0 ? W.k2[g] : W.k1[g])];
    sa = add(va, g, t1, t2, sa);
    if (TWO) sb = add(vb, g, t1, t2, sb);
    const int done = g + 1;
    if (P.n >= 16 && done < W.n && (done == (W.n * 12) / 16 || done == (W.n * 13) / 16 || done == (W.n * 14) / 16 || done == (W.n * 15) / 16)) {
      const int rest = 64 * (2 * P.n - W.pts[g]);
      if (__ballot((valid && sa + rest >= need) || (TWO && sb + rest >= need)) == 0) {
        sum_a = sa;
        sum_b = sb;
        return;
      }
    }
  }
  sum_a = sa;
  sum_b = sb;
}

// (one circle per lane, no early exit: the form the micro-benchmarks of the walk use)
template <int R>
__device__ __forceinline__ int score_r(const uint8_t* lds, int vaddr, const uint2* __restrict__ tabs, int need = -(1 << 30),
                                       bool valid = true) {
  int sum, unused;
  score_walk<R, false>(lds, vaddr, vaddr, tabs, need, valid, sum, unused);
  return sum;
}

// ---- prefilter ----------------------------------------------------------------------------------------
// LDS: [0, WBASE) small tables, [WBASE, +side_y * WSTR) the window.
// Survivors are collected per super-tile in LDS and appended to the plane's list with ONE global atomic: a returning
// atomic per wave-with-survivors (~9 000 per plane, all on one address, while only one or two planes are being
// worked on at any time) cost as much as the perimeter walks of a single plane.
constexpr int MAP_OFF = (NSUB * SEGW + SEGW + 32 + 3) * 4, MAP_BYTES = 32 * 4 * 16;
constexpr int SURV_OFF = 3584, SURV_LDS = (WBASE - SURV_OFF) / 8;
static_assert(MAP_OFF % 16 == 0 && MAP_OFF + MAP_BYTES <= SURV_OFF && NSUB == 8, "small tables");

// Position -> key of one radius in a super-tile.  The circles of radius rho are the concatenation of the eight
// sub-tiles' segments of the sorted key lists; map[rho] holds, as four int4 a wave reads with four broadcast
// ds_read_b128, {count, pre[1..7]} (pre[s]: positions before sub-tile s; pre[0] = 0 gives its slot to the count)
// and {first key of segment s - pre[s]}.  Position m lies in the LAST sub-tile with pre[s] <= m (an empty sub-tile
// shares its successor's pre and is never the last): seven compare-selects give the key's index m + dlt[s] and the
// window offset of the sub-tile's corner.
struct KeyAt {
  int i, wo;
};
__device__ __forceinline__ KeyAt locate(int m, const int4 p0, const int4 p1, const int4 d0, const int4 d1) {
  int d = d0.x, wo = 0;
#define MG_STEP(P, D, S)                                    \
  {                                                         \
    const bool c = m >= (P);                                \
    d = c ? (D) : d;                                        \
    wo = c ? ((S) / SUBX) * TS * WSTR + ((S) % SUBX) * TS : wo; \
  }
  MG_STEP(p0.y, d0.y, 1) MG_STEP(p0.z, d0.z, 2) MG_STEP(p0.w, d0.w, 3) MG_STEP(p1.x, d1.x, 4)
  MG_STEP(p1.y, d1.y, 5) MG_STEP(p1.z, d1.z, 6) MG_STEP(p1.w, d1.w, 7)
#undef MG_STEP
  return {m + d, wo};
}

// bits 0..3 of x -> bit 0 of bytes 0..3
__device__ __forceinline__ uint32_t spread4(uint32_t x) { return ((x & 0xFu) * 0x00204081u) & 0x01010101u; }

__global__ __launch_bounds__(NP) __attribute__((amdgpu_waves_per_eu(6))) void k_prefilter(const uint32_t* __restrict__ d_bits, const uint32_t* __restrict__ d_class,
                                                  int64_t words_per_plane, int h, int w,
                                                  const uint32_t* __restrict__ d_ukeys, int64_t circle_cap,
                                                  const int32_t* __restrict__ d_layer_starts, int n_tiles, int ntr, int ntc,
                                                  int nsc, int n_st, int64_t total_st, int min_r, int max_r, int nr,
                                                  const uint2* __restrict__ d_tabs,
                                                  const int32_t* __restrict__ d_per_starts, float min_roundness,
                                                  int write_skipped, float* __restrict__ d_scores,
                                                  int32_t* __restrict__ d_surv, int64_t surv_cap,
                                                  int32_t* __restrict__ d_num_surv) {
  extern __shared__ __attribute__((aligned(16))) uint8_t lds[];
  int32_t* seg = reinterpret_cast<int32_t*>(lds);  // [NSUB][SEGW]: index of the first key of radius rho in sub-tile s
  int32_t* chunk0 = seg + NSUB * SEGW;             // [nr + 1]: first ticket of radius rho
  int32_t* need = chunk0 + SEGW;                   // [nr]: threshold on the sum of bounds (1/64)
  int32_t* next = need + 32;                       // the block's ticket counter
  int32_t* n_held = next + 1;                      // survivors of this super-tile held in LDS (may count past SURV_LDS)
  int32_t* g_base = next + 2;                      // where they go in the plane's list
  int4* map = reinterpret_cast<int4*>(lds + MAP_OFF);    // [nr][4]: position -> key of radius rho (locate)
  int2* held = reinterpret_cast<int2*>(lds + SURV_OFF);  // [SURV_LDS] (index in the key list, key)
  uint8_t* win = lds + WBASE;
  const int side_y = STY + 2 * max_r, side_x = STX + 2 * max_r;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (int i = threadIdx.x; i < nr; i += NP) {
    const int len = d_per_starts[i + 1] - d_per_starts[i];
    // a circle can only pass with sum(terms) >= mg_score_floor, and sum(terms) <= sum(bounds) / 64
    need[i] = (int)ceil(64.0 * mg_score_floor(min_roundness, len));
  }
  const int wgroups_all = (side_x + 31) >> 5;  // 32-pixel groups per window row
  for (int64_t st = blockIdx.x; st < total_st; st += gridDim.x) {
    const int plane = (int)(st / n_st), sidx = (int)(st - (int64_t)plane * n_st);
    const int sr = sidx / nsc, sc = sidx - sr * nsc;
    __syncthreads();  // the previous super-tile's window and tables are no longer read
    // (opaque: what a thread derives from its index for the tables and the window -- rows, columns, addresses -- is
    // worked out again for every super-tile instead of being kept in ~20 registers through the walks, which need them)
    int tid = threadIdx.x, wgroups = wgroups_all, nr1 = nr + 1;
    asm volatile("" : "+v"(tid), "+s"(wgroups), "+s"(nr1));
    // ---- segment table: first key of every radius in the sub-tiles' sorted lists (mg_keys_to_circles) ----
    if (tid < NSUB * nr1) {
      const int s = tid / nr1, q = tid - s * nr1;
      const int tr = SUBY * sr + s / SUBX, tc = SUBX * sc + s % SUBX;
      int v = 0;
      if (tr < ntr && tc < ntc) v = d_layer_starts[((int64_t)plane * n_tiles + tr * ntc + tc) * nr1 + q];
      seg[s * SEGW + q] = v;  // a sub-tile beyond the grid: all zero = empty
    }
    if (threadIdx.x == 0) *next = 0, *n_held = 0;
    // ---- the window: orientation bin of every edge pixel, 0x0C elsewhere.  All loads of a thread's (at most
    // WI) 32-pixel groups are issued before the first is used: the block would otherwise wait for two to four
    // global round trips per group, one after the other ----
    const int wy0 = sr * STY - 2 * max_r, wx0 = sc * STX - 2 * max_r;
    {
      const uint32_t* pl[4] = {d_bits + plane * words_per_plane, d_class + (3 * plane) * words_per_plane,
                               d_class + (3 * plane + 1) * words_per_plane, d_class + (3 * plane + 2) * words_per_plane};
      constexpr int WI = ((STY + 2 * MAXR) * ((WSTR + 31) / 32) + NP - 1) / NP;
      uint32_t lo[WI][4], hi[WI][4];
#pragma unroll
      for (int it = 0; it < WI; ++it) {
        const int i = tid + it * NP;
        const int j = i / wgroups, k = i - j * wgroups;
        const int y = wy0 + j, xs = wx0 + 32 * k;
        const int x_lo = max(xs, 0), x_hi = min(min(xs + 33, wx0 + side_x), w);  // (33: the last pixel's right neighbour)
        const bool live = i < side_y * wgroups && y >= 0 && y < h && x_lo < x_hi;
        const int64_t wi = live ? ((int64_t)y * w + x_lo) >> 5 : 0;
#pragma unroll
        for (int c = 0; c < 4; ++c) {
          lo[it][c] = pl[c][wi];
          hi[it][c] = pl[c][wi + 1];  // (the bitmaps carry one spare word)
        }
      }
#pragma unroll
      for (int it = 0; it < WI; ++it) {
        const int i = tid + it * NP;
        if (i >= side_y * wgroups) break;
        const int j = i / wgroups, k = i - j * wgroups;
        const int y = wy0 + j, xs = wx0 + 32 * k;
        const int x_lo = max(xs, 0), x_hi = min(min(xs + 33, wx0 + side_x), w);
        // edge bit, c0, c1, c2 of the group's 32 pixels and (nb) of the pixel to their right: a pixel beyond the
        // window's last column or outside the image is "no edge" as a neighbour too
        uint32_t pv[4] = {0u, 0u, 0u, 0u}, nb[4] = {0u, 0u, 0u, 0u};
        if (y >= 0 && y < h && x_lo < x_hi) {
          const int sh = (int)(((int64_t)y * w + x_lo) & 31), n = x_hi - x_lo;  // 1 <= n <= 33
          const uint64_t keep = (1ull << n) - 1ull;
#pragma unroll
          for (int c = 0; c < 4; ++c) {
            const uint64_t v = ((((((uint64_t)hi[it][c]) << 32) | lo[it][c]) >> sh) & keep) << (x_lo - xs);
            pv[c] = (uint32_t)v;
            nb[c] = (uint32_t)(v >> 32);
          }
        }
        uint32_t* rowp = reinterpret_cast<uint32_t*>(win + j * WSTR) + 8 * k;
        const int nd = min(8, (WSTR >> 2) - 8 * k);  // dwords of this group inside the row
        // four pixels -> four bytes: bin = 4 c1 + 2 c0 + c2 where the pixel is an edge, else 0x0C
        auto bins4 = [](uint32_t e, uint32_t c0, uint32_t c1, uint32_t c2) -> uint32_t {
          const uint32_t m = spread4(e) * 0xFFu;
          return ((4u * spread4(c1) + 2u * spread4(c0) + spread4(c2)) & m) | (0x0C0C0C0Cu & ~m);
        };
        uint32_t own = bins4(pv[0], pv[1], pv[2], pv[3]);
#pragma unroll
        for (int q = 0; q < 8; ++q) {
          if (q >= nd) break;
          // (dword 8: only its first byte, the neighbour pixel, is used)
          const uint32_t nxt = q < 7 ? bins4(pv[0] >> (4 * q + 4), pv[1] >> (4 * q + 4), pv[2] >> (4 * q + 4), pv[3] >> (4 * q + 4))
                                     : bins4(nb[0], nb[1], nb[2], nb[3]);
          // byte = own bin | right neighbour's bin << 4 (bins are <= 0x0C: nothing crosses a byte)
          rowp[q] = own | (__builtin_amdgcn_alignbyte(nxt, own, 1) << 4);
          own = nxt;
        }
      }
    }
    const uint32_t* ukeys = d_ukeys + (int64_t)plane * circle_cap;
    __syncthreads();
    if (wave == 0) {  // the radii's position maps and tickets: 128 circles each while 128 are left, then 64 (or fewer)
      int cnt = 0;
      if (lane < nr) {
        int pre[NSUB], dlt[NSUB];
#pragma unroll
        for (int s = 0; s < NSUB; ++s) {
          const int a = seg[s * SEGW + lane];
          pre[s] = cnt;
          dlt[s] = a - cnt;
          cnt += seg[s * SEGW + lane + 1] - a;
        }
        map[4 * lane + 0] = make_int4(cnt, pre[1], pre[2], pre[3]);
        map[4 * lane + 1] = make_int4(pre[4], pre[5], pre[6], pre[7]);
        map[4 * lane + 2] = make_int4(dlt[0], dlt[1], dlt[2], dlt[3]);
        map[4 * lane + 3] = make_int4(dlt[4], dlt[5], dlt[6], dlt[7]);
      }
      const int tickets = (cnt >> 7) + (((cnt & 127) + 63) >> 6);
      const int incl = mg_wave_scan_incl_i32(tickets);
      if (lane < nr) chunk0[lane] = incl - tickets;
      if (lane == nr - 1) chunk0[nr] = incl;
    }
    __syncthreads();
    const int total_tickets = chunk0[nr];
    // Ticket loop, software-pipelined: the keys of the NEXT ticket are requested before the current one is scored
    // (a wave's tickets are otherwise one global round trip each).  A ticket is 64 positions of one radius, a
    // circle per lane (A), or 128, two per lane (A: position m, B: m + 64), walked together: the two circles share
    // the ticket, the radius decode, the map, the switch and the walk's scalar table loads.
    int rho_n = 0;
    bool two_n = false, valid_n = false;
    KeyAt a_n = {0, 0}, b_n = {0, 0};
    uint32_t key_an = 0, key_bn = 0;
    auto fetch = [&]() -> bool {
      int c = 0;
      if (lane == 0) c = atomicAdd(next, 1);
      c = __builtin_amdgcn_readfirstlane(c);
      if (c >= total_tickets) return false;
      // the ticket's radius: the last rho with chunk0[rho] <= c (empty radii share their successor's start)
      rho_n = __builtin_popcountll(__ballot(lane < nr && chunk0[lane] <= c)) - 1;
      const int4 p0 = map[4 * rho_n], p1 = map[4 * rho_n + 1], d0 = map[4 * rho_n + 2], d1 = map[4 * rho_n + 3];
      const int cnt = __builtin_amdgcn_readfirstlane(p0.x), t = c - __builtin_amdgcn_readfirstlane(chunk0[rho_n]);
      const int nd = cnt >> 7;  // double tickets of this radius; then singles
      two_n = t < nd;
      const int m = 64 * (t + min(t, nd)) + lane;
      valid_n = m < cnt;
      a_n = locate(m, p0, p1, d0, d1);
      if (!valid_n) a_n.i = 0;
      key_an = ukeys[a_n.i];  // (an idle lane reads a valid address: no branch around the load)
      if (two_n) {            // (all 128 positions exist)
        b_n = locate(m + 64, p0, p1, d0, d1);
        key_bn = ukeys[b_n.i];
      }
      return true;
    };
    // sum against need -> the survivors of a chunk to the block's list
    auto hand_over = [&](bool valid, int sum, int need_rho, int i, uint32_t key) {
      const bool pass = valid && sum >= need_rho;
      if (write_skipped && valid && !pass) d_scores[(int64_t)plane * circle_cap + i] = MG_SCORE_SKIPPED;
      const uint64_t pm = __ballot(pass);
      if (pm) {  // rare: hold the survivors in LDS until the super-tile is done
        int hbase = 0;
        if (lane == 0) hbase = atomicAdd(n_held, __builtin_popcountll(pm));
        hbase = __builtin_amdgcn_readfirstlane(hbase);
        const int slot = hbase + __builtin_amdgcn_mbcnt_hi((uint32_t)(pm >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)pm, 0u));
        if (pass && slot < SURV_LDS) held[slot] = make_int2((int32_t)i, (int32_t)key);
        const uint64_t om = __ballot(pass && slot >= SURV_LDS);
        if (om) {  // LDS full (hundreds of survivors in one super-tile): straight to the plane's list
          int sbase = 0;
          if (lane == 0) sbase = atomicAdd(&d_num_surv[plane], __builtin_popcountll(om));
          sbase = __builtin_amdgcn_readfirstlane(sbase);
          const int rank = __builtin_amdgcn_mbcnt_hi((uint32_t)(om >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)om, 0u));
          if (pass && slot >= SURV_LDS && (int64_t)sbase + rank < surv_cap)
            reinterpret_cast<int2*>(d_surv)[(int64_t)plane * surv_cap + sbase + rank] = make_int2((int32_t)i, (int32_t)key);
        }
      }
    };
    const int corner = WBASE - BIAS + max_r * (WSTR + 1);  // window byte of a sub-tile's position (0, 0), less BIAS
    bool have = fetch();
    while (have) {
      const int rho = rho_n;
      const bool two = two_n, valid = valid_n;
      const KeyAt a = a_n, b = b_n;
      const uint32_t key_a = valid ? key_an : 0u, key_b = key_bn;
      have = fetch();
      const int va = corner + a.wo + mg_key_row(key_a) * WSTR + mg_key_col(key_a);
      int sum_a = 0, sum_b = 0;
      const int need_rho = need[rho];
      if (two) {
        const int vb = corner + b.wo + mg_key_row(key_b) * WSTR + mg_key_col(key_b);
        switch (rho + min_r) {
#define MG_CASE(R) case R: score_walk<R, true>(lds, va, vb, d_tabs, need_rho, true, sum_a, sum_b); break;
          MG_CASE(2) MG_CASE(3) MG_CASE(4) MG_CASE(5) MG_CASE(6) MG_CASE(7) MG_CASE(8) MG_CASE(9) MG_CASE(10)
          MG_CASE(11) MG_CASE(12) MG_CASE(13) MG_CASE(14) MG_CASE(15) MG_CASE(16) MG_CASE(17) MG_CASE(18)
          MG_CASE(19) MG_CASE(20) MG_CASE(21) MG_CASE(22) MG_CASE(23) MG_CASE(24) MG_CASE(25) MG_CASE(26)
#undef MG_CASE
          default: break;
        }
      } else {
        switch (rho + min_r) {
#define MG_CASE(R) case R: score_walk<R, false>(lds, va, va, d_tabs, need_rho, valid, sum_a, sum_b); break;
          MG_CASE(2) MG_CASE(3) MG_CASE(4) MG_CASE(5) MG_CASE(6) MG_CASE(7) MG_CASE(8) MG_CASE(9) MG_CASE(10)
          MG_CASE(11) MG_CASE(12) MG_CASE(13) MG_CASE(14) MG_CASE(15) MG_CASE(16) MG_CASE(17) MG_CASE(18)
          MG_CASE(19) MG_CASE(20) MG_CASE(21) MG_CASE(22) MG_CASE(23) MG_CASE(24) MG_CASE(25) MG_CASE(26)
#undef MG_CASE
          default: break;
        }
      }
      hand_over(valid, sum_a, need_rho, a.i, key_a);
      if (two) hand_over(true, sum_b, need_rho, b.i, key_b);
    }
    // ---- the super-tile's survivors -> the plane's list ----
    __syncthreads();
    const int n_out = min(*n_held, SURV_LDS);  // block-uniform
    if (n_out > 0) {
      if (threadIdx.x == 0) *g_base = atomicAdd(&d_num_surv[plane], n_out);
      __syncthreads();
      const int64_t gb = *g_base;
      for (int k = threadIdx.x; k < n_out; k += NP)
        if (gb + k < surv_cap) reinterpret_cast<int2*>(d_surv)[(int64_t)plane * surv_cap + gb + k] = held[k];
    }
  }
}

// ---- exact sums of the survivors --------------------------------------------------------------------
// The reference's sum is sequential per circle, but finding the edge pixels on a perimeter and evaluating their
// gradient angles is not, and most survivors are dropped after a handful of terms (sum + remaining hits can no
// longer reach the threshold).  A workgroup takes XS survivors per round:
//   1. four lanes per survivor test its perimeter points against the edge bitmap -> a hit mask per survivor;
//   2. a lane per survivor turns the mask into the list of its hits, in perimeter order;
//   3. all lanes evaluate (survivor, hit) pairs: the next `ch` hits of every survivor that is still undecided --
//      angle on demand from the blurred image, term in float64 -- `ch` grows as the undecided get fewer;
//   4. a lane per survivor adds its terms in order with the early exit, and the undecided are listed again.
// XS survivors per workgroup and round: 64 at large batches; 16 at small ones, where the survivors of a plane would
// otherwise sit in ~150 workgroups whose phases are chains of latencies (NT / XS lanes per survivor in phase 1,
// more hits per step in phase 3).
constexpr int XCH_MAX = 32;  // hits per survivor evaluated per step, at most
constexpr int XPMAX = 2 * MAXP;

template <int XS>
__global__ __launch_bounds__(NT) void k_exact(const uint8_t* __restrict__ d_blur, const float* __restrict__ d_angle,
                                              const uint32_t* __restrict__ d_bits, int64_t words_per_plane, int h, int w,
                                              int32_t* __restrict__ d_circles, int64_t circle_cap, int ntc, int min_r,
                                              int max_r, const int32_t* __restrict__ d_per_rc, int per_total,
                                              const double* __restrict__ d_per_expected,
                                              const int32_t* __restrict__ d_per_starts, float min_roundness,
                                              int write_skipped, float* __restrict__ d_scores,
                                              int32_t* __restrict__ d_alive, int32_t* __restrict__ d_num_alive,
                                              int32_t* __restrict__ d_max_rc, int32_t* __restrict__ d_num_scored,
                                              const int32_t* __restrict__ d_surv, int64_t surv_cap,
                                              const int32_t* __restrict__ d_num_surv) {
  extern __shared__ __attribute__((aligned(16))) int32_t tab[];  // [per_total] (dr << 16) | (dc & 0xFFFF)
  __shared__ double s_term[XS][XCH_MAX];
  __shared__ uint32_t s_mask[XS][XPMAX / 32];
  __shared__ uint8_t s_hits[XS][XPMAX];
  __shared__ int s_row[XS], s_col[XS], s_p0[XS], s_p1[XS], s_nh[XS], s_base[XS], s_list[XS], s_n;
  __shared__ int32_t starts[34];
  const int plane = blockIdx.y;
  const int64_t n = min((int64_t)d_num_surv[plane], surv_cap);
  if ((int64_t)blockIdx.x * XS >= n) return;  // block-uniform
  for (int i = threadIdx.x; i < per_total; i += NT) tab[i] = (d_per_rc[2 * i] << 16) | (d_per_rc[2 * i + 1] & 0xFFFF);
  if ((int)threadIdx.x <= max_r - min_r + 1) starts[threadIdx.x] = d_per_starts[threadIdx.x];
  if (blockIdx.x == 0 && threadIdx.x == 0 && d_num_scored) d_num_scored[plane] = (int32_t)n;
  int32_t* circles = d_circles + (int64_t)plane * circle_cap * 3;
  const uint32_t* bits = d_bits + plane * words_per_plane;
  const uint8_t* blur = d_blur + (int64_t)plane * h * w;
  const float* ang = d_angle ? d_angle + (int64_t)plane * h * w : nullptr;
  float* scores = d_scores + (int64_t)plane * circle_cap;
  const int t = threadIdx.x;
  const int64_t rounds = (n + (int64_t)gridDim.x * XS - 1) / ((int64_t)gridDim.x * XS);
  for (int64_t rd = 0; rd < rounds; ++rd) {
    __syncthreads();  // tables in place / the previous round's lists are no longer read
    // 0. the round's survivors (threads 0..63 = wave 0 own one each)
    int64_t ci = 0;      // index in the plane's key list
    int rad = 0;
    bool active = false, dead = true;
    double acc = 0.0, floor_sum = 0.0;
    int left = 0;
    if (t < XS) {
      const int64_t k = (rd * gridDim.x + blockIdx.x) * XS + t;
      active = k < n;
      // record = (index in the plane's key list, key): written by the prefilter, no dependent load here
      const int2 rec = active ? reinterpret_cast<const int2*>(d_surv)[(int64_t)plane * surv_cap + k] : make_int2(0, 0);
      ci = rec.x;
      const uint32_t key = (uint32_t)rec.y;
      const int tile = (int)mg_key_tile(key);
      rad = min_r + mg_key_layer(key);
      s_row[t] = (tile / ntc) * TS - max_r + mg_key_row(key);
      s_col[t] = (tile % ntc) * TS - max_r + mg_key_col(key);
      s_p0[t] = starts[rad - min_r];
      s_p1[t] = active ? starts[rad - min_r + 1] : s_p0[t];
      floor_sum = mg_score_floor(min_roundness, s_p1[t] - s_p0[t]);
    }
    for (int i = t; i < XS * (XPMAX / 32); i += NT) (&s_mask[0][0])[i] = 0u;
    __syncthreads();
    // 1. hit masks: NT / XS lanes per survivor, four loads in flight per lane
    {
      constexpr int LPS = NT / XS;
      const int s = t / LPS, j0 = t % LPS;
      const int row = s_row[s], col = s_col[s], p0 = s_p0[s], len = s_p1[s] - p0;
      for (int j = j0; j < len; j += 4 * LPS) {
        uint32_t wv[4];
        int bi[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
          const int jj = j + LPS * u;
          const int v = tab[p0 + min(jj, len - 1)];
          const int y = row + (v >> 16), x = col + (int)(int16_t)(v & 0xFFFF);
          const bool inb = jj < len && y >= 0 && y < h && x >= 0 && x < w;
          bi[u] = inb ? y * w + x : -1;
          wv[u] = bits[max(bi[u], 0) >> 5];
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) {
          const int jj = j + LPS * u;
          if (bi[u] >= 0 && ((wv[u] >> (bi[u] & 31)) & 1u)) atomicOr(&s_mask[s][jj >> 5], 1u << (jj & 31));
        }
      }
    }
    __syncthreads();
    // 2. hit lists in perimeter order; the undecided survivors
    if (t < XS) {
      int nh = 0;
#pragma unroll
      for (int wd = 0; wd < XPMAX / 32; ++wd) {
        uint32_t m = s_mask[t][wd];
        while (m) {
          s_hits[t][nh++] = (uint8_t)(32 * wd + __ffs(m) - 1);
          m &= m - 1;
        }
      }
      s_nh[t] = nh;
      s_base[t] = 0;
      left = nh;  // edge pixels not yet summed: each adds at most 1 (+1.2e-7, inside the margin)
      dead = !active || (double)left < floor_sum;
      const bool open = !dead && nh > 0;
      const uint64_t om = __ballot(open);
      if (open) s_list[__builtin_amdgcn_mbcnt_hi((uint32_t)(om >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)om, 0u))] = t;
      if (t == 0) s_n = __builtin_popcountll(om);
    }
    __syncthreads();
    // 3. + 4. until every survivor of the round is decided
    for (int na = s_n; na > 0; na = s_n) {
      const int ch = min(XCH_MAX, max(8, (2 * NT / na) & ~7));
      for (int pair = t; pair < na * ch; pair += NT) {
        const int s = s_list[pair / ch], j = pair % ch;
        const int idx = s_base[s] + j;
        if (idx < s_nh[s]) {
          const int p = s_p0[s] + s_hits[s][idx];
          const int v = tab[p];
          const int y = s_row[s] + (v >> 16), x = s_col[s] + (int)(int16_t)(v & 0xFFFF);
          const float a = ang ? ang[(int64_t)y * w + x] : mg_edge_angle(blur, h, w, y, x);
          s_term[s][j] = mg_alignment_term(a, d_per_expected[p]);
        }
      }
      __syncthreads();
      if (t < XS) {
        bool open = false;
        if (!dead && s_base[t] < s_nh[t]) {
          const int cnt = min(ch, s_nh[t] - s_base[t]);
          for (int j = 0; j < cnt && !dead; ++j) {
            acc += s_term[t][j];
            --left;
            if (acc + (double)left < floor_sum) dead = true;  // exact: the remaining hits add <= 1 each
          }
          s_base[t] += cnt;
          open = !dead && s_base[t] < s_nh[t];
        }
        const uint64_t om = __ballot(open);
        if (open) s_list[__builtin_amdgcn_mbcnt_hi((uint32_t)(om >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)om, 0u))] = t;
        if (t == 0) s_n = __builtin_popcountll(om);
      }
      __syncthreads();
    }
    // 5. results
    if (t < XS && active) {
      if (dead) {
        if (write_skipped) scores[ci] = MG_SCORE_SKIPPED;
      } else {
        const float score = (float)acc / (float)(s_p1[t] - s_p0[t]);
        scores[ci] = score;
        if (score >= min_roundness)
          mg_emit_alive<true>(d_num_alive, d_alive, d_max_rc, plane, circle_cap, circles, ci, s_row[t], s_col[t], rad);
      }
    }
  }
}

}  // namespace

extern "C" int mg_score_walk_reads(int r) {
  switch (r) {
#define MG_CASE(R) case R: return 2 * Walk<R>{}.n;
    MG_CASE(2) MG_CASE(3) MG_CASE(4) MG_CASE(5) MG_CASE(6) MG_CASE(7) MG_CASE(8) MG_CASE(9) MG_CASE(10)
    MG_CASE(11) MG_CASE(12) MG_CASE(13) MG_CASE(14) MG_CASE(15) MG_CASE(16) MG_CASE(17) MG_CASE(18)
    MG_CASE(19) MG_CASE(20) MG_CASE(21) MG_CASE(22) MG_CASE(23) MG_CASE(24) MG_CASE(25) MG_CASE(26)
#undef MG_CASE
    default: return 0;
  }
}

extern "C" int mg_score_keyed_supported(int min_r, int max_r) {
  return (min_r >= 2 && max_r >= min_r && max_r <= MG_SCORE_MAX_R && max_r - min_r + 1 <= 32) ? 1 : 0;
}

extern "C" int mg_score_circles_keyed(const uint8_t* d_blur, const float* d_angle, const uint32_t* d_edge_bits,
                                      const uint32_t* d_class_bits, int64_t words_per_plane, int n_planes, int h, int w,
                                      int32_t* d_circles, int64_t circle_cap, const uint32_t* d_unique_keys,
                                      const int32_t* d_layer_starts, int min_r, int max_r, const int32_t* d_per_rc,
                                      const double* d_per_expected, const int32_t* d_per_starts, int per_total,
                                      const uint64_t* d_pair_table, float min_roundness, int write_skipped,
                                      float* d_scores, int32_t* d_alive, int32_t* d_num_alive, int32_t* d_max_rc,
                                      int32_t* d_num_scored, int32_t* d_surv_list, int64_t surv_cap, int32_t* d_num_surv,
                                      int counters_clear, void* stream) {
  if ((!d_blur && !d_angle) || !d_edge_bits || !d_class_bits || !d_circles || !d_unique_keys || !d_layer_starts ||
      !d_per_rc || !d_per_expected || !d_per_starts || !d_pair_table || !d_scores || !d_alive || !d_num_alive ||
      !d_max_rc || !d_surv_list || !d_num_surv)
    return MG_EINVAL;
  if (n_planes < 0 || n_planes > 65535 || per_total <= 0 || surv_cap < circle_cap) return MG_EINVAL;  // (a survivor per circle)
  if (mg_score_keyed_supported(min_r, max_r) != 1) return MG_EINVAL;
  if (h <= 0 || w <= 0 || h >= (1 << 24) || w >= (1 << 24) || (int64_t)h * w >= (1LL << 31)) return MG_EINVAL;
  int ntr, ntc, nr;
  if (mg_key_layout(h, w, min_r, max_r, &ntr, &ntc, &nr) != MG_OK) return MG_EINVAL;
  if ((size_t)per_total * 12 > 48 * 1024 || NSUB * (nr + 1) > NP) return MG_EINVAL;
  hipStream_t s = mg_stream(stream);
  if (!counters_clear && mg_zero_async(d_num_surv, (size_t)std::max(n_planes, 1) * sizeof(int32_t), s) != hipSuccess)
    return MG_ELAUNCH;
  if (n_planes == 0 || circle_cap == 0) return MG_OK;
  const size_t lds_bytes = (size_t)WBASE + (size_t)(STY + 2 * max_r) * WSTR;
  const int nsr = (ntr + SUBY - 1) / SUBY, nsc = (ntc + SUBX - 1) / SUBX, n_st = nsr * nsc;
  const int64_t total_st = (int64_t)n_st * n_planes;
  static bool attr_set = false;
  if (!attr_set) {
    if (hipFuncSetAttribute(reinterpret_cast<const void*>(k_prefilter), hipFuncAttributeMaxDynamicSharedMemorySize,
                            (int)(WBASE + (STY + 2 * MAXR) * WSTR)) != hipSuccess)
      return MG_ELAUNCH;
    attr_set = true;
  }
  // persistent blocks, super-tiles dealt round-robin (neighbouring super-tiles run at the same time)
  const int blocks = (int)std::min<int64_t>(total_st, MG_SCORE_PREFILTER_WALK);
  hipLaunchKernelGGL(k_prefilter, dim3(blocks), dim3(NP), lds_bytes, s, d_edge_bits, d_class_bits, words_per_plane, h, w,
                     d_unique_keys, circle_cap, d_layer_starts, ntr * ntc, ntr, ntc, nsc, n_st, total_st, min_r, max_r, nr,
                     reinterpret_cast<const uint2*>(d_pair_table), d_per_starts, min_roundness, write_skipped, d_scores,
                     d_surv_list, surv_cap, d_num_surv);
  MG_CHECK_LAUNCH();
  // blocks per plane: enough to fill the chip at any batch size, few enough to amortise the table load
  const int xblocks = std::max(16, std::min(256, MG_SCORE_EXACT_WALK / std::max(n_planes, 1)));
  if (n_planes <= 4)
    hipLaunchKernelGGL(k_exact<16>, dim3(4 * xblocks, n_planes), dim3(NT), (size_t)per_total * 4, s, d_blur, d_angle,
                       d_edge_bits, words_per_plane, h, w, d_circles, circle_cap, ntc, min_r, max_r, d_per_rc, per_total,
                       d_per_expected, d_per_starts, min_roundness, write_skipped, d_scores, d_alive, d_num_alive, d_max_rc,
                       d_num_scored, d_surv_list, surv_cap, d_num_surv);
  else
    hipLaunchKernelGGL(k_exact<64>, dim3(xblocks, n_planes), dim3(NT), (size_t)per_total * 4, s, d_blur, d_angle,
                       d_edge_bits, words_per_plane, h, w, d_circles, circle_cap, ntc, min_r, max_r, d_per_rc, per_total,
                       d_per_expected, d_per_starts, min_roundness, write_skipped, d_scores, d_alive, d_num_alive, d_max_rc,
                       d_num_scored, d_surv_list, surv_cap, d_num_surv);
  MG_CHECK_LAUNCH();
  return MG_OK;
}
