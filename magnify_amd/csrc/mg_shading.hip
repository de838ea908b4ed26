// BaSiC shading model (Peng et al., Nat. Commun. 8:14836, 2017): the fit of a flat- and a dark-field from a stack of
// training tiles (inexact ALM, low-rank + sparse, DCT-domain smoothness) and its apply fused with the stitch crop.
// The contract is DESIGN.md §4 "shading"; tests/ref_shading.py is its float64 oracle.
//
// The fit works on a small stack D (N x W^2 float32, W <= 128).  One ALM iteration is a chain of dependent phases, each
// one plain launch on the caller's stream: mean over images -> DCT update (two W^3 products) -> IDCT (two more) ->
// E / Y update with per-image partial sums -> per-image coefficients and darkfield scalars (one workgroup) ->
// darkfield smoothing (one per-pixel kernel and four products) -> stop test.  A block of K iterations is enqueued at
// once; the stop test writes a device `done` word and every kernel returns at once when it is set, so the host reads
// one word per block.  Every reduction is a fixed-order tree or loop (no floating-point atomics): two fits of the same
// input give the same bits.
#include <math.h>

#include "mg_common.h"
#include "mg_shadeop.h"
#include "mg_stitch.h"

namespace {

constexpr int SH_THREADS = 256;
constexpr int SH_CHUNK = 1024;  // pixels of one image per workgroup of the E update (4 per lane)
constexpr int SH_PART = 8;      // doubles per (image, chunk) partial record
constexpr double SH_ENT1 = 1.0, SH_ENT2 = 10.0, SH_RHO = 1.5;

// scalar slots (double) and flag words (int32) of the workspace
enum {
  SC_MU, SC_MUBAR, SC_LF, SC_LD, SC_TOL, SC_NORMF, SC_BUP, SC_B1, SC_MEANF, SC_MEANA, SC_CBAR, SC_MEANA1, SC_RATIO,
  SC_WSCALE, SC_COUNT = 32
};
enum { FL_DONE, FL_ITER, FL_MAXIT, FL_SKIPDARK, FL_COUNT = 8 };

struct Ws {
  float *D, *E, *Y, *Wt;                                     // N x P
  double *What, *Fw, *Aoff, *M, *T, *colmean, *colmin;       // P
  double *C, *CT;                                            // W x W cosine table and its transpose
  double *coeff, *tot, *part, *partF, *gram, *sc;            // N; N x 8; N x nch x 8; nbp; N x N; SC_COUNT
  int* flags;
  int n, w, P, nch, nbp;
};

__host__ __device__ inline int64_t align256(int64_t b) { return (b + 255) & ~(int64_t)255; }

// Byte offsets of the workspace regions, in the order of MG_SHADING_* field ids (include/magnify_hip.h).
__host__ inline int64_t layout(int n, int w, int64_t* off) {
  const int64_t P = (int64_t)w * w, nch = (P + SH_CHUNK - 1) / SH_CHUNK, nbp = (P + SH_THREADS - 1) / SH_THREADS;
  const int64_t sizes[] = {
      4 * n * P, 4 * n * P, 4 * n * P, 4 * n * P,                 // D E Y weight
      8 * P, 8 * P, 8 * P, 8 * P, 8 * P, 8 * P, 8 * P,           // What Fw Aoff M T colmean colmin
      8 * P, 8 * P,                                               // C CT
      8 * (int64_t)n, 8 * SH_PART * (int64_t)n, 8 * SH_PART * n * nch, 8 * nbp, 8 * (int64_t)n * n,  // coeff tot part partF gram
      8 * SC_COUNT, 4 * FL_COUNT};
  int64_t o = 0;
  for (int i = 0; i < (int)(sizeof(sizes) / sizeof(sizes[0])); ++i) {
    if (off) off[i] = o;
    o += align256(sizes[i]);
  }
  return o;
}
constexpr int SH_FIELDS = 20;

__host__ inline Ws make_ws(void* base, int n, int w) {
  int64_t o[SH_FIELDS];
  layout(n, w, o);
  char* b = static_cast<char*>(base);
  Ws s;
  s.D = (float*)(b + o[0]), s.E = (float*)(b + o[1]), s.Y = (float*)(b + o[2]), s.Wt = (float*)(b + o[3]);
  s.What = (double*)(b + o[4]), s.Fw = (double*)(b + o[5]), s.Aoff = (double*)(b + o[6]), s.M = (double*)(b + o[7]);
  s.T = (double*)(b + o[8]), s.colmean = (double*)(b + o[9]), s.colmin = (double*)(b + o[10]);
  s.C = (double*)(b + o[11]), s.CT = (double*)(b + o[12]);
  s.coeff = (double*)(b + o[13]), s.tot = (double*)(b + o[14]), s.part = (double*)(b + o[15]);
  s.partF = (double*)(b + o[16]), s.gram = (double*)(b + o[17]), s.sc = (double*)(b + o[18]);
  s.flags = (int*)(b + o[19]);
  s.n = n, s.w = w, s.P = w * w;
  s.nch = (s.P + SH_CHUNK - 1) / SH_CHUNK, s.nbp = (s.P + SH_THREADS - 1) / SH_THREADS;
  return s;
}

__device__ __forceinline__ double shrink(double x, double t) { return x > t ? x - t : (x < -t ? x + t : 0.0); }

// Fixed-order tree sum of NV values over the 256 lanes of a workgroup; the result is valid in lane 0.
template <int NV>
__device__ __forceinline__ void block_sum(double (&v)[NV]) {
  __shared__ double s[NV][SH_THREADS];
  const int t = threadIdx.x;
#pragma unroll
  for (int k = 0; k < NV; ++k) s[k][t] = v[k];
  __syncthreads();
  for (int stride = SH_THREADS / 2; stride > 0; stride >>= 1) {
    if (t < stride) {
#pragma unroll
      for (int k = 0; k < NV; ++k) s[k][t] += s[k][t + stride];
    }
    __syncthreads();
  }
#pragma unroll
  for (int k = 0; k < NV; ++k) v[k] = s[k][0];
}

// ---- area downsample: working pixel (i, j) of image n is the mean over [i*ty/w, (i+1)*ty/w) x [j*tx/w, (j+1)*tx/w),
// edge source pixels weighted by the covered fraction.  Integer overlaps in units of 1/w, so the weights are exact.
template <typename T>
__global__ __launch_bounds__(256) void k_downsample(const T* __restrict__ tiles, int ty, int tx, int w,
                                                    float* __restrict__ out) {
  const int p = blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= w * w) return;
  const int n = blockIdx.y;
  const int i = p / w, j = p - i * w;
  const int64_t ay = (int64_t)i * ty, by = (int64_t)(i + 1) * ty, ax = (int64_t)j * tx, bx = (int64_t)(j + 1) * tx;
  const int s0 = (int)(ay / w), s1 = (int)min<int64_t>((by + w - 1) / w, ty);
  const int c0 = (int)(ax / w), c1 = (int)min<int64_t>((bx + w - 1) / w, tx);
  const T* img = tiles + (int64_t)n * ty * tx;
  double acc = 0.0;
  for (int s = s0; s < s1; ++s) {
    const double wy = (double)(min(by, (int64_t)(s + 1) * w) - max(ay, (int64_t)s * w));
    double row = 0.0;
    const T* src = img + (int64_t)s * tx;
    for (int c = c0; c < c1; ++c) {
      const double wx = (double)(min(bx, (int64_t)(c + 1) * w) - max(ax, (int64_t)c * w));
      row += wx * (double)src[c];
    }
    acc += wy * row;
  }
  out[(int64_t)n * w * w + p] = (float)(acc / ((double)ty * (double)tx));
}

// ---- setup: orthonormal DCT-II table, per-pixel mean / min over images, Gram matrix, weight = 1
__global__ __launch_bounds__(256) void k_setup(Ws s) {
  const int64_t NP = (int64_t)s.n * s.P;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < NP; i += (int64_t)gridDim.x * blockDim.x) {
    s.Wt[i] = 1.0f;
    if (i < s.P) {
      const int k = (int)(i / s.w), x = (int)(i - (int64_t)k * s.w);
      const double a = k == 0 ? sqrt(1.0 / s.w) : sqrt(2.0 / s.w);
      const double v = a * cos(M_PI * (double)((2 * x + 1) * k) / (2.0 * s.w));
      s.C[(int64_t)k * s.w + x] = v;
      s.CT[(int64_t)x * s.w + k] = v;
      double sum = 0.0, mn = INFINITY;
      for (int n = 0; n < s.n; ++n) {
        const double d = s.D[(int64_t)n * s.P + i];
        sum += d;
        mn = d < mn ? d : mn;
      }
      s.colmean[i] = sum / s.n;
      s.colmin[i] = mn;
    }
  }
}

__global__ __launch_bounds__(256) void k_gram(Ws s) {
  const int a = blockIdx.x, b = blockIdx.y;
  if (b < a) return;
  const float* da = s.D + (int64_t)a * s.P;
  const float* db = s.D + (int64_t)b * s.P;
  double v[1] = {0.0};
  for (int p = threadIdx.x; p < s.P; p += SH_THREADS) v[0] += (double)da[p] * (double)db[p];
  block_sum<1>(v);
  if (threadIdx.x == 0) {
    s.gram[(int64_t)a * s.n + b] = v[0];
    s.gram[(int64_t)b * s.n + a] = v[0];
  }
}

// ---- ALM state of a fresh pass
__global__ __launch_bounds__(256) void k_begin(Ws s, int get_dark, int max_iter, double mu, double lam_f, double lam_d,
                                               double tol, double norm_f, double b_up) {
  const int64_t NP = (int64_t)s.n * s.P;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < NP; i += (int64_t)gridDim.x * blockDim.x) {
    s.E[i] = 0.0f;
    s.Y[i] = 0.0f;
    if (i < s.P) s.What[i] = 0.0, s.Fw[i] = 0.0, s.Aoff[i] = 0.0;
    if (i < s.n) s.coeff[i] = 1.0;
    if (i < s.nbp) s.partF[i] = 0.0;
    if (i == 0) {
      for (int k = 0; k < SC_COUNT; ++k) s.sc[k] = 0.0;
      s.sc[SC_MU] = mu;
      s.sc[SC_MUBAR] = 1e7 * mu;
      s.sc[SC_LF] = lam_f;
      s.sc[SC_LD] = lam_d;
      s.sc[SC_TOL] = tol;
      s.sc[SC_NORMF] = norm_f;
      s.sc[SC_BUP] = b_up;
      s.flags[FL_DONE] = 0;
      s.flags[FL_ITER] = 0;
      s.flags[FL_MAXIT] = max_iter;
      s.flags[FL_SKIPDARK] = get_dark ? 0 : 1;
    }
  }
}

// M[p] = mean_n(D - A - E + Y / mu) / ent1 with A = Fw[p] coeff[n] + Aoff[p]
__global__ __launch_bounds__(256) void k_resid_mean(Ws s) {
  if (s.flags[FL_DONE]) return;
  const int p = blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= s.P) return;
  const double mu = s.sc[SC_MU], fw = s.Fw[p], ao = s.Aoff[p];
  double acc = 0.0;
  for (int n = 0; n < s.n; ++n) {
    const int64_t idx = (int64_t)n * s.P + p;
    const double a = fw * s.coeff[n] + ao;
    acc += (((double)s.D[idx] - a) - (double)s.E[idx]) + (double)s.Y[idx] / mu;
  }
  s.M[p] = acc / s.n / SH_ENT1;
}

enum { MM_PLAIN, MM_WHAT, MM_FW, MM_DARK_SHRINK, MM_AOFF };
enum { GATE_NONE, GATE_DONE, GATE_DARK };

// out = L . R (W x W, row-major), thread = one output element, float64 accumulation in fixed order; the epilogue of
// `mode` folds in the step that consumes the product.
__global__ __launch_bounds__(256) void k_mm(Ws s, const double* __restrict__ L, const double* __restrict__ R,
                                            double* __restrict__ out, int mode, int gate) {
  if (gate != GATE_NONE && s.flags[FL_DONE]) return;
  if (gate == GATE_DARK && s.flags[FL_SKIPDARK]) return;
  const int w = s.w;
  const int p = blockIdx.x * blockDim.x + threadIdx.x;
  double v[1] = {0.0};
  if (p < s.P) {
    const int i = p / w, j = p - i * w;
    const double* l = L + (int64_t)i * w;
    double acc = 0.0;
    // (unrolled: 16 loads in flight instead of one dependent L2 round trip per term; the sum order is unchanged)
#pragma unroll 16
    for (int k = 0; k < w; ++k) acc = fma(l[k], R[(int64_t)k * w + j], acc);
    const double mu = s.sc[SC_MU];
    if (mode == MM_WHAT) {
      acc = shrink(out[p] + acc, s.sc[SC_LF] / (SH_ENT1 * mu));  // (M already holds the mean / ent1)
    } else if (mode == MM_DARK_SHRINK) {
      acc = shrink(acc, s.sc[SC_LD] / (SH_ENT2 * mu));
    } else if (mode == MM_AOFF) {
      const double b1 = s.sc[SC_B1], fw = s.Fw[p];
      acc = shrink(acc, s.sc[SC_LD] / (SH_ENT2 * mu)) + (b1 * s.sc[SC_MEANF] - b1 * fw);
    }
    out[p] = acc;
    v[0] = acc;
  }
  if (mode == MM_FW) {
    block_sum<1>(v);
    if (threadIdx.x == 0) s.partF[blockIdx.x] = v[0];
  }
}

__device__ __forceinline__ double sum_partF(const Ws& s) {
  double m = 0.0;
  for (int b = 0; b < s.nbp; ++b) m += s.partF[b];
  return m;
}

// E update, residual R = D - E, Z = D - A - E, Y += mu Z, with per-(image, chunk) partial sums of R (all / hi / lo
// pixels), A and Z^2.  Workgroup = (chunk, image).
__global__ __launch_bounds__(256) void k_update(Ws s) {
  if (s.flags[FL_DONE]) return;
  const int chunk = blockIdx.x, n = blockIdx.y;
  const double meanF = sum_partF(s) / s.P;
  const double mu = s.sc[SC_MU], cn = s.coeff[n];
  double v[7] = {0, 0, 0, 0, 0, 0, 0};  // R, R hi, R lo, A, Z^2, count hi, count lo
  const int p1 = min((chunk + 1) * SH_CHUNK, s.P);
  for (int p = chunk * SH_CHUNK + threadIdx.x; p < p1; p += SH_THREADS) {
    const int64_t idx = (int64_t)n * s.P + p;
    const double fw = s.Fw[p];
    const double a = fw * cn + s.Aoff[p];
    const double d = s.D[idx], e = s.E[idx], y = s.Y[idx];
    double en = e + ((((d - a) - e) + y / mu) / SH_ENT1);
    en = shrink(en, (double)s.Wt[idx] / (SH_ENT1 * mu));
    const float ef = (float)en;
    s.E[idx] = ef;
    const double r = d - (double)ef;
    const double z = (d - a) - (double)ef;
    s.Y[idx] = (float)(y + mu * z);
    const bool hi = fw > meanF - 1e-6, lo = fw < meanF + 1e-6;
    v[0] += r;
    v[1] += hi ? r : 0.0;
    v[2] += lo ? r : 0.0;
    v[3] += a;
    v[4] += z * z;
    v[5] += hi ? 1.0 : 0.0;
    v[6] += lo ? 1.0 : 0.0;
  }
  block_sum<7>(v);
  if (threadIdx.x == 0) {
    double* o = s.part + ((int64_t)n * s.nch + chunk) * SH_PART;
    for (int k = 0; k < 7; ++k) o[k] = v[k];
  }
}

// One workgroup: per-image totals, coeff, mean(A), the stop ratio and the darkfield scalars.
__global__ __launch_bounds__(256) void k_coeff(Ws s, int get_dark) {
  if (s.flags[FL_DONE]) return;
  __shared__ double sh_meanA, sh_meanF;
  const int P = s.P;
  for (int n = threadIdx.x; n < s.n; n += SH_THREADS) {
    double t[7] = {0, 0, 0, 0, 0, 0, 0};
    for (int c = 0; c < s.nch; ++c) {
      const double* o = s.part + ((int64_t)n * s.nch + c) * SH_PART;
      for (int k = 0; k < 7; ++k) t[k] += o[k];
    }
    for (int k = 0; k < 7; ++k) s.tot[(int64_t)n * SH_PART + k] = t[k];
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    double sa = 0.0, sz = 0.0;
    for (int n = 0; n < s.n; ++n) sa += s.tot[(int64_t)n * SH_PART + 3], sz += s.tot[(int64_t)n * SH_PART + 4];
    sh_meanA = sa / ((double)s.n * P);
    sh_meanF = sum_partF(s) / P;
    s.sc[SC_MEANA] = sh_meanA;
    s.sc[SC_MEANF] = sh_meanF;
    s.sc[SC_RATIO] = sqrt(sz) / s.sc[SC_NORMF];
  }
  __syncthreads();
  const double meanA = sh_meanA, meanF = sh_meanF;
  for (int n = threadIdx.x; n < s.n; n += SH_THREADS) {
    double* t = s.tot + (int64_t)n * SH_PART;
    const double c = t[0] / P / meanA;
    s.coeff[n] = c > 0.0 ? c : 0.0;
    t[7] = (t[1] / t[5] - t[2] / t[6]) / meanA;  // B1c (the hi / lo counts are those of every image)
  }
  __syncthreads();
  if (threadIdx.x == 0 && get_dark) {
    int k = 0;
    double t1 = 0, t2 = 0, t3 = 0, t4 = 0, sr = 0;
    for (int n = 0; n < s.n; ++n) {
      const double c = s.coeff[n];
      if (!(c < 1.0)) continue;
      const double b1c = s.tot[(int64_t)n * SH_PART + 7];
      ++k;
      t1 += c * c, t2 += c, t3 += b1c, t4 += c * b1c;
      sr += s.tot[(int64_t)n * SH_PART + 0] / P;
    }
    s.flags[FL_SKIPDARK] = k == 0;  // no image below the mean brightness: the darkfield step is skipped
    if (k > 0) {
      const double t5 = t2 * t3 - k * t4;
      double b1 = t5 == 0.0 ? 0.0 : (t1 * t3 - t2 * t4) / t5;
      b1 = b1 > 0.0 ? b1 : 0.0;
      const double cap = s.sc[SC_BUP] / meanF;
      b1 = b1 < cap ? b1 : cap;
      s.sc[SC_B1] = b1;
      s.sc[SC_CBAR] = t2 / k;
      s.sc[SC_MEANA1] = sr / k - (t2 / k) * meanF;
    }
  }
}

// X = A1 - mean(A1) - B_off with A1 = mean_{n in V}(D - E) - cbar Fw (mean(A1) from the per-image totals)
__global__ __launch_bounds__(256) void k_dark_a1(Ws s) {
  if (s.flags[FL_DONE] || s.flags[FL_SKIPDARK]) return;
  const int p = blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= s.P) return;
  double acc = 0.0;
  int k = 0;
  for (int n = 0; n < s.n; ++n) {
    if (!(s.coeff[n] < 1.0)) continue;
    const int64_t idx = (int64_t)n * s.P + p;
    acc += (double)s.D[idx] - (double)s.E[idx];
    ++k;
  }
  const double fw = s.Fw[p], b1 = s.sc[SC_B1];
  const double a1 = acc / k - s.sc[SC_CBAR] * fw;
  s.M[p] = (a1 - s.sc[SC_MEANA1]) - (b1 * s.sc[SC_MEANF] - b1 * fw);
}

// Stop test and mu update; the only writer of `done`.
__global__ void k_finish(Ws s) {
  if (threadIdx.x != 0 || s.flags[FL_DONE]) return;
  const int it = s.flags[FL_ITER] + 1;
  s.flags[FL_ITER] = it;
  const double mu = SH_RHO * s.sc[SC_MU];
  s.sc[SC_MU] = mu < s.sc[SC_MUBAR] ? mu : s.sc[SC_MUBAR];
  if (s.sc[SC_RATIO] < s.sc[SC_TOL] || it >= s.flags[FL_MAXIT]) s.flags[FL_DONE] = 1;
}

// ---- reweighting: weight = 1 / (|E / mXA| + eps), scaled to mean 1 (mXA = mean_n XA, in M)
__global__ __launch_bounds__(256) void k_weight(Ws s, double eps, int write) {
  const int chunk = blockIdx.x, n = blockIdx.y;
  const double scale = write ? s.sc[SC_WSCALE] : 1.0;
  double v[1] = {0.0};
  const int p1 = min((chunk + 1) * SH_CHUNK, s.P);
  for (int p = chunk * SH_CHUNK + threadIdx.x; p < p1; p += SH_THREADS) {
    const int64_t idx = (int64_t)n * s.P + p;
    const double wv = 1.0 / (fabs((double)s.E[idx] / s.M[p]) + eps);
    if (write) s.Wt[idx] = (float)(wv * scale);
    v[0] += wv;
  }
  if (write) return;
  block_sum<1>(v);
  if (threadIdx.x == 0) s.part[((int64_t)n * s.nch + chunk) * SH_PART] = v[0];
}

__global__ void k_weight_scale(Ws s) {
  if (threadIdx.x != 0) return;
  double sum = 0.0;
  for (int64_t i = 0; i < (int64_t)s.n * s.nch; ++i) sum += s.part[i * SH_PART];
  s.sc[SC_WSCALE] = ((double)s.n * s.P) / sum;
}

// ---- bilinear upsample (half-pixel centres, clamped) of the working fields to ty x tx
__device__ __forceinline__ void lin_coord(int i, double scale, int src, int& i0, int& i1, double& f) {
  const double sp = (i + 0.5) * scale - 0.5;
  i0 = (int)floor(sp);
  f = sp - i0;
  if (i0 < 0) i0 = 0, f = 0.0;
  if (i0 >= src - 1) i0 = src - 1, f = 0.0;
  i1 = min(i0 + 1, src - 1);
}
__device__ __forceinline__ double lin_at(const double* __restrict__ a, int w, int y, int x, double sy, double sx) {
  int y0, y1, x0, x1;
  double fy, fx;
  lin_coord(y, sy, w, y0, y1, fy);
  lin_coord(x, sx, w, x0, x1, fx);
  const double r0 = (1.0 - fx) * a[y0 * w + x0] + fx * a[y0 * w + x1];
  const double r1 = (1.0 - fx) * a[y1 * w + x0] + fx * a[y1 * w + x1];
  return (1.0 - fy) * r0 + fy * r1;
}

constexpr int SH_UP_BLOCKS = 256;
__global__ __launch_bounds__(256) void k_upsample(const double* __restrict__ flat_w, const double* __restrict__ dark_w,
                                                  int w, int ty, int tx, double* __restrict__ partial,
                                                  float* __restrict__ flat, float* __restrict__ dark, int write) {
  const double sy = (double)w / ty, sx = (double)w / tx;
  double v[1] = {0.0};
  double mean = 1.0;
  if (write) {
    v[0] = partial[threadIdx.x];
    block_sum<1>(v);
    mean = v[0] / ((double)ty * tx);
  }
  double acc[1] = {0.0};
  const int64_t total = (int64_t)ty * tx;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
    const int y = (int)(i / tx), x = (int)(i - (int64_t)y * tx);
    const double f = lin_at(flat_w, w, y, x, sy, sx);
    if (write) {
      flat[i] = (float)(f / mean);
      dark[i] = (float)lin_at(dark_w, w, y, x, sy, sx);
    } else {
      acc[0] += f;
    }
  }
  if (write) return;
  block_sum<1>(acc);
  if (threadIdx.x == 0) partial[blockIdx.x] = acc[0];
}

// ---- apply fused with the stitch crop: v = (x - dark) / flat, IEEE operations, integer outputs clamped to
// [0, max] and truncated; per-plane min / max of the values written.
constexpr int SH_APPLY_VEC = 4;

template <typename T>
__global__ __launch_bounds__(256) void k_shading_apply(const T* __restrict__ tiles, int64_t planes_per_field, int n_tr,
                                                       int n_tc, int ty, int tx, int clip, int hy, int hx,
                                                       const float* __restrict__ flat, const float* __restrict__ dark,
                                                       T* __restrict__ image, double* __restrict__ d_minmax,
                                                       int rows_per_block) {
  const int64_t plane = blockIdx.z;
  const int64_t field = plane / planes_per_field;
  const int64_t tile_elems = (int64_t)ty * tx;
  const float* fl = flat + field * tile_elems;
  const float* dk = dark + field * tile_elems;
  const T* src = tiles + plane * n_tr * n_tc * tile_elems;
  const int h_out = n_tr * hy, w_out = n_tc * hx;
  T* dst_plane = image + plane * h_out * w_out;
  const int ox0 = (blockIdx.x * blockDim.x + threadIdx.x) * SH_APPLY_VEC;
  PlaneMinMax<T, 1> mm;
  int64_t col_off[SH_APPLY_VEC];  // tile column offset + x inside the tile, per lane pixel
  int xin[SH_APPLY_VEC];          // x inside the tile
  int cnt = 0;
#pragma unroll
  for (int j = 0; j < SH_APPLY_VEC; ++j) {
    const int ox = ox0 + j;
    if (ox < w_out) {
      const int tc = ox / hx;
      xin[j] = ox - tc * hx + clip;
      col_off[j] = (int64_t)tc * tile_elems + xin[j];
      ++cnt;
    } else {
      col_off[j] = 0, xin[j] = 0;
    }
  }
  if (cnt > 0)
    for (int yg = blockIdx.y; yg * rows_per_block < h_out; yg += gridDim.y) {
      const int row_end = min((yg + 1) * rows_per_block, h_out);
      for (int oy = yg * rows_per_block; oy < row_end; ++oy) {
        const int tr = oy / hy;
        const int y = oy - tr * hy + clip;
        const int64_t row_src = (int64_t)tr * n_tc * tile_elems + (int64_t)y * tx;
        const int64_t row_fld = (int64_t)y * tx;
        T o[SH_APPLY_VEC];
#pragma unroll
        for (int j = 0; j < SH_APPLY_VEC; ++j) {
          if (j >= cnt) break;
          o[j] = ShadeOp<T>::apply(src[row_src + col_off[j]], dk[row_fld + xin[j]], fl[row_fld + xin[j]]);
          if (d_minmax) mm.add(0, o[j]);
        }
        T* dst = dst_plane + (int64_t)oy * w_out + ox0;
        for (int j = 0; j < cnt; ++j) dst[j] = o[j];
      }
    }
  if (!d_minmax) return;
  mm.flush(1, d_minmax, plane);
}

template <typename T>
int launch_shading_apply(const void* d_tiles, int64_t n_planes, int64_t ppf, int n_tr, int n_tc, int ty, int tx,
                         int overlap, const float* d_flat, const float* d_dark, void* d_image, double* d_minmax,
                         hipStream_t s) {
  const auto [clip, hy, hx, h_out, w_out] = mg_stitch_geom(ty, tx, overlap, n_tr, n_tc);
  if (n_planes == 0) return MG_OK;
  const int gx = (w_out + 256 * SH_APPLY_VEC - 1) / (256 * SH_APPLY_VEC);
  const int rows = 8;
  const int64_t groups = (h_out + rows - 1) / rows;
  // about 8 workgroups per CU over the whole launch; each takes row groups blockIdx.y, +gridDim.y, ...
  const int64_t want = std::max<int64_t>(1, MG_SHADING_APPLY_WALK / std::max<int64_t>(1, gx * n_planes));
  const int gy = (int)std::min<int64_t>(groups, std::min<int64_t>(want, MG_WALK_MAX_Y));
  hipLaunchKernelGGL((k_shading_apply<T>), dim3(gx, gy, (unsigned)n_planes), dim3(256), 0, s, (const T*)d_tiles, ppf,
                     n_tr, n_tc, ty, tx, clip, hy, hx, d_flat, d_dark, (T*)d_image, d_minmax, rows);
  MG_CHECK_LAUNCH();
  return MG_OK;
}

inline bool shape_ok(int n, int w) { return n >= 1 && w >= 1 && w <= 128; }

}  // namespace

extern "C" int64_t mg_shading_workspace_bytes(int n, int w) {
  if (!shape_ok(n, w)) return -1;
  return layout(n, w, nullptr);
}

extern "C" int64_t mg_shading_offset(int n, int w, int field) {
  if (!shape_ok(n, w) || field < 0 || field >= SH_FIELDS) return -1;
  int64_t o[SH_FIELDS];
  layout(n, w, o);
  return o[field];
}

extern "C" int mg_shading_downsample(const void* d_tiles, int dtype, int64_t n, int ty, int tx, int w, float* d_out,
                                     void* stream) {
  if (!d_tiles || !d_out || n < 1 || n > 65535 || w < 1 || w > 128 || ty < w || tx < w) return MG_EINVAL;
  hipStream_t s = mg_stream(stream);
  const dim3 grid((unsigned)((w * w + 255) / 256), (unsigned)n);
  return mg_dispatch_pixel(dtype, [&](auto t) {
    using T = decltype(t);
    hipLaunchKernelGGL((k_downsample<T>), grid, dim3(256), 0, s, (const T*)d_tiles, ty, tx, w, d_out);
    MG_CHECK_LAUNCH();
    return MG_OK;
  });
}

extern "C" int mg_shading_prepare(void* d_ws, int n, int w, void* stream) {
  if (!d_ws || !shape_ok(n, w) || n > 65535) return MG_EINVAL;
  const Ws ws = make_ws(d_ws, n, w);
  hipStream_t s = mg_stream(stream);
  hipLaunchKernelGGL(k_setup, dim3(MG_SHADING_SETUP_WALK), dim3(256), 0, s, ws);
  hipLaunchKernelGGL(k_gram, dim3((unsigned)n, (unsigned)n), dim3(256), 0, s, ws);
  MG_CHECK_LAUNCH();
  return MG_OK;
}

extern "C" int mg_shading_dct2(void* d_ws, int n, int w, const double* d_in, double* d_out, int inverse, void* stream) {
  if (!d_ws || !d_in || !d_out || !shape_ok(n, w)) return MG_EINVAL;
  const Ws ws = make_ws(d_ws, n, w);
  hipStream_t s = mg_stream(stream);
  const dim3 g((unsigned)ws.nbp);
  // dct2(X) = C X C^T, idct2(X) = C^T X C
  hipLaunchKernelGGL(k_mm, g, dim3(256), 0, s, ws, inverse ? ws.CT : ws.C, d_in, ws.T, (int)MM_PLAIN, (int)GATE_NONE);
  hipLaunchKernelGGL(k_mm, g, dim3(256), 0, s, ws, ws.T, inverse ? ws.C : ws.CT, d_out, (int)MM_PLAIN, (int)GATE_NONE);
  MG_CHECK_LAUNCH();
  return MG_OK;
}

extern "C" int mg_shading_alm_begin(void* d_ws, int n, int w, int get_darkfield, int max_iterations, double mu,
                                    double lam_f, double lam_d, double tol, double norm_f, double b_up, void* stream) {
  if (!d_ws || !shape_ok(n, w) || max_iterations < 1) return MG_EINVAL;
  const Ws ws = make_ws(d_ws, n, w);
  hipStream_t s = mg_stream(stream);
  hipLaunchKernelGGL(k_begin, dim3(MG_SHADING_SETUP_WALK), dim3(256), 0, s, ws, get_darkfield, max_iterations, mu, lam_f, lam_d, tol,
                     norm_f, b_up);
  MG_CHECK_LAUNCH();
  return MG_OK;
}

extern "C" int mg_shading_alm_iterate(void* d_ws, int n, int w, int k, int get_darkfield, void* stream) {
  if (!d_ws || !shape_ok(n, w) || n > 65535 || k < 0) return MG_EINVAL;
  const Ws ws = make_ws(d_ws, n, w);
  hipStream_t s = mg_stream(stream);
  const dim3 gp((unsigned)ws.nbp), b(256), gu((unsigned)ws.nch, (unsigned)n);
  for (int it = 0; it < k; ++it) {
    hipLaunchKernelGGL(k_resid_mean, gp, b, 0, s, ws);
    hipLaunchKernelGGL(k_mm, gp, b, 0, s, ws, ws.C, ws.M, ws.T, (int)MM_PLAIN, (int)GATE_DONE);
    hipLaunchKernelGGL(k_mm, gp, b, 0, s, ws, ws.T, ws.CT, ws.What, (int)MM_WHAT, (int)GATE_DONE);
    hipLaunchKernelGGL(k_mm, gp, b, 0, s, ws, ws.CT, ws.What, ws.T, (int)MM_PLAIN, (int)GATE_DONE);
    hipLaunchKernelGGL(k_mm, gp, b, 0, s, ws, ws.T, ws.C, ws.Fw, (int)MM_FW, (int)GATE_DONE);
    hipLaunchKernelGGL(k_update, gu, b, 0, s, ws);
    hipLaunchKernelGGL(k_coeff, dim3(1), b, 0, s, ws, get_darkfield);
    if (get_darkfield) {
      hipLaunchKernelGGL(k_dark_a1, gp, b, 0, s, ws);
      hipLaunchKernelGGL(k_mm, gp, b, 0, s, ws, ws.C, ws.M, ws.T, (int)MM_PLAIN, (int)GATE_DARK);
      hipLaunchKernelGGL(k_mm, gp, b, 0, s, ws, ws.T, ws.CT, ws.M, (int)MM_DARK_SHRINK, (int)GATE_DARK);
      hipLaunchKernelGGL(k_mm, gp, b, 0, s, ws, ws.CT, ws.M, ws.T, (int)MM_PLAIN, (int)GATE_DARK);
      hipLaunchKernelGGL(k_mm, gp, b, 0, s, ws, ws.T, ws.C, ws.Aoff, (int)MM_AOFF, (int)GATE_DARK);
    }
    hipLaunchKernelGGL(k_finish, dim3(1), dim3(64), 0, s, ws);
  }
  MG_CHECK_LAUNCH();
  return MG_OK;
}

extern "C" int mg_shading_reweight(void* d_ws, int n, int w, double epsilon, void* stream) {
  if (!d_ws || !shape_ok(n, w) || n > 65535) return MG_EINVAL;
  const Ws ws = make_ws(d_ws, n, w);
  hipStream_t s = mg_stream(stream);
  const dim3 gu((unsigned)ws.nch, (unsigned)n);
  hipLaunchKernelGGL(k_weight, gu, dim3(256), 0, s, ws, epsilon, 0);
  hipLaunchKernelGGL(k_weight_scale, dim3(1), dim3(64), 0, s, ws);
  hipLaunchKernelGGL(k_weight, gu, dim3(256), 0, s, ws, epsilon, 1);
  MG_CHECK_LAUNCH();
  return MG_OK;
}

extern "C" int mg_shading_upsample(const double* d_flat_w, const double* d_dark_w, int w, int ty, int tx,
                                   double* d_partial, float* d_flat, float* d_dark, void* stream) {
  if (!d_flat_w || !d_dark_w || !d_partial || !d_flat || !d_dark || w < 1 || w > 128 || ty < 1 || tx < 1)
    return MG_EINVAL;
  hipStream_t s = mg_stream(stream);
  hipLaunchKernelGGL(k_upsample, dim3(SH_UP_BLOCKS), dim3(256), 0, s, d_flat_w, d_dark_w, w, ty, tx, d_partial, d_flat,
                     d_dark, 0);
  hipLaunchKernelGGL(k_upsample, dim3(SH_UP_BLOCKS), dim3(256), 0, s, d_flat_w, d_dark_w, w, ty, tx, d_partial, d_flat,
                     d_dark, 1);
  MG_CHECK_LAUNCH();
  return MG_OK;
}

extern "C" int mg_shading_apply_stitch(const void* d_tiles, int dtype, int n_fields, int64_t planes_per_field,
                                       int n_tile_rows, int n_tile_cols, int ty, int tx, int overlap,
                                       const float* d_flat, const float* d_dark, void* d_image, double* d_minmax,
                                       void* stream) {
  if (!d_tiles || !d_image || !d_flat || !d_dark || n_fields < 1 || planes_per_field < 0 || n_tile_rows <= 0 ||
      n_tile_cols <= 0 || ty <= 0 || tx <= 0)
    return MG_EINVAL;
  if (overlap < 0 || overlap >= ty || overlap >= tx) return MG_EINVAL;
  const int64_t n_planes = (int64_t)n_fields * planes_per_field;
  if (n_planes > 65535) return MG_EINVAL;
  hipStream_t s = mg_stream(stream);
  return mg_dispatch_pixel(dtype, [&](auto t) {
    return launch_shading_apply<decltype(t)>(d_tiles, n_planes, planes_per_field, n_tile_rows, n_tile_cols, ty, tx,
                                             overlap, d_flat, d_dark, d_image, d_minmax, s);
  });
}
