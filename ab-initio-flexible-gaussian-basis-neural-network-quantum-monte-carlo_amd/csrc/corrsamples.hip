// corrsamples.hip -- correlated sampling between nuclear geometries: the space-warp transform
// with its Jacobian (aiqmc_space_warp) and the reweighted energy-difference estimator as three
// reduction levels (aiqmc_corr_level, aiqmc_corr_final; context-free, as the loss levels).
//
// Warp of one electron r from the context's atoms R_a to R'_a = R_a + dR_a (Filippi-Umrigar; the
// reference's correlatedsamples/corrsamples.py:23-47 with the weights scaled so that nothing
// overflows):
//   d_a = r - R_a, r_a = |d_a|, r_min = min_a r_a, n = the first atom at r_min
//   q_a = (r_min / r_a)^4, w_a = q_a / sum_b q_b       (= r_a^-4 / sum_b r_b^-4)
//   r'  = r + dR_n + sum_a w_a (dR_a - dR_n)             (= r + sum_a w_a dR_a since sum_a w_a = 1:
//                                                         a rigid translation is reproduced exactly)
//   grad w_a = 4 w_a sum_{b != a} w_b (g_b - g_a),  g_a = d_a / r_a^2
//   J[k][l] = delta_kl + sum_a (dR_a - dR_n)[k] d_l w_a  (sum_a grad w_a = 0), det in closed form
//   r_min = 0: w_a = 1/k on the k atoms at zero distance, 0 elsewhere, grad w_a = 0
// logjac = sum_i log|det J_i|, electrons in ascending slot order.  Nothing is clamped: a singular
// J_i gives -inf.  dR is formed in double from new_atoms and the context's atoms, everything else
// in the context dtype.
//
// k_space_warp: one row of 16 lanes per (m, b), lane = electron slot (N <= 16, lanes >= N idle),
// four rows per wave, 16 per workgroup.  A row reads its walker's 3N coordinates once and writes
// the 3N warped ones contiguously; lane 0 of the row collects the N log-determinants by lane reads
// in ascending slot order.  A row depends on nothing but its own (m, b): the same bits for any B,
// M or chunking of either, and from run to run.  No workspace.
//
// Levels (one workgroup of 1024 per geometry m, every sum in double in a fixed tree order):
//   lw_b = 2 (logabs1[m][b] - logabs0[b]) + logjac[m][b]
//   1  out[m]       = max_b lw_b                                   (ranks combine with MAX)
//   2  out[m][0..4] = [n, sum e0, sum w, sum w e1, sum w^2],  w_b = exp(lw_b - L1[m])      (SUM)
//   3  out[m][0..1] = [sum d, sum d^2],  d_b = (w_b n / sum w)(e1_b - E_m) - (e0_b - E_0)  (SUM)
//   final  res[m][0..4] = [E_0, E_m, E_m - E_0, sqrt((sum d^2 - (sum d)^2 / n) / (n (n - 1))),
//                          (sum w)^2 / sum w^2]
// NaN and inf propagate (the level-1 maximum too).
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <string>

#include "aiqmc.h"
#include "api_util.h"
#include "reduce.h"

namespace {

constexpr int WARP_MAXA = 5;    // the largest A of a built shape
constexpr int WARP_ROW = 16;    // lanes per (m, b): the largest N of a built shape
constexpr int WARP_WG = 256;    // 16 rows per workgroup

struct WarpAtoms {
  double r[3 * WARP_MAXA];
};

__device__ __forceinline__ float warp_log(float x) { return logf(x); }
__device__ __forceinline__ double warp_log(double x) { return log(x); }
__device__ __forceinline__ float warp_sqrt(float x) { return sqrtf(x); }
__device__ __forceinline__ double warp_sqrt(double x) { return sqrt(x); }
__device__ __forceinline__ float warp_abs(float x) { return fabsf(x); }
__device__ __forceinline__ double warp_abs(double x) { return fabs(x); }

// pos [B][3N], new_atoms [M][A][3] (double) -> newpos [M][B][3N], logjac [M][B] (optional)
template <typename T>
__global__ __launch_bounds__(WARP_WG) void k_space_warp(const T* __restrict__ pos, const double* __restrict__ new_atoms,
                                                        WarpAtoms at, int N, int A, int B, int64_t nrows,
                                                        T* __restrict__ newpos, T* __restrict__ logjac) {
  const int e = threadIdx.x % WARP_ROW;
  const int64_t q = (int64_t)blockIdx.x * (WARP_WG / WARP_ROW) + threadIdx.x / WARP_ROW;   // m B + b
  const bool act = q < nrows && e < N;
  T ld = T(0);
  if (act) {
    const int64_t m = q / B, b = q - m * B;
    const T* x = pos + ((size_t)b * N + e) * 3;
    const T r[3] = {x[0], x[1], x[2]};
    T d[WARP_MAXA][3], r2[WARP_MAXA], ra[WARP_MAXA];
    T rmin = T(0);
    int nn = 0;
#pragma unroll
    for (int a = 0; a < WARP_MAXA; ++a)
      if (a < A) {
#pragma unroll
        for (int c = 0; c < 3; ++c) d[a][c] = r[c] - (T)at.r[3 * a + c];
        r2[a] = d[a][0] * d[a][0] + d[a][1] * d[a][1] + d[a][2] * d[a][2];
        ra[a] = warp_sqrt(r2[a]);
        if (a == 0 || ra[a] < rmin) {
          rmin = ra[a];
          nn = a;
        }
      }
    // dR_a - dR_n, formed in double
    const double* na = new_atoms + (size_t)m * A * 3;
    double dn[3] = {0.0, 0.0, 0.0};
#pragma unroll
    for (int a = 0; a < WARP_MAXA; ++a)
      if (a == nn) {
#pragma unroll
        for (int c = 0; c < 3; ++c) dn[c] = na[3 * a + c] - at.r[3 * a + c];
      }
    T D[WARP_MAXA][3], w[WARP_MAXA];
    T S = T(0);
#pragma unroll
    for (int a = 0; a < WARP_MAXA; ++a)
      if (a < A) {
#pragma unroll
        for (int c = 0; c < 3; ++c) D[a][c] = (T)((na[3 * a + c] - at.r[3 * a + c]) - dn[c]);
        if (rmin == T(0)) {
          w[a] = ra[a] == T(0) ? T(1) : T(0);
        } else {
          const T t = rmin / ra[a], t2 = t * t;
          w[a] = t2 * t2;
        }
        S += w[a];
      }
    T mv[3] = {T(0), T(0), T(0)};
    T J[3][3] = {{T(1), T(0), T(0)}, {T(0), T(1), T(0)}, {T(0), T(0), T(1)}};
#pragma unroll
    for (int a = 0; a < WARP_MAXA; ++a)
      if (a < A) {
        w[a] = w[a] / S;
#pragma unroll
        for (int c = 0; c < 3; ++c) mv[c] += w[a] * D[a][c];
      }
    if (rmin != T(0)) {
      T g[WARP_MAXA][3];
#pragma unroll
      for (int a = 0; a < WARP_MAXA; ++a)
        if (a < A) {
#pragma unroll
          for (int c = 0; c < 3; ++c) g[a][c] = d[a][c] / r2[a];
        }
#pragma unroll
      for (int a = 0; a < WARP_MAXA; ++a)
        if (a < A) {
          T G[3] = {T(0), T(0), T(0)};
#pragma unroll
          for (int b2 = 0; b2 < WARP_MAXA; ++b2)
            if (b2 < A && b2 != a) {
#pragma unroll
              for (int c = 0; c < 3; ++c) G[c] += w[b2] * (g[b2][c] - g[a][c]);
            }
#pragma unroll
          for (int k = 0; k < 3; ++k)
#pragma unroll
            for (int l = 0; l < 3; ++l) J[k][l] += D[a][k] * (T(4) * w[a] * G[l]);
        }
    }
    T* y = newpos + ((size_t)q * N + e) * 3;
#pragma unroll
    for (int c = 0; c < 3; ++c) y[c] = r[c] + ((T)dn[c] + mv[c]);
    const T det = J[0][0] * (J[1][1] * J[2][2] - J[1][2] * J[2][1]) - J[0][1] * (J[1][0] * J[2][2] - J[1][2] * J[2][0]) +
                  J[0][2] * (J[1][0] * J[2][1] - J[1][1] * J[2][0]);
    ld = warp_log(warp_abs(det));
  }
  // every lane of the wave takes part; lane 0 of the row adds its electrons in ascending order
  const int row0 = (threadIdx.x & 63) & ~(WARP_ROW - 1);
  T s = T(0);
  for (int i = 0; i < N; ++i) s += __shfl(ld, row0 + i, 64);
  if (logjac && q < nrows && e == 0) logjac[q] = s;
}

// ---- estimator levels (sums and the maximum: reduce.h's butterfly-then-ordered form)
using aq::block_max_nan;
using aq::block_sum;
using aq::nan_max;

template <typename T>
__device__ __forceinline__ double corr_lw(const T* la0, const T* la1, const T* lj, int64_t i) {
  return 2.0 * ((double)la1[i] - (double)la0[i]) + (double)lj[i];
}

template <typename T>
__global__ __launch_bounds__(1024) void k_corr_l1(const T* __restrict__ la0, const T* __restrict__ la1,
                                                  const T* __restrict__ lj, int64_t n, double* __restrict__ out) {
  __shared__ double red[16];
  const int m = blockIdx.x;
  la1 += (size_t)m * n;
  lj += (size_t)m * n;
  double v = -INFINITY;
  for (int64_t i = threadIdx.x; i < n; i += blockDim.x) v = nan_max(v, corr_lw(la0, la1, lj, i));
  v = block_max_nan(v, red);
  if (threadIdx.x == 0) out[m] = v;
}

template <typename T>
__global__ __launch_bounds__(1024) void k_corr_l2(const T* __restrict__ la0, const T* __restrict__ e0,
                                                  const T* __restrict__ la1, const T* __restrict__ lj,
                                                  const T* __restrict__ e1, int64_t n, const double* __restrict__ L1,
                                                  double* __restrict__ out) {
  __shared__ double red[16];
  const int m = blockIdx.x;
  la1 += (size_t)m * n;
  lj += (size_t)m * n;
  e1 += (size_t)m * n;
  const double mx = L1[m];
  double s0 = 0.0, sw = 0.0, swe = 0.0, sw2 = 0.0;
  for (int64_t i = threadIdx.x; i < n; i += blockDim.x) {
    const double w = exp(corr_lw(la0, la1, lj, i) - mx);
    s0 += (double)e0[i];
    sw += w;
    swe += w * (double)e1[i];
    sw2 += w * w;
  }
  s0 = block_sum(s0, red);
  sw = block_sum(sw, red);
  swe = block_sum(swe, red);
  sw2 = block_sum(sw2, red);
  if (threadIdx.x == 0) {
    double* o = out + 5 * (size_t)m;
    o[0] = (double)n;
    o[1] = s0;
    o[2] = sw;
    o[3] = swe;
    o[4] = sw2;
  }
}

template <typename T>
__global__ __launch_bounds__(1024) void k_corr_l3(const T* __restrict__ la0, const T* __restrict__ e0,
                                                  const T* __restrict__ la1, const T* __restrict__ lj,
                                                  const T* __restrict__ e1, int64_t n, const double* __restrict__ L1,
                                                  const double* __restrict__ L2, double* __restrict__ out) {
  __shared__ double red[16];
  const int m = blockIdx.x;
  la1 += (size_t)m * n;
  lj += (size_t)m * n;
  e1 += (size_t)m * n;
  const double mx = L1[m];
  const double* l2 = L2 + 5 * (size_t)m;
  const double E0 = l2[1] / l2[0], Em = l2[3] / l2[2], scale = l2[0] / l2[2];
  double sd = 0.0, sd2 = 0.0;
  for (int64_t i = threadIdx.x; i < n; i += blockDim.x) {
    const double w = exp(corr_lw(la0, la1, lj, i) - mx);
    const double d = (w * scale) * ((double)e1[i] - Em) - ((double)e0[i] - E0);
    sd += d;
    sd2 += d * d;
  }
  sd = block_sum(sd, red);
  sd2 = block_sum(sd2, red);
  if (threadIdx.x == 0) {
    out[2 * (size_t)m] = sd;
    out[2 * (size_t)m + 1] = sd2;
  }
}

__global__ void k_corr_final(const double* __restrict__ L2, const double* __restrict__ L3, int M,
                             double* __restrict__ res) {
#pragma clang fp contract(off)
  const int m = blockIdx.x * blockDim.x + threadIdx.x;
  if (m >= M) return;
  const double* l2 = L2 + 5 * (size_t)m;
  const double n = l2[0], sd = L3[2 * (size_t)m], sd2 = L3[2 * (size_t)m + 1];
  const double E0 = l2[1] / n, Em = l2[3] / l2[2];
  double* r = res + 5 * (size_t)m;
  r[0] = E0;
  r[1] = Em;
  r[2] = Em - E0;
  r[3] = sqrt((sd2 - sd * sd / n) / (n * (n - 1.0)));
  r[4] = l2[2] * l2[2] / l2[4];
}

}  // namespace

extern "C" {

int aiqmc_space_warp(aiqmc_ctx* c, const void* pos, int32_t B, const double* new_atoms, int32_t M, void* newpos,
                     void* logjac, void* stream) {
  if (!c) return fail(AIQMC_EINVAL, "null context");
  if (B < 0 || M < 0) return fail(AIQMC_EINVAL, "negative batch or geometry count");
  if (!pos || !new_atoms || !newpos) return fail(AIQMC_EINVAL, "null pos / new_atoms / newpos");
  if (c->A > WARP_MAXA || c->N > WARP_ROW) return fail(AIQMC_EUNSUPPORTED, "space warp is built for A <= 5, N <= 16");
  if (B == 0 || M == 0) return AIQMC_OK;
  const int64_t nrows = (int64_t)M * B;
  if (nrows > ((int64_t)1 << 34)) return fail(AIQMC_EINVAL, "too many warped configurations for one call");
  HIPCHK(hipSetDevice(c->device));
  WarpAtoms at;
  for (int i = 0; i < 3 * WARP_MAXA; ++i) at.r[i] = i < 3 * c->A ? c->atoms[i] : 0.0;
  by_dtype(c->dtype, [&](auto t) {
    using T = decltype(t);
    k_space_warp<T><<<blocks(nrows, WARP_WG / WARP_ROW), dim3(WARP_WG), 0, (hipStream_t)stream>>>(
        (const T*)pos, new_atoms, at, c->N, c->A, B, nrows, (T*)newpos, (T*)logjac);
  });
  HIPCHK(hipGetLastError());
  return AIQMC_OK;
}

int aiqmc_corr_level(int32_t level, int32_t dtype, int64_t n, int32_t M, const void* logabs0, const void* e0,
                     const void* logabs1, const void* logjac, const void* e1, const double* L1, const double* L2,
                     double* out, void* stream) {
  if (n <= 0 || M <= 0) return fail(AIQMC_EINVAL, "empty batch or no geometry");
  if (!is_dtype(dtype)) return fail(AIQMC_EINVAL, "dtype must be AIQMC_F32 or AIQMC_F64");
  if (level < 1 || level > 3) return fail(AIQMC_EINVAL, "level must be 1, 2 or 3");
  if (!logabs0 || !logabs1 || !logjac || !out) return fail(AIQMC_EINVAL, "null argument");
  if (level >= 2 && (!e0 || !e1 || !L1)) return fail(AIQMC_EINVAL, "levels 2 and 3 need e0, e1 and the combined L1");
  if (level == 3 && !L2) return fail(AIQMC_EINVAL, "level 3 needs the summed L2");
  by_dtype(dtype, [&](auto t) {
    using T = decltype(t);
    const dim3 grid(M), wg(1024);
    hipStream_t s = (hipStream_t)stream;
    const T *a0 = (const T*)logabs0, *a1 = (const T*)logabs1, *lj = (const T*)logjac;
    if (level == 1)
      k_corr_l1<T><<<grid, wg, 0, s>>>(a0, a1, lj, n, out);
    else if (level == 2)
      k_corr_l2<T><<<grid, wg, 0, s>>>(a0, (const T*)e0, a1, lj, (const T*)e1, n, L1, out);
    else
      k_corr_l3<T><<<grid, wg, 0, s>>>(a0, (const T*)e0, a1, lj, (const T*)e1, n, L1, L2, out);
  });
  HIPCHK(hipGetLastError());
  return AIQMC_OK;
}

int aiqmc_corr_final(const double* L2, const double* L3, int32_t M, double* res, void* stream) {
  if (!L2 || !L3 || !res || M <= 0) return fail(AIQMC_EINVAL, "null argument");
  k_corr_final<<<blocks(M, 64), dim3(64), 0, (hipStream_t)stream>>>(L2, L3, M, res);
  HIPCHK(hipGetLastError());
  return AIQMC_OK;
}

}  // extern "C"
