// aiqmc_sr_gram: the centred Gram product of the per-walker parameter Jacobian, the heavy part of the
// exact Fisher matrix S = Cov_b(O_b) of stochastic reconfiguration (aiqmc/Optimizer/sr.py).
//
//   G[i][j] = sum_b (o_re[b][i] - c_re[i]) (o_re[b][j] - c_re[j]) + the same with o_im, c_im
//
// One workgroup (4 waves) owns one 64 x 64 tile of G for ALL walkers: no atomics, so the result is
// the same bits run to run.  Only tiles with tj >= ti are computed; both triangles are written.
// The product runs on the matrix cores, v_mfma_{f32,f64}_16x16x4 with K = walker: lane l's A
// operand is A[m = l & 15][k = l >> 4] = O[b + (l >> 4)][i0 + (l & 15)], the B operand the same
// with j0, i.e. 16 consecutive columns of one walker row; the centre is subtracted (and tail
// rows / columns set to zero) when the panel of SR_PANEL walker rows is staged in LDS.
// Summation order (fixed, independent of the grid): the operand dtype over one part (re, then im)
// of SR_CHUNK walkers in ascending walker order -- for float bit for bit an fmaf chain -- then
// that chunk tile added into fp64 accumulators, chunks ascending.  The column sums s_re, s_im come
// from the diagonal tiles: each thread sums the values it stages (rows rg, rg + 4, .. of the
// chunk in the operand dtype, chunks in fp64), the four row groups are combined in fp64.
#include <hip/hip_runtime.h>

#include <cstdint>
#include <string>

#include "aiqmc.h"
#include "api_util.h"

static_assert(AIQMC_SR_CHUNK % 4 == 0, "SR_CHUNK is a whole number of K = 4 MFMA steps");

namespace {

constexpr int SR_TILE = 64;                  // output tile edge (4 x 4 MFMA tiles, 2 x 2 per wave)
constexpr int SR_PANEL = 32;                 // walker rows staged per barrier pair
constexpr int SR_LDS_STRIDE = SR_TILE + 16;  // floats: the 4 rows one MFMA operand reads fall in disjoint banks
constexpr int SR_T_STRIDE = SR_TILE + 1;     // the fp64 tile staged for the (transposed) write-out
constexpr int SR_PANELS_PER_CHUNK = AIQMC_SR_CHUNK / SR_PANEL;
constexpr int SR_ROWS_PER_THREAD = SR_PANEL / 4;   // 256 threads = 64 columns x 4 row groups
static_assert(AIQMC_SR_CHUNK % SR_PANEL == 0, "a chunk is a whole number of panels");

template <typename T> struct SrMfma;
template <> struct SrMfma<float> {
  typedef float v4 __attribute__((ext_vector_type(4)));
  static __device__ __forceinline__ v4 mma(float a, float b, v4 c) {
    return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0);
  }
  // accumulator register v of lane group q holds row 4q + v (column = lane & 15)
  static constexpr __device__ int row(int q, int v) { return 4 * q + v; }
};
template <> struct SrMfma<double> {
  typedef double v4 __attribute__((ext_vector_type(4)));
  static __device__ __forceinline__ v4 mma(double a, double b, v4 c) {
    return __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, c, 0, 0, 0);
  }
  static constexpr __device__ int row(int q, int v) { return q + 4 * v; }   // f64 C/D map
};

template <typename T> constexpr size_t sr_lds_bytes() {
  const size_t panels = (size_t)2 * SR_PANEL * SR_LDS_STRIDE * sizeof(T);
  const size_t tile = (size_t)SR_TILE * SR_T_STRIDE * sizeof(double);
  return panels > tile ? panels : tile;
}

template <typename T>
__global__ __launch_bounds__(256) void k_sr_gram(const T* __restrict__ o_re, const T* __restrict__ o_im, int64_t B,
                                                 int P, const T* __restrict__ c_re, const T* __restrict__ c_im,
                                                 double* __restrict__ out, int accumulate) {
  const int ti = blockIdx.y, tj = blockIdx.x;
  if (tj < ti) return;
  using M = SrMfma<T>;
  using V4 = typename M::v4;
  __shared__ __attribute__((aligned(16))) unsigned char smem[sr_lds_bytes<T>()];
  T* pa = (T*)smem;                               // [SR_PANEL][SR_LDS_STRIDE], columns i0..
  T* pb = pa + SR_PANEL * SR_LDS_STRIDE;          // columns j0..
  double* tile = (double*)smem;                   // after the walker loop: [SR_TILE][SR_T_STRIDE]
  const bool diag = ti == tj;
  const int t = (int)threadIdx.x;
  const int lane = t & 63, wave = t >> 6;
  const int q = lane >> 4, e = lane & 15;
  const int wr = wave >> 1, wc = wave & 1;        // the wave's 32 x 32 quadrant of the tile
  const int i0 = ti * SR_TILE, j0 = tj * SR_TILE;
  // staging role: column lc of the tile, walker rows rg, rg + 4, .. of the panel
  const int lc = t & 63, rg = t >> 6;
  const int ca = i0 + lc, cb = j0 + lc;
  const bool va = ca < P, vb = cb < P;
  const int nparts = o_im ? 2 : 1;
  T cen_a[2] = {T(0), T(0)}, cen_b[2] = {T(0), T(0)};
  if (va && c_re) cen_a[0] = c_re[ca];
  if (vb && c_re) cen_b[0] = c_re[cb];
  if (va && c_im && o_im) cen_a[1] = c_im[ca];
  if (vb && c_im && o_im) cen_b[1] = c_im[cb];

  const int64_t nchunks = (B + AIQMC_SR_CHUNK - 1) / AIQMC_SR_CHUNK;
  const int64_t nit = nchunks * nparts * SR_PANELS_PER_CHUNK;

  T ra[SR_ROWS_PER_THREAD], rb[SR_ROWS_PER_THREAD];
  auto fetch = [&](int64_t it) {
    const int64_t chunk = it / (nparts * SR_PANELS_PER_CHUNK);
    const int rem = (int)(it % (nparts * SR_PANELS_PER_CHUNK));
    const int part = rem / SR_PANELS_PER_CHUNK, pnl = rem % SR_PANELS_PER_CHUNK;
    const T* __restrict__ src = part ? o_im : o_re;
    const int64_t b0 = chunk * AIQMC_SR_CHUNK + (int64_t)pnl * SR_PANEL + rg;
#pragma unroll
    for (int r = 0; r < SR_ROWS_PER_THREAD; ++r) {
      const int64_t b = b0 + 4 * r;
      const bool vr = b < B;
      ra[r] = (vr && va) ? src[(size_t)b * P + ca] - (part ? cen_a[1] : cen_a[0]) : T(0);
      if (!diag) rb[r] = (vr && vb) ? src[(size_t)b * P + cb] - (part ? cen_b[1] : cen_b[0]) : T(0);
    }
  };

  V4 acc[2][2];
  double acc64[2][2][4];
#pragma unroll
  for (int a = 0; a < 2; ++a)
#pragma unroll
    for (int b = 0; b < 2; ++b) {
      acc[a][b] = V4{T(0), T(0), T(0), T(0)};
#pragma unroll
      for (int v = 0; v < 4; ++v) acc64[a][b][v] = 0.0;
    }
  T csum = T(0);                 // diagonal tiles: this thread's column sum of the current chunk part
  double cs64[2] = {0.0, 0.0};

  if (nit > 0) fetch(0);
  for (int64_t it = 0; it < nit; ++it) {
    const int rem = (int)(it % (nparts * SR_PANELS_PER_CHUNK));
    const int part = rem / SR_PANELS_PER_CHUNK, pnl = rem % SR_PANELS_PER_CHUNK;
    __syncthreads();             // the previous panel has been read
#pragma unroll
    for (int r = 0; r < SR_ROWS_PER_THREAD; ++r) {
      pa[(rg + 4 * r) * SR_LDS_STRIDE + lc] = ra[r];
      if (!diag) pb[(rg + 4 * r) * SR_LDS_STRIDE + lc] = rb[r];
      if (diag) csum += ra[r];
    }
    __syncthreads();
    if (it + 1 < nit) fetch(it + 1);
    const T* __restrict__ qa = pa;
    const T* __restrict__ qb = diag ? pa : pb;
#pragma unroll
    for (int ks = 0; ks < SR_PANEL / 4; ++ks) {
      const int ro = (ks * 4 + q) * SR_LDS_STRIDE + e;
      const T a0 = qa[ro + wr * 32], a1 = qa[ro + wr * 32 + 16];
      const T b0 = qb[ro + wc * 32], b1 = qb[ro + wc * 32 + 16];
      acc[0][0] = M::mma(a0, b0, acc[0][0]);
      acc[0][1] = M::mma(a0, b1, acc[0][1]);
      acc[1][0] = M::mma(a1, b0, acc[1][0]);
      acc[1][1] = M::mma(a1, b1, acc[1][1]);
    }
    if (pnl == SR_PANELS_PER_CHUNK - 1) {   // end of this part of the chunk: into the fp64 accumulators
#pragma unroll
      for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int b = 0; b < 2; ++b) {
#pragma unroll
          for (int v = 0; v < 4; ++v) acc64[a][b][v] += (double)acc[a][b][v];
          acc[a][b] = V4{T(0), T(0), T(0), T(0)};
        }
      if (part) cs64[1] += (double)csum; else cs64[0] += (double)csum;
      csum = T(0);
    }
  }

  // the tile through LDS, so that both triangles are written with consecutive lanes on
  // consecutive addresses
  __syncthreads();
#pragma unroll
  for (int a = 0; a < 2; ++a)
#pragma unroll
    for (int b = 0; b < 2; ++b)
#pragma unroll
      for (int v = 0; v < 4; ++v)
        tile[(wr * 32 + a * 16 + M::row(q, v)) * SR_T_STRIDE + wc * 32 + b * 16 + e] = acc64[a][b][v];
  __syncthreads();
  const size_t Ps = (size_t)P;
  for (int idx = t; idx < SR_TILE * SR_TILE; idx += 256) {
    const int hi = idx >> 6, lo = idx & 63;
    {   // G[i0 + hi][j0 + lo]
      const int gi = i0 + hi, gj = j0 + lo;
      if (gi < P && gj < P && (!diag || lo >= hi)) {
        const double v = tile[hi * SR_T_STRIDE + lo];
        double* dst = out + (size_t)gi * Ps + gj;
        *dst = accumulate ? *dst + v : v;
      }
    }
    {   // the mirror G[j0 + hi][i0 + lo] = tile[lo][hi]
      const int gi = i0 + lo, gj = j0 + hi;
      if (gi < P && gj < P && (!diag || hi > lo)) {
        const double v = tile[lo * SR_T_STRIDE + hi];
        double* dst = out + (size_t)gj * Ps + gi;
        *dst = accumulate ? *dst + v : v;
      }
    }
  }

  if (diag) {
    // column sums: the four row groups in ascending order
    __syncthreads();
    double* cs = (double*)smem;                   // [2][4][64]
    cs[(0 * 4 + rg) * 64 + lc] = cs64[0];
    cs[(1 * 4 + rg) * 64 + lc] = cs64[1];
    __syncthreads();
    if (rg == 0 && va) {
#pragma unroll
      for (int p = 0; p < 2; ++p) {
        double s = cs[(p * 4 + 0) * 64 + lc];
        s += cs[(p * 4 + 1) * 64 + lc];
        s += cs[(p * 4 + 2) * 64 + lc];
        s += cs[(p * 4 + 3) * 64 + lc];
        double* dst = out + Ps * Ps + (size_t)p * Ps + ca;
        *dst = accumulate ? *dst + s : s;
      }
    }
    if (ti == 0 && t == 0) {
      double* dst = out + Ps * Ps + 2 * Ps;
      *dst = accumulate ? *dst + (double)B : (double)B;
    }
  }
}

}  // namespace

extern "C" {

int aiqmc_sr_gram(const void* o_re, const void* o_im, int32_t dtype, int64_t B, int32_t P, const void* center_re,
                  const void* center_im, double* out, int32_t accumulate, void* stream) {
  if (!out || P <= 0 || B < 0) return fail(AIQMC_EINVAL, "sr_gram: null out, P <= 0 or B < 0");
  if (B > 0 && !o_re) return fail(AIQMC_EINVAL, "sr_gram: null o_re");
  if (P > 32768) return fail(AIQMC_EINVAL, "sr_gram: P > 32768");
  if (!is_dtype(dtype)) return fail(AIQMC_EINVAL, "dtype must be AIQMC_F32 or AIQMC_F64");
  hipStream_t s = (hipStream_t)stream;
  const int nt = (P + SR_TILE - 1) / SR_TILE;
  const dim3 gr(nt, nt);
  by_dtype(dtype, [&](auto t) {
    using T = decltype(t);
    k_sr_gram<T><<<gr, dim3(256), 0, s>>>((const T*)o_re, (const T*)o_im, B, P, (const T*)center_re,
                                          (const T*)center_im, out, accumulate);
  });
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) return fail(AIQMC_EHIP, std::string("sr_gram: ") + hipGetErrorString(e));
  return AIQMC_OK;
}

}  // extern "C"
