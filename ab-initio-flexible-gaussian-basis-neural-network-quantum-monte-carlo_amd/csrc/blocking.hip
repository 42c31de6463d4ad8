// blocking.hip -- serial-correlation-aware error bars: the Flyvbjerg-Petersen blocking analysis of
// K time series over B Markov chains in its online form (aiqmc_blocking_layout,
// aiqmc_blocking_update).  No trace is stored: the state is O(log T) sums per series plus one
// waiting block per (level, series, chain), all caller-owned and resident on the device.
//
// State (doubles):
//   acc      [t, shift[K], level 0 words[M], .., level L-1 words[M]],  M = 1 + K + K (K + 1) / 2,
//            a level's words = [n, S[K], Q[K (K + 1) / 2]] (Q: upper triangle i <= j, row-major)
//   pend     [L][K][B]: pend[k] holds the level-(k-1) block of a chain that has no partner yet
//            (pend[0] is never used)
//   scratch  [chunks][L][M - 1]: the chunk partials of one call, chunks = ceil(B / 256)
//
// Sample number t (0-based, read from acc[0] on the device, so the host never knows how many
// levels complete): v_0 = x - shift completes level 0; for k = 0, 1, ..: stop if k + 1 == L; if bit
// k of t is set, v_{k+1} = (pend[k+1] + v_k) / 2 completes level k + 1, go on; otherwise pend[k+1] =
// v_k, stop.  Every completing level adds n += B, S[i] += sum_b v_i, Q[i][j] += sum_b v_i v_j.
// Nothing is clamped, everything is fp64 (fp32 samples widen exactly), NaN and inf propagate into
// exactly the levels they reach.
//
// Two launches, no atomics, a fixed summation order:
//   k_blocking_chunks   one 256-thread workgroup per chunk of 256 chains, thread = chain: the
//                       cascade above, and per completing level and word an xor-butterfly over the
//                       wave followed by ((w0 + w1) + w2) + w3 over the four waves through LDS;
//                       lanes beyond B add +0.0.  Reads t, writes pend and scratch.
//   k_blocking_combine  ONE workgroup; thread e owns word e of the completing levels and adds the
//                       chunk partials in ascending chunk order, then the sum into acc.  Every
//                       thread reads t before the barrier, thread 0 writes t + 1 after it.
// The words are therefore a function of (B, the samples) only: the same bits from run to run.
// The number of completing levels is uniform over both launches (it depends on t alone); grid
// and scratch are sized for all L levels.
#include <hip/hip_runtime.h>

#include <cstdint>
#include <string>

#include "aiqmc.h"
#include "api_util.h"

static_assert(AIQMC_BLOCKING_MAX_SERIES == 8, "aiqmc_blocking_update instantiates K = 1..8");
static_assert(AIQMC_BLOCKING_MAX_LEVELS <= 64, "the level bits of t are taken from a uint64");

namespace {

constexpr int BLK_CHUNK = 256;                      // chains per workgroup, the unit of the summation order
constexpr int64_t BLK_MAX_B = (int64_t)1 << 38;      // 2^30 chunks: inside the grid limit, no int64 overflow

constexpr int blk_words(int K) { return K + K * (K + 1) / 2; }   // S and Q of one level (M - 1)

// out[w] = the sum over the workgroup's 256 chains of word w of v: S then Q, in the layout's order
template <int K>
__device__ __forceinline__ void chunk_sums(const double (&v)[K], double (*red)[blk_words(K)], double* __restrict__ out) {
#pragma clang fp contract(off)
  constexpr int MW = blk_words(K);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  double term[MW];
#pragma unroll
  for (int i = 0; i < K; ++i) term[i] = v[i];
  int w = K;
#pragma unroll
  for (int i = 0; i < K; ++i)
#pragma unroll
    for (int j = i; j < K; ++j) term[w++] = v[i] * v[j];
  // butterfly step outermost: the MW exchanges of a step are independent and stay in flight
  // together (word outermost, the steps of one word wait for each other: 12 us per level at K = 8)
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    double other[MW];
#pragma unroll
    for (int q = 0; q < MW; ++q) other[q] = __shfl_xor(term[q], o);
#pragma unroll
    for (int q = 0; q < MW; ++q) term[q] += other[q];
  }
  if (lane == 0) {
#pragma unroll
    for (int q = 0; q < MW; ++q) red[wave][q] = term[q];
  }
  __syncthreads();
  if (threadIdx.x < MW) {
    const int q = threadIdx.x;
    out[q] = ((red[0][q] + red[1][q]) + red[2][q]) + red[3][q];
  }
  __syncthreads();   // red is written again at the next level
}

template <typename T, int K>
__global__ __launch_bounds__(BLK_CHUNK) void k_blocking_chunks(const T* __restrict__ x, int64_t B, int L,
                                                               const double* __restrict__ acc, double* __restrict__ pend,
                                                               double* __restrict__ scratch) {
  constexpr int MW = blk_words(K);
  __shared__ double red[4][MW];
  const int64_t b = (int64_t)blockIdx.x * BLK_CHUNK + threadIdx.x;
  const bool live = b < B;
  const uint64_t t = (uint64_t)acc[0];   // the same for every thread of the launch
  double v[K];
#pragma unroll
  for (int i = 0; i < K; ++i) v[i] = live ? (double)x[(int64_t)i * B + b] - acc[1 + i] : 0.0;
  double* out = scratch + (int64_t)blockIdx.x * L * MW;
  for (int k = 0;; ++k) {   // every branch on k, L and t is uniform
    chunk_sums<K>(v, red, out + (int64_t)k * MW);
    if (k + 1 == L) break;
    double* p = pend + (int64_t)(k + 1) * K * B + b;
    if ((t >> k) & 1) {
      if (live) {
#pragma unroll
        for (int i = 0; i < K; ++i) v[i] = (p[(int64_t)i * B] + v[i]) / 2.0;
      }
    } else {
      if (live) {
#pragma unroll
        for (int i = 0; i < K; ++i) p[(int64_t)i * B] = v[i];
      }
      break;
    }
  }
}

__global__ __launch_bounds__(BLK_CHUNK) void k_blocking_combine(int64_t B, int K, int L, int64_t chunks,
                                                                double* __restrict__ acc,
                                                                const double* __restrict__ scratch) {
  const int MW = blk_words(K), M = MW + 1;
  const double td = acc[0];
  const uint64_t t = (uint64_t)td;
  int nl = 1;   // completing levels: level 0, then one more per trailing set bit of t, up to L
  while (nl < L && ((t >> (nl - 1)) & 1)) ++nl;
  __syncthreads();   // every reader has t
  double* lev = acc + 1 + K;
  for (int e = threadIdx.x; e < nl * M; e += BLK_CHUNK) {
    const int k = e / M, w = e - k * M;
    if (w == 0) {
      lev[e] += (double)B;
    } else {
      const double* part = scratch + (int64_t)k * MW + (w - 1);
      double s = part[0];
      for (int64_t c = 1; c < chunks; ++c) s += part[c * L * MW];
      lev[e] += s;
    }
  }
  if (threadIdx.x == 0) acc[0] = td + 1.0;
}

int blk_check(int64_t B, int32_t K, int32_t L) {
  if (B < 1) return fail(AIQMC_EINVAL, "blocking: B must be at least 1");
  if (B > BLK_MAX_B) return fail(AIQMC_EINVAL, "blocking: B above 2^38");
  if (K < 1 || K > AIQMC_BLOCKING_MAX_SERIES)
    return fail(AIQMC_EINVAL, "blocking: K must be in 1.." + std::to_string(AIQMC_BLOCKING_MAX_SERIES));
  if (L < 1 || L > AIQMC_BLOCKING_MAX_LEVELS)
    return fail(AIQMC_EINVAL, "blocking: L must be in 1.." + std::to_string(AIQMC_BLOCKING_MAX_LEVELS));
  return 0;
}

template <typename T, int K>
void blk_launch_chunks(const void* x, int64_t B, int L, const double* acc, double* pend, double* scratch, dim3 grd,
                       hipStream_t s) {
  k_blocking_chunks<T, K><<<grd, dim3(BLK_CHUNK), 0, s>>>((const T*)x, B, L, acc, pend, scratch);
}

}  // namespace

extern "C" {

int aiqmc_blocking_layout(int64_t B, int32_t K, int32_t L, int64_t* acc_words, int64_t* pend_words,
                          int64_t* scratch_words) {
  if (int rc = blk_check(B, K, L)) return rc;
  if (!acc_words || !pend_words || !scratch_words)
    return fail(AIQMC_EINVAL, "blocking: null acc_words / pend_words / scratch_words");
  const int64_t chunks = (B + BLK_CHUNK - 1) / BLK_CHUNK;
  *acc_words = 1 + K + (int64_t)L * (1 + blk_words(K));
  *pend_words = (int64_t)L * K * B;
  *scratch_words = chunks * L * blk_words(K);
  return AIQMC_OK;
}

int aiqmc_blocking_update(const void* x, int32_t dtype, int64_t B, int32_t K, int32_t L, double* acc, double* pend,
                          double* scratch, void* stream) {
  if (!x) return fail(AIQMC_EINVAL, "blocking: null x");
  if (!acc) return fail(AIQMC_EINVAL, "blocking: null acc");
  if (!pend) return fail(AIQMC_EINVAL, "blocking: null pend");
  if (!scratch) return fail(AIQMC_EINVAL, "blocking: null scratch");
  if (int rc = blk_check(B, K, L)) return rc;
  if (!is_dtype(dtype)) return fail(AIQMC_EINVAL, "blocking: dtype must be AIQMC_F32 or AIQMC_F64");
  hipStream_t s = (hipStream_t)stream;
  const int64_t chunks = (B + BLK_CHUNK - 1) / BLK_CHUNK;
  const dim3 grd((unsigned)chunks);
  by_dtype(dtype, [&](auto t) {
    using T = decltype(t);
    switch (K) {
#define BLK_CASE(k) \
  case k:           \
    blk_launch_chunks<T, k>(x, B, L, acc, pend, scratch, grd, s); \
    break;
      BLK_CASE(1) BLK_CASE(2) BLK_CASE(3) BLK_CASE(4) BLK_CASE(5) BLK_CASE(6) BLK_CASE(7) BLK_CASE(8)
#undef BLK_CASE
    }
  });
  HIPCHK(hipGetLastError());
  k_blocking_combine<<<dim3(1), dim3(BLK_CHUNK), 0, s>>>(B, K, L, chunks, acc, scratch);
  HIPCHK(hipGetLastError());
  return AIQMC_OK;
}

}  // extern "C"
