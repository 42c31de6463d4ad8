// observables.hip -- expectation values other than the energy: the spin-squared estimator for a
// fixed spin assignment (aiqmc_spin_squared) and the dipole moment (aiqmc_dipole).
//
//   S2_L(x) = (na - nb)/2 ((na - nb)/2 + 1) + nb - sum_{i in up} sum_{j in down} psi(x_{i<->j}) / psi(x)
//
// with na = max(n_up, n_down), nb = min(n_up, n_down) and x_{i<->j} = x with the coordinates of
// electron slots i and j exchanged (the spin labels stay on the slots).  Pair k = ia * n_down + ib
// exchanges i = spin_up_indices[ia] and j = spin_down_indices[ib].
//
// Per chunk of W walkers, three launches on the caller's stream:
//   k_s2_exchange  the W (K + 1) configurations [w][p][3N], K = n_up n_down: p = 0 the walker
//                  itself, p = 1 + k its pair-k exchange (one thread per configuration and electron)
//   value launch   log|psi| and the phase of all of them: ShapeOps::walker with aiqmc_logpsi's
//                  arguments, so the packed kernels for N <= 8 and the same bits as aiqmc_logpsi
//   k_s2_reduce    one group of G lanes per walker (G = the power of two >= K, at least 4: 64 / G
//                  walkers per wave; K <= 64 since N <= 16), lane l holds pair l's ratio
//                  exp(dlogabs) (cos dphase, sin dphase); an xor butterfly sums the group in a fixed
//                  order, so the estimator is the same bits run to run and for any chunking
// W = obs_chunk / (K + 1): the workspace (configurations, values, the value launch's walker cache)
// is sized by the chunk and does not grow with the batch.  Nothing is clamped: a walker on a node
// of psi gives an infinite or NaN ratio, as the expression does.
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstring>
#include <string>

#include "aiqmc.h"
#include "host_shared.h"
#include "jets.h"

using namespace aq;

namespace {

constexpr int OBS_CHUNK_DEFAULT = 4096;   // configurations per value launch

// x[q][3N] for q = w (K + 1) + p < nconf from walkers pos[b0 + w][3N]; rowsrc: up slots then down slots
template <typename T>
__global__ __launch_bounds__(256) void k_s2_exchange(const T* __restrict__ pos, const int* __restrict__ rowsrc, int N,
                                                     int nup, int ndn, int b0, int nconf, T* __restrict__ x) {
  const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (t >= (int64_t)nconf * N) return;
  const int q = (int)(t / N), e = (int)(t - (int64_t)q * N);
  const int K1 = nup * ndn + 1;
  const int w = q / K1, p = q - w * K1;
  int src = e;
  if (p > 0) {
    const int k = p - 1;
    const int i = rowsrc[k / ndn], j = rowsrc[nup + k % ndn];
    src = e == i ? j : (e == j ? i : e);
  }
  const T* xs = pos + (size_t)(b0 + w) * 3 * N + 3 * src;
  T* xd = x + (size_t)q * 3 * N + 3 * e;
#pragma unroll
  for (int c = 0; c < 3; ++c) xd[c] = xs[c];
}

// lp / ph [nw][K + 1] of one chunk -> s2_re / s2_im [b0 + w], dlogabs / dphase [b0 + w][K] (optional)
template <typename T, int G>
__global__ __launch_bounds__(64) void k_s2_reduce(const T* __restrict__ lp, const T* __restrict__ ph, int K, int b0,
                                                  int nw, T diag, T* __restrict__ s2_re, T* __restrict__ s2_im,
                                                  T* __restrict__ dlogabs, T* __restrict__ dphase) {
  const int lane = threadIdx.x;
  const int w = blockIdx.x * (64 / G) + lane / G, l = lane % G;
  const bool act = w < nw && l < K;
  T re = T(0), im = T(0);
  if (act) {
    const size_t q0 = (size_t)w * (K + 1);
    const T dl = lp[q0 + 1 + l] - lp[q0], dp = ph[q0 + 1 + l] - ph[q0];
    unit_ratio(dl, dp, re, im);
    const size_t o = (size_t)(b0 + w) * K + l;
    if (dlogabs) dlogabs[o] = dl;
    if (dphase) dphase[o] = dp;
  }
  // every lane of the wave takes part; the partner lane ^ m stays inside the group
#pragma unroll
  for (int m = G / 2; m >= 1; m >>= 1) {
    re += __shfl_xor(re, m);
    im += __shfl_xor(im, m);
  }
  if (w < nw && l == 0) {
    s2_re[b0 + w] = diag - re;
    s2_im[b0 + w] = -im;
  }
}

// mu[b][c] = nuc[c] - sum_i pos[b][3 i + c], electrons in ascending order
template <typename T>
__global__ __launch_bounds__(256) void k_dipole(const T* __restrict__ pos, int N, int B, double n0, double n1,
                                                double n2, T* __restrict__ mu) {
  const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (t >= (int64_t)B * 3) return;
  const int64_t b = t / 3;
  const int c = (int)(t - 3 * b);
  T s = T(0);
  for (int i = 0; i < N; ++i) s += pos[(size_t)b * 3 * N + 3 * i + c];
  mu[t] = (T)(c == 0 ? n0 : (c == 1 ? n1 : n2)) - s;
}

template <typename T>
void s2_reduce_launch(int G, int nw, const void* lp, const void* ph, int K, int b0, double diag, void* re, void* im,
                      void* dl, void* dp, hipStream_t s) {
#define OBS_RED(g)                                                                                            \
  k_s2_reduce<T, g><<<dim3((nw + 64 / g - 1) / (64 / g)), dim3(64), 0, s>>>((const T*)lp, (const T*)ph, K, b0, nw, \
                                                                            (T)diag, (T*)re, (T*)im, (T*)dl, (T*)dp)
  if (G == 4) OBS_RED(4);
  else if (G == 8) OBS_RED(8);
  else if (G == 16) OBS_RED(16);
  else if (G == 32) OBS_RED(32);
  else OBS_RED(64);
#undef OBS_RED
}

}  // namespace

// host_shared.h: the chunk workspace and the value launch, shared with rdm.hip
int aq_host::ensure_obs(aiqmc_ctx* c, int nconf, const ShapeOps& ops) {
  const size_t s = elem_size(c), n = (size_t)nconf;
  HIPCHK(c->d_obs_x.reserve(n * 3 * c->N * s));
  HIPCHK(c->d_obs_lp.reserve(n * s));
  HIPCHK(c->d_obs_ph.reserve(n * s));
  HIPCHK(c->d_obs_wc.reserve(n * ops.wcache_n * s));
  return 0;
}
void aq_host::obs_values(aiqmc_ctx* c, const ShapeOps& ops, int nconf, hipStream_t s) {
  WalkerCall w = launch_args(c, Launch::WalkerValue, c->d_obs_x.as(), nconf, c->d_obs_lp.as(), &c->d_obs_wc);   // aiqmc_logpsi's
  w.ka.phase = c->d_obs_ph.as();
  ops.walker(c->dtype, w, nconf, s);
}

extern "C" {

int aiqmc_spin_squared(aiqmc_ctx* c, const void* pos, int32_t B, void* s2_re, void* s2_im, void* dlogabs,
                       void* dphase, void* stream) {
  AIQMC_ENTER(c, pos, B, ops);
  if (!s2_re || !s2_im) return fail(AIQMC_EINVAL, "null s2_re / s2_im");
  const int K = c->nup * c->ndn;
  if ((int64_t)B * K > INT32_MAX) return fail(AIQMC_EINVAL, "too many exchanged configurations for one call");
  int W = c->obs_chunk / (K + 1);   // walkers per chunk
  if (W < 1) W = 1;
  if (W > B) W = B;
  if (int rc = aq_host::ensure_obs(c, W * (K + 1), ops)) return rc;
  const int na = c->nup > c->ndn ? c->nup : c->ndn, nb = c->nup + c->ndn - na;
  const double sz = 0.5 * (na - nb), diag = sz * (sz + 1.0) + nb;
  int G = 4;
  while (G < K) G *= 2;
  hipStream_t s = (hipStream_t)stream;
  void *lp = c->d_obs_lp.as(), *ph = c->d_obs_ph.as();
  for (int b0 = 0; b0 < B; b0 += W) {
    const int nw = B - b0 < W ? B - b0 : W;
    const int nconf = nw * (K + 1);
    by_dtype(c->dtype, [&](auto t) {
      using T = decltype(t);
      k_s2_exchange<T><<<blocks((int64_t)nconf * c->N, 256), dim3(256), 0, s>>>(
          (const T*)pos, c->d_rowsrc.as<int>(), c->N, c->nup, c->ndn, b0, nconf, c->d_obs_x.as<T>());
      aq_host::obs_values(c, ops, nconf, s);
      s2_reduce_launch<T>(G, nw, lp, ph, K, b0, diag, s2_re, s2_im, dlogabs, dphase, s);
    });
  }
  HIPCHK(hipGetLastError());
  return AIQMC_OK;
}

int aiqmc_dipole(aiqmc_ctx* c, const void* pos, int32_t B, void* mu, void* stream) {
  if (!c) return fail(AIQMC_EINVAL, "null context");
  if (B < 0) return fail(AIQMC_EINVAL, "negative batch");
  if (B == 0) return AIQMC_OK;
  if (!pos) return fail(AIQMC_EINVAL, "null positions");
  if (!mu) return fail(AIQMC_EINVAL, "null mu");
  HIPCHK(hipSetDevice(c->device));
  double nuc[3] = {0.0, 0.0, 0.0};
  for (int a = 0; a < c->A; ++a)
    for (int d = 0; d < 3; ++d) nuc[d] += c->charges[a] * c->atoms[3 * a + d];
  hipStream_t s = (hipStream_t)stream;
  by_dtype(c->dtype, [&](auto t) {
    using T = decltype(t);
    k_dipole<T><<<blocks((int64_t)B * 3, 256), dim3(256), 0, s>>>((const T*)pos, c->N, B, nuc[0], nuc[1], nuc[2], (T*)mu);
  });
  HIPCHK(hipGetLastError());
  return AIQMC_OK;
}

int aiqmc_debug_set_obs_chunk(aiqmc_ctx* c, int32_t nconf) {
  if (!c) return fail(AIQMC_EINVAL, "null context");
  c->obs_chunk = nconf > 0 ? nconf : OBS_CHUNK_DEFAULT;
  return AIQMC_OK;
}

}  // extern "C"
