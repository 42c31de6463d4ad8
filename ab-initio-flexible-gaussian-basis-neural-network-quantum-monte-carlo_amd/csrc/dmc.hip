// dmc.hip -- the diffusion Monte Carlo entry points (aiqmc_dmc_*) and their kernels: the
// drift-diffusion sums, the energy-cut minima, the weights and the stochastic comb.  The sweep and
// the pseudopotential quadrature are the VMC / ECP paths' (mc_sweep, ecp_quadrature: aiqmc.hip,
// through host_shared.h); k_tmove and k_tmove_none are ecp.h's.  Kernels defined here:
//   k_dmc_sum_part, k_dmc_sum_fin       coordinate sums of the drift-diffusion step (tdamp)
//   k_scale_grad                        limdrift of a gradient
//   k_dmc_cut_part, k_dmc_cut_fin       energy-cut minima
//   k_dmc_weights                       weight update
//   k_dmc_branch                        stochastic comb
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <string>

#include "aiqmc.h"
#include "host_shared.h"
#include "reduce.h"
#include "ecp.h"

using namespace aq;
using namespace aq_host;

// ============================================================================ kernels

// DMC reductions run over DMC_NB blocks (partial sums / minima per block in a fixed order), then
// one thread combines the block results in block order: deterministic, and the chip is not
// reduced to one block (the single-block forms took 29 us (sum), 72 us (weights) at B = 4096).
constexpr int DMC_NB = 64;

// DMC drift-diffusion extras (DMC/drift_diffusion.py:15-22):
// grad != nullptr: out[0] = sum over all coordinates of the proposed configuration
//   x + limdrift(grad) tau + sqrt(tau) gauss1 (the `changed_configuration` of :66);
// grad == nullptr: out[1] = sum of x (after acceptance), out[2] = tdamp = out[1] / out[0].
// k_dmc_sum_part: part[blk] = this block's share; k_dmc_sum_fin: the sum of part[0..DMC_NB) in order.
template <typename T>
__global__ __launch_bounds__(256) void k_dmc_sum_part(const T* __restrict__ x, const T* __restrict__ grad,
                                                      const T* __restrict__ g1, const double* __restrict__ taueff,
                                                      double tstep_d, int n, double* __restrict__ part) {
  __shared__ double red[256];
  const T tstep = (T)tstep_d;
  const T sq = sqrt(tstep);
  const T te = grad ? (T)taueff[0] : T(0);
  double acc = 0.0;
  for (int i = blockIdx.x * 256 + threadIdx.x; i < n; i += 256 * DMC_NB) {
    T v = x[i];
    if (grad) v = v + (grad[i] * te * tstep + sq * g1[i]);
    acc += (double)v;
  }
  red[threadIdx.x] = acc;
  __syncthreads();
  block_tree_sum<256>(red);
  if (threadIdx.x == 0) part[blockIdx.x] = red[0];
}
__global__ void k_dmc_sum_fin(const double* __restrict__ part, int proposed, double* out) {
  if (threadIdx.x != 0) return;
  double a = 0.0;
  for (int b = 0; b < DMC_NB; ++b) a += part[b];
  if (proposed) {
    out[0] = a;
  } else {
    out[1] = a;
    out[2] = a / out[0];
  }
}

// out[i] = grad[i] * taueff (limdrift, VMCmcstep.py:11-14 / drift_diffusion.py:9-12)
template <typename T>
__global__ __launch_bounds__(256) void k_scale_grad(const T* __restrict__ g, const double* __restrict__ taueff, int n,
                                                    T* __restrict__ out) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) out[i] = g[i] * (T)taueff[0];
}

// DMC energy cut minima (S_matrix.py:21-22): jnp.min over the stacked [|e_est - eloc|, branchcut]
// array is ONE minimum over every walker (of every device: the reference stacks the pmapped
// [ndev, B] arrays) and the cut.  k_dmc_cut_part: part[2 blk], part[2 blk + 1] = this block's
// minima for eloc_old / eloc_new (the branch cut included); a minimum is exact in any order, so
// the consumers take the min over the DMC_NB block results directly.
// eest_b (nullable): per-walker e_est (the first block, main_dmc.py:115-116), else e_est.
template <typename T>
__global__ __launch_bounds__(256) void k_dmc_cut_part(int B, const T* __restrict__ eold, const T* __restrict__ enew,
                                                      const T* __restrict__ eest_b, double e_est, double branchcut,
                                                      double* __restrict__ part) {
  __shared__ double mo[256], mn[256];
  double a = branchcut, b = branchcut;
  for (int i = blockIdx.x * 256 + threadIdx.x; i < B; i += 256 * DMC_NB) {
    const double ee = eest_b ? (double)eest_b[i] : e_est;
    a = fmin(a, fabs(ee - (double)eold[i]));
    b = fmin(b, fabs(ee - (double)enew[i]));
  }
  mo[threadIdx.x] = a;
  mn[threadIdx.x] = b;
  __syncthreads();
  block_tree_min2<256>(mo, mn);
  if (threadIdx.x == 0) {
    part[2 * blockIdx.x] = mo[0];
    part[2 * blockIdx.x + 1] = mn[0];
  }
}
__global__ void k_dmc_cut_fin(const double* __restrict__ part, double* __restrict__ out) {
  if (threadIdx.x != 0) return;
  double a = part[0], b = part[1];
  for (int k = 1; k < DMC_NB; ++k) {
    a = fmin(a, part[2 * k]);
    b = fmin(b, part[2 * k + 1]);
  }
  out[0] = a;
  out[1] = b;
}

// DMC weights (DMC/S_matrix.py:4-24, dmc.py:80-92), one thread per walker:
//   S = e_trial - e_est + e_cut / (1 + (v2 tau / N)^2), v2 = |grad_eff|^2 per walker,
//   e_cut = cut * sign(e_est - eloc_b), cut = the global minimum above: the caller's all-reduced
//   cuts[2] (multi-device run), or the min over k_dmc_cut_part's block minima of this batch (cpart),
//   w *= exp(tau tdamp (S_new + S_old) / 2).
// etr_b / eest_b (nullable): per-walker e_trial / e_est of the first DMC block.
template <typename T>
__global__ __launch_bounds__(256) void k_dmc_weights(int B, int N, const T* __restrict__ eold, const T* __restrict__ enew,
                                                     const T* __restrict__ gold, const T* __restrict__ gnew,
                                                     const double* __restrict__ tdamp, double tau,
                                                     const T* __restrict__ etr_b, const T* __restrict__ eest_b,
                                                     double e_trial, double e_est, const double* __restrict__ cuts,
                                                     const double* __restrict__ cpart, T* __restrict__ w) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= B) return;
  double cut_o, cut_n;
  if (cuts) {
    cut_o = cuts[0];
    cut_n = cuts[1];
  } else {
    cut_o = cpart[0];
    cut_n = cpart[1];
    for (int k = 1; k < DMC_NB; ++k) {
      cut_o = fmin(cut_o, cpart[2 * k]);
      cut_n = fmin(cut_n, cpart[2 * k + 1]);
    }
  }
  const double td = tdamp[2];   // [sum proposed, sum new, tdamp] of aiqmc_dmc_drift_diffusion
  double vo = 0.0, vn = 0.0;
  for (int k = 0; k < 3 * N; ++k) {
    const double x = (double)gold[(size_t)i * 3 * N + k], y = (double)gnew[(size_t)i * 3 * N + k];
    vo += x * x;
    vn += y * y;
  }
  const double ee = eest_b ? (double)eest_b[i] : e_est;
  const double et = etr_b ? (double)etr_b[i] : e_trial;
  const double co = ee - (double)eold[i], cn = ee - (double)enew[i];
  const double so = et - ee + cut_o * (double)((co > 0) - (co < 0)) / (1.0 + (vo * tau / N) * (vo * tau / N));
  const double sn = et - ee + cut_n * (double)((cn > 0) - (cn < 0)) / (1.0 + (vn * tau / N) * (vn * tau / N));
  w[i] = (T)(exp(tau * td * (0.5 * sn + 0.5 * so)) * (double)w[i]);
}

// Stochastic comb (DMC/branch.py:10-33), one block: cumulative weights in a fixed order, then
// newinds[j] = searchsorted_left(cumsum, (u wtot + j wtot / n) mod wtot); wout[0] = wtot / n.
// The cumulative sum is a blocked scan: thread t sums its contiguous chunk of ceil(n / 1024)
// weights, the 1024 chunk sums are scanned in a fixed tree (Hillis-Steele over LDS), and each
// thread re-walks its chunk from its prefix.  Deterministic; it equals the sequential sum up to
// fp64 rounding.  (A single thread carrying the running sum took 196 us at n = 4096 from global
// memory and 69 us through LDS.)  The searches read an LDS copy when the cumsum fits.
constexpr int COMB_LDS = 4096;
template <typename T>
__global__ __launch_bounds__(1024) void k_dmc_branch(int n, const T* __restrict__ w, double u, double* __restrict__ csum,
                                                     int32_t* __restrict__ newinds, T* __restrict__ wout) {
  __shared__ double sc[1024];
  __shared__ double cl[COMB_LDS];
  const int t = threadIdx.x;
  const int ch = (n + 1023) / 1024;
  const int i0 = t * ch < n ? t * ch : n, i1 = i0 + ch < n ? i0 + ch : n;
  double s = 0.0;
  for (int i = i0; i < i1; ++i) s += (double)w[i];
  sc[t] = s;
  __syncthreads();
  for (int d = 1; d < 1024; d <<= 1) {   // inclusive scan of the chunk sums
    const double v = t >= d ? sc[t - d] : 0.0;
    __syncthreads();
    sc[t] += v;
    __syncthreads();
  }
  double a = t > 0 ? sc[t - 1] : 0.0;
  const bool lds = n <= COMB_LDS;
  for (int i = i0; i < i1; ++i) {
    a += (double)w[i];
    if (lds) cl[i] = a;
    else csum[i] = a;
  }
  __syncthreads();   // (block-scope fence: the global cumsum of the other threads is visible)
  const double* cp = lds ? cl : csum;
  const double wtot = cp[n - 1];
  for (int j = t; j < n; j += 1024) {
    const double tt = fmod(u * wtot + (double)j * (wtot / (double)n), wtot);
    int lo = 0, hi = n;
    while (lo < hi) {
      const int mid = (lo + hi) >> 1;
      if (cp[mid] < tt) lo = mid + 1;
      else hi = mid;
    }
    newinds[j] = lo;
  }
  if (t == 0) wout[0] = (T)(wtot / (double)n);
}

// ============================================================================ host side

namespace aq_host {

// DMC reduction scratch (2 * DMC_NB doubles), allocated on first use
double* dmc_scratch(aiqmc_ctx* c) {
  (void)c->d_dscr.reserve(2 * DMC_NB * sizeof(double));
  return c->d_dscr.as<double>();
}

// mc_sweep's DMC extras: the sum of the n proposed (g1 given; the sweep's walker gradients and
// first limdrift factor) or moved (g1 == nullptr) coordinates, in block order
void dmc_coord_sum(aiqmc_ctx* c, const void* pos, const void* g1, double tstep, int n, double* dscr, double* dmc,
                   hipStream_t s) {
  by_dtype(c->dtype, [&](auto t) {
    using T = decltype(t);
    if (g1)
      k_dmc_sum_part<T><<<dim3(DMC_NB), dim3(256), 0, s>>>((const T*)pos, c->d_grad.as<T>(), (const T*)g1,
                                                           c->d_taueff.as<double>(), tstep, n, dscr);
    else
      k_dmc_sum_part<T><<<dim3(DMC_NB), dim3(256), 0, s>>>((const T*)pos, nullptr, nullptr, nullptr, tstep, n, dscr);
  });
  k_dmc_sum_fin<<<dim3(1), dim3(64), 0, s>>>(dscr, g1 ? 1 : 0, dmc);
}

}  // namespace aq_host

// k_tmove<T>'s static LDS bytes (the pair-radial table), asked of the runtime once per T
template <typename T>
static hipError_t tmove_static_lds(size_t* bytes) {
  static hipFuncAttributes fa;
  static const hipError_t e = hipFuncGetAttributes(&fa, (const void*)&k_tmove<T>);
  *bytes = fa.sharedSizeBytes;
  return e;
}

// ============================================================================ C-ABI

extern "C" {

int aiqmc_dmc_tmoves(aiqmc_ctx* c, void* pos, int32_t B, double tstep, int32_t rng_mode, const void* rot,
                     const void* u_sel, const void* u_acc, uint64_t seed, uint64_t offset, void* acceptance,
                     void* stream) {
  AIQMC_CHECK(c, pos, B);
  if (!c->ecp_set) return fail(AIQMC_ESTATE, "aiqmc_set_ecp has not been called");
  if (int rc = check_sampling(&tstep, rng_mode, B, rot && u_sel && u_acc, "rot, u_sel and u_acc")) return rc;
  AIQMC_BEGIN(c, B, ops);
  hipStream_t s = (hipStream_t)stream;
  if (c->ecp_nl_zero) {   // no T-move amplitude: nothing moves, acceptance exactly 1 (k_tmove_none)
    if (acceptance) {
      const int n = B * c->N;
      by_dtype(c->dtype, [&](auto t) {
        k_tmove_none<decltype(t)><<<blocks(n, 256), dim3(256), 0, s>>>((decltype(t)*)acceptance, n);
      });
      HIPCHK(hipGetLastError());
    }
    return AIQMC_OK;
  }
  int rc = ensure_ecp_ws(c, B, ops);
  if (rc) return rc;
  HIPCHK(c->d_tm_scr.reserve((size_t)B * c->N * c->A * ECP_NQ * 4 * sizeof(double)));
  EcpArgs ea;
  rc = ecp_quadrature(c, ops, pos, B, rng_mode, rot, seed, offset, nullptr, nullptr, ea, s);
  if (rc) return rc;
  ea.tstep = tstep;
  ea.usel = rng_mode == AIQMC_RNG_HOST ? u_sel : nullptr;
  ea.uacc = rng_mode == AIQMC_RNG_HOST ? u_acc : nullptr;
  ea.acc = acceptance;
  ea.pos_out = pos;
  ea.scr = c->d_tm_scr.as<double>();
  // every electron's cdf row in LDS for the searches (<= 40 KB for the built shapes) when it fits
  // beside k_tmove's static LDS (the pair-radial table) in 64 KB; else the per-probe fallback
  const size_t cdf_bytes = (size_t)c->N * (c->A * ECP_NQ + 1) * 2 * sizeof(double);
  return by_dtype(c->dtype, [&](auto t) {
    using T = decltype(t);
    size_t static_lds = 0;
    HIPCHK(tmove_static_lds<T>(&static_lds));
    ea.cdf_lds = cdf_bytes + static_lds <= 65536 ? 1 : 0;
    k_tmove<T><<<dim3(B), dim3(64), ea.cdf_lds ? (unsigned)cdf_bytes : 0u, s>>>(ea);
    HIPCHK(hipGetLastError());
    return (int)AIQMC_OK;
  });
}

int aiqmc_dmc_drift_diffusion(aiqmc_ctx* c, void* pos, int32_t B, double tstep, int32_t rng_mode, const void* gauss1,
                              const void* gauss2, const void* u, uint64_t seed, uint64_t offset, void* grad_eff_old,
                              void* grad_new_eff, double* tdamp, void* stream) {
  AIQMC_CHECK(c, pos, B);
  if (int rc = check_sampling(&tstep, rng_mode, B, gauss1 && gauss2 && u, "gauss1, gauss2 and u")) return rc;
  AIQMC_BEGIN(c, B, ops);
  if (!grad_eff_old || !grad_new_eff || !tdamp) return fail(AIQMC_EINVAL, "null output");
  int rc = ensure_ws(c, B, ops);
  if (rc) return rc;
  if (!c->reuse) {
    rc = ensure_wcp(c, (int64_t)B * c->N, ops);
    if (rc) return rc;
  }
  hipStream_t s = (hipStream_t)stream;
  double* const taueff = c->d_taueff.as<double>();
  const int n = B * 3 * c->N;
  SweepArgs sw;
  sw.pos = pos;
  sw.B = B;
  sw.tstep = tstep;
  sw.rng_mode = rng_mode;
  sw.gauss1 = gauss1;
  sw.gauss2 = gauss2;
  sw.u = u;
  sw.seed = seed;
  sw.step = offset;
  sw.dmc = tdamp;
  rc = mc_sweep(c, ops, s, sw);
  if (rc) return rc;
  // grad_new_eff_s: the gradients at the moved walkers (:103-104)
  WalkerCall w = launch_args(c, Launch::WalkerGrad, pos, B, nullptr, &c->d_wc);
  w.ka.grad = grad_new_eff;
  w.ka.sumsq = c->d_sq.as();
  by_dtype(c->dtype, [&](auto t) {
    using T = decltype(t);
    // grad_eff_old: limdrift of the walker gradients of this sweep (drift_diffusion.py:60-61)
    k_scale_grad<T><<<blocks(n, 256), dim3(256), 0, s>>>(c->d_grad.as<T>(), taueff, n, (T*)grad_eff_old);
    ops.walker(c->dtype, w, B, s);
    // ... and their limdrift
    launch_taueff(c->dtype, c->d_sq.as(), B, tstep, taueff + 1, s);
    k_scale_grad<T><<<blocks(n, 256), dim3(256), 0, s>>>((const T*)grad_new_eff, taueff + 1, n, (T*)grad_new_eff);
  });
  HIPCHK(hipGetLastError());
  return AIQMC_OK;
}

// k_dmc_cut_part over this batch: the block minima [2 * DMC_NB] in d
static void cut_minima_part(int dtype, int B, const void* eloc_old, const void* eloc_new, const void* e_est_b,
                            double e_est, double branchcut, double* d, hipStream_t s) {
  by_dtype(dtype, [&](auto t) {
    using T = decltype(t);
    k_dmc_cut_part<T><<<dim3(DMC_NB), dim3(256), 0, s>>>(B, (const T*)eloc_old, (const T*)eloc_new, (const T*)e_est_b,
                                                         e_est, branchcut, d);
  });
}

int aiqmc_dmc_weights_ex(aiqmc_ctx* c, int32_t B, const void* eloc_old, const void* eloc_new,
                         const void* grad_eff_old, const void* grad_new_eff, const double* tdamp, double tstep,
                         const void* e_trial_b, const void* e_est_b, double e_trial, double e_est, double branchcut,
                         const double* cut_minima, void* weights_inout, void* stream) {
  if (!c) return fail(AIQMC_EINVAL, "null context");
  if (B < 0) return fail(AIQMC_EINVAL, "negative batch");
  if (B == 0) return AIQMC_OK;
  if (!eloc_old || !eloc_new || !grad_eff_old || !grad_new_eff || !tdamp || !weights_inout)
    return fail(AIQMC_EINVAL, "null argument");
  HIPCHK(hipSetDevice(c->device));
  hipStream_t s = (hipStream_t)stream;
  const double* cpart = nullptr;
  if (!cut_minima) {   // this batch's minima (single device)
    double* d = dmc_scratch(c);
    if (!d) return fail(AIQMC_EHIP, "hipMalloc: DMC scratch");
    cut_minima_part(c->dtype, B, eloc_old, eloc_new, e_est_b, e_est, branchcut, d, s);
    cpart = d;
  }
  by_dtype(c->dtype, [&](auto t) {
    using T = decltype(t);
    k_dmc_weights<T><<<blocks(B, 256), dim3(256), 0, s>>>(
        B, c->N, (const T*)eloc_old, (const T*)eloc_new, (const T*)grad_eff_old, (const T*)grad_new_eff, tdamp, tstep,
        (const T*)e_trial_b, (const T*)e_est_b, e_trial, e_est, cut_minima, cpart, (T*)weights_inout);
  });
  HIPCHK(hipGetLastError());
  return AIQMC_OK;
}

int aiqmc_dmc_weights(aiqmc_ctx* c, int32_t B, const void* eloc_old, const void* eloc_new, const void* grad_eff_old,
                      const void* grad_new_eff, const double* tdamp, double tstep, double e_trial, double e_est,
                      double branchcut, void* weights_inout, void* stream) {
  return aiqmc_dmc_weights_ex(c, B, eloc_old, eloc_new, grad_eff_old, grad_new_eff, tdamp, tstep, nullptr, nullptr,
                              e_trial, e_est, branchcut, nullptr, weights_inout, stream);
}

int aiqmc_dmc_cut_minima(aiqmc_ctx* c, int32_t B, const void* eloc_old, const void* eloc_new, const void* e_est_b,
                         double e_est, double branchcut, double* out, void* stream) {
  if (!c) return fail(AIQMC_EINVAL, "null context");
  if (B < 0) return fail(AIQMC_EINVAL, "negative batch");
  if (!out || (B > 0 && (!eloc_old || !eloc_new))) return fail(AIQMC_EINVAL, "null argument");
  HIPCHK(hipSetDevice(c->device));
  hipStream_t s = (hipStream_t)stream;
  double* d = dmc_scratch(c);
  if (!d) return fail(AIQMC_EHIP, "hipMalloc: DMC scratch");
  cut_minima_part(c->dtype, B, eloc_old, eloc_new, e_est_b, e_est, branchcut, d, s);
  k_dmc_cut_fin<<<dim3(1), dim3(64), 0, s>>>(d, out);
  HIPCHK(hipGetLastError());
  return AIQMC_OK;
}

int aiqmc_dmc_branch(aiqmc_ctx* c, int32_t B, const void* weights, double u, int32_t* newinds, void* weight_out,
                     void* stream) {
  if (!c) return fail(AIQMC_EINVAL, "null context");
  if (B <= 0) return fail(AIQMC_EINVAL, "empty batch");
  if (!weights || !newinds || !weight_out) return fail(AIQMC_EINVAL, "null argument");
  if (!(u >= 0.0 && u < 1.0)) return fail(AIQMC_EINVAL, "u must be in [0, 1)");
  HIPCHK(hipSetDevice(c->device));
  double* csum = nullptr;
  HIPCHK(hipMallocAsync((void**)&csum, (size_t)B * sizeof(double), (hipStream_t)stream));
  hipStream_t s = (hipStream_t)stream;
  by_dtype(c->dtype, [&](auto t) {
    using T = decltype(t);
    k_dmc_branch<T><<<dim3(1), dim3(1024), 0, s>>>(B, (const T*)weights, u, csum, newinds, (T*)weight_out);
  });
  HIPCHK(hipFreeAsync(csum, s));
  HIPCHK(hipGetLastError());
  return AIQMC_OK;
}

}  // extern "C"
