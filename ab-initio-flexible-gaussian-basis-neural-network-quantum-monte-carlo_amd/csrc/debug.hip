// debug.hip -- profiling (aiqmc_profile_*) and the diagnostics entry points (aiqmc_debug_*) of a
// context: switches of the launch paths, forward-mode checks, reads of internal buffers.  Kernels
// defined here:
//   k_tacc_feed, k_taueff_read          aiqmc_debug_limdrift_factor
// (aiqmc_debug_set_obs_chunk is in observables.hip, beside what it sets.)
#include <hip/hip_runtime.h>

#include <cstdint>
#include <string>

#include "aiqmc.h"
#include "host_shared.h"
#include "limdrift.h"

using namespace aq;
using namespace aq_host;

// aiqmc_debug_limdrift_factor: the fused path's per-configuration accumulation (tacc_add, one
// thread per configuration instead of lane 0 of its wave) and the consumers' read (taueff_wave).
__global__ __launch_bounds__(256) void k_tacc_feed(const float* __restrict__ x, int n, unsigned long long* acc) {
  const int i = blockIdx.x * 256 + (int)threadIdx.x;
  if (i < n) tacc_add(acc, 0, i, (double)x[i]);
}
__global__ __launch_bounds__(64) void k_taueff_read(const unsigned long long* acc, const unsigned long long* part,
                                                    double tstep, double* out) {
  const float te = taueff_wave<float>(nullptr, acc, 0, tstep, part);
  if (threadIdx.x == 0) *out = (double)te;
}

extern "C" {

int aiqmc_debug_local_energy_forward(aiqmc_ctx* c, const void* pos, int32_t B, void* e_l, void* logabs, void* grad,
                                     void* stream) {
  AIQMC_ENTER(c, pos, B, ops);
  if (!e_l) return fail(AIQMC_EINVAL, "null e_l");
  WalkerCall w = launch_args(c, Launch::LapForward, pos, B, logabs);
  w.ka.el = e_l;
  w.ka.grad = grad;
  ops.walker(c->dtype, w, B, (hipStream_t)stream);
  HIPCHK(hipGetLastError());
  return AIQMC_OK;
}

int aiqmc_profile_enable(aiqmc_ctx* c, int32_t on) {
  if (!c) return fail(AIQMC_EINVAL, "null context");
  c->prof = on != 0;
  return AIQMC_OK;
}

int aiqmc_profile_read(aiqmc_ctx* c, int32_t slot, double* total_ms, int64_t* launches) {
  if (!c || slot < 0 || slot >= AIQMC_PROF_SLOTS || !total_ms || !launches) return fail(AIQMC_EINVAL, "bad argument");
  double tot = 0.0;
  int64_t n = 0;
  for (auto& p : c->ev_used[slot]) {
    HIPCHK(hipEventSynchronize(p.second));
    float ms = 0.f;
    HIPCHK(hipEventElapsedTime(&ms, p.first, p.second));
    tot += ms;
    ++n;
    c->ev_free.push_back(p.first);
    c->ev_free.push_back(p.second);
  }
  c->ev_used[slot].clear();
  *total_ms = tot;
  *launches = n;
  return AIQMC_OK;
}

int aiqmc_debug_logpsi_grad_forward(aiqmc_ctx* c, const void* pos, int32_t B, void* logabs, void* grad,
                                     void* stream) {
  AIQMC_ENTER(c, pos, B, ops);
  if (!grad) return fail(AIQMC_EINVAL, "null grad");
  WalkerCall w = launch_args(c, Launch::GradForward, pos, B, logabs);
  w.ka.grad = grad;
  ops.walker(c->dtype, w, B, (hipStream_t)stream);
  HIPCHK(hipGetLastError());
  return AIQMC_OK;
}

int aiqmc_debug_set_ablate(aiqmc_ctx* c, int32_t mask) {
  if (!c) return fail(AIQMC_EINVAL, "null context");
  c->ablate = mask;
  return AIQMC_OK;
}

int aiqmc_debug_set_lap_waves(aiqmc_ctx* c, int32_t waves) {
  if (!c) return fail(AIQMC_EINVAL, "null context");
  if (waves != 0 && waves != 1 && waves != 2 && waves != 4) return fail(AIQMC_EINVAL, "lap waves must be 0, 1, 2 or 4");
  c->lap_waves = waves;
  return AIQMC_OK;
}

int aiqmc_debug_set_fuse_accept(aiqmc_ctx* c, int32_t on) {
  if (!c) return fail(AIQMC_EINVAL, "null context");
  c->fuse_accept = on != 0;
  return AIQMC_OK;
}

int aiqmc_debug_set_quad_pivoted(aiqmc_ctx* c, int32_t on) {
  if (!c) return fail(AIQMC_EINVAL, "null context");
  c->quad_pivoted = on != 0;
  return AIQMC_OK;
}

int aiqmc_debug_set_packed_walkers(aiqmc_ctx* c, int32_t on) {
  if (!c) return fail(AIQMC_EINVAL, "null context");
  c->packed_walkers = on != 0;
  return AIQMC_OK;
}

int aiqmc_debug_launch_lds(int32_t nelectrons, int32_t natoms, int32_t dtype, int32_t kind, int32_t* bytes,
                           int32_t* waves) {
  ShapeOps ops{};
  if (!aiqmc_shape_ops(nelectrons, natoms, &ops)) return fail(AIQMC_EUNSUPPORTED, "no kernel instantiation for this shape");
  if (kind < 0 || kind > 5) return fail(AIQMC_EINVAL, "kind must be one of AIQMC_LDS_*");
  if (!is_dtype(dtype)) return fail(AIQMC_EINVAL, "dtype must be AIQMC_F32 or AIQMC_F64");
  const int d = dtype == AIQMC_F32 ? 0 : 1;
  if (bytes) *bytes = ops.dyn_lds[d][kind];
  if (waves) *waves = ops.wg_waves[d][kind];
  return AIQMC_OK;
}

// The row (launch_route.h Row, 1..8) a walker launch of `kind` (Launch, 0..7) over nconf
// configurations would reach with this context's shape, dtype and current switches; nconf decides
// only the sweep walker's split, by mc_sweep's batch condition.  Launches nothing.
static_assert((int)Launch::WalkerValue == AIQMC_LAUNCH_WALKER_VALUE && (int)Launch::WalkerOrbitals == AIQMC_LAUNCH_WALKER_ORBITALS &&
                  (int)Launch::WalkerGrad == AIQMC_LAUNCH_WALKER_GRAD && (int)Launch::SweepWalker == AIQMC_LAUNCH_SWEEP_WALKER &&
                  (int)Launch::Proposal == AIQMC_LAUNCH_PROPOSAL && (int)Launch::Quadrature == AIQMC_LAUNCH_QUADRATURE &&
                  (int)Launch::LapForward == AIQMC_LAUNCH_LAP_FORWARD && (int)Launch::GradForward == AIQMC_LAUNCH_GRAD_FORWARD,
              "AIQMC_LAUNCH_* of aiqmc.h are aq::Launch");
int aiqmc_debug_launch_row(aiqmc_ctx* c, int32_t kind, int32_t nconf, int32_t* row) {
  if (!c || !row) return fail(AIQMC_EINVAL, "null argument");
  if (kind < 0 || kind >= LAUNCH_KINDS) return fail(AIQMC_EINVAL, "kind must be one of AIQMC_LAUNCH_*");
  if (nconf < 0) return fail(AIQMC_EINVAL, "negative nconf");
  LaunchOpts o = launch_opts(c);
  o.split = sweep_split(c, nconf);
  *row = (int32_t)route((Launch)kind, c->dtype == AIQMC_F32, c->N, o);
  return AIQMC_OK;
}

int aiqmc_debug_set_walker_pivots(aiqmc_ctx* c, int32_t reuse) {
  if (!c) return fail(AIQMC_EINVAL, "null context");
  c->walker_fixed_gj = reuse != 0;
  return AIQMC_OK;
}

int aiqmc_debug_set_fuse_reduce(aiqmc_ctx* c, int32_t on) {
  if (!c) return fail(AIQMC_EINVAL, "null context");
  if (on < 0 || on > 3) return fail(AIQMC_EINVAL, "fuse_reduce must be 0, 1, 2 or 3");
  c->fuse_reduce = on == 3 ? 0 : on;
  c->wide_reduce = on == 3 ? 0 : 1;
  return AIQMC_OK;
}


int aiqmc_debug_limdrift_factor(aiqmc_ctx* c, const void* sumsq, int32_t n, double tstep, int32_t mode, double* out,
                                void* stream) {
  if (!c) return fail(AIQMC_EINVAL, "null context");
  if (!sumsq || !out || n <= 0) return fail(AIQMC_EINVAL, "limdrift_factor: null buffer or n <= 0");
  if (n >= TACC_MAX_CONF && mode != 2) return fail(AIQMC_EINVAL, "limdrift_factor: n >= 2^24 needs mode 2");
  if (mode < 0 || mode > 2) return fail(AIQMC_EINVAL, "limdrift_factor: mode must be 0, 1 or 2");
  HIPCHK(hipSetDevice(c->device));
  hipStream_t s = (hipStream_t)stream;
  const size_t words = (size_t)TACC_STRIDE + TPART_KIND + 1;   // acc | part | out (as a double)
  DevBuf scratch;   // freed on every return
  HIPCHK(scratch.reserve(words * sizeof(unsigned long long)));
  unsigned long long* d = scratch.as<unsigned long long>();
  unsigned long long* acc = d;
  unsigned long long* part = d + TACC_STRIDE;
  double* dout = (double*)(d + TACC_STRIDE + TPART_KIND);
  int rc = AIQMC_OK;
  if (hipMemsetAsync(d, 0, words * sizeof(unsigned long long), s) != hipSuccess) rc = fail(AIQMC_EHIP, "memset");
  if (!rc) {
    const float* x = (const float*)sumsq;   // a float entry point: the fp32 sweep's three reductions
    if (mode == 0) {
      k_tacc_feed<<<dim3((n + 255) / 256), dim3(256), 0, s>>>(x, n, acc);
      k_taueff_read<<<dim3(1), dim3(64), 0, s>>>(acc, nullptr, tstep, dout);
    } else if (mode == 1) {
      launch_taueff_part(x, n, part, s);
      k_taueff_read<<<dim3(1), dim3(64), 0, s>>>(nullptr, part, tstep, dout);
    } else {
      launch_taueff(AIQMC_F32, x, n, tstep, dout, s);
    }
    if (hipGetLastError() != hipSuccess || hipMemcpyAsync(out, dout, sizeof(double), hipMemcpyDeviceToHost, s) != hipSuccess ||
        hipStreamSynchronize(s) != hipSuccess)
      rc = fail(AIQMC_EHIP, "limdrift_factor: launch or copy");
  }
  return rc;
}

int aiqmc_debug_set_proposal_reuse(aiqmc_ctx* c, int32_t on) {
  if (!c) return fail(AIQMC_EINVAL, "null context");
  c->reuse = on != 0;
  return AIQMC_OK;
}

int aiqmc_debug_read_draws(aiqmc_ctx* c, int32_t which, void* dst, int64_t count, void* stream) {
  if (!c) return fail(AIQMC_EINVAL, "null context");
  if (!dst || count < 0) return fail(AIQMC_EINVAL, "read_draws: null destination or negative count");
  const DevBuf* const bufs[4] = {&c->d_g1, &c->d_g2, &c->d_u, &c->d_ecp_rot};
  if (which < 0 || which > 3) return fail(AIQMC_EINVAL, "read_draws: which must be 0 (gauss1), 1 (gauss2), 2 (u) or 3 (rotations)");
  const DevBuf& src = *bufs[which];
  // (the quotient form cannot overflow; an unallocated buffer has capacity 0)
  if ((uint64_t)count > src.capacity() / elem_size(c)) return fail(AIQMC_EINVAL, "read_draws: count exceeds the buffer");
  if (count == 0) return AIQMC_OK;
  HIPCHK(hipSetDevice(c->device));
  HIPCHK(hipMemcpyAsync(dst, src.as(), (size_t)count * elem_size(c), hipMemcpyDeviceToDevice, (hipStream_t)stream));
  return AIQMC_OK;
}

int aiqmc_debug_phase_cycles(aiqmc_ctx* c, uint64_t* out32) {
  if (!c || !out32) return fail(AIQMC_EINVAL, "null argument");
  ShapeOps ops;
  aiqmc_shape_ops(c->N, c->A, &ops);
  HIPCHK(hipSetDevice(c->device));
  HIPCHK(hipDeviceSynchronize());
  ops.phase_read((unsigned long long*)out32);
  return AIQMC_OK;
}

}  // extern "C"
