// host_shared.h -- the host helpers that more than one context translation unit calls (the units
// that include it are listed in ctx.h).  Each is defined in the unit named beside it; none is
// exported (hidden visibility: the library's dynamic symbol table is the C-ABI of include/aiqmc.h).
#pragma once
#include "api_util.h"
#include "ecp_args.h"

namespace aq_host {
#pragma GCC visibility push(hidden)

// What one sweep is given (mc_sweep); a caller sets the fields it uses by name.
struct SweepArgs {
  void* pos = nullptr;   // [B][3N] walkers, moved in place
  int B = 0;
  double tstep = 0.0;
  int rng_mode = AIQMC_RNG_PHILOX;
  const void *gauss1 = nullptr, *gauss2 = nullptr, *u = nullptr;   // AIQMC_RNG_HOST: the caller's draws [nsteps][...]
  int st = 0;                    // ... and the index of this sweep in them
  uint64_t seed = 0, step = 0;   // Philox key and counter of this sweep
  int32_t* accept_out = nullptr; // [B] accepted moves (optional)
  // DMC drift-diffusion extras (device doubles [3], DMC/drift_diffusion.py:15-22): dmc[0] = sum of the
  // proposed coordinates, dmc[2] = tdamp = sum(x_new) / dmc[0]; such a sweep is never deferred or fused
  double* dmc = nullptr;
  // defer: leave the acceptance in *pending for the next sweep's walker launch (one launch and one
  // inter-kernel gap fewer per sweep; same arithmetic, accept_one); a set *pending is applied first
  aq::AccArgs* pending = nullptr;
  bool defer = false;
  // fp32 mc_step: this sweep's zeroed pair of fused limdrift accumulators (kargs.h
  // TACC_STRIDE; the two k_taueff launches are then skipped), or its k_taueff_part partial sums
  unsigned long long* tacc = nullptr;
  unsigned long long* tpart = nullptr;
  bool pvok = false;             // the walker cache holds the previous sweep's pivot order
  unsigned long long* zero_next = nullptr;   // k_accept: accumulator words to zero for the next call
  int nzero = 0;
};

// ---- aiqmc.hip
int ensure_ws(aiqmc_ctx* c, int B, const ShapeOps& ops);
int ensure_wcp(aiqmc_ctx* c, int64_t n, const ShapeOps& ops);
int ensure_ecp_ws(aiqmc_ctx* c, int B, const ShapeOps& ops);
int check_sampling(const double* tstep, int rng_mode, int B, bool have, const char* what);
int mc_sweep(aiqmc_ctx* c, const ShapeOps& ops, hipStream_t s, const SweepArgs& sw);
// the batch condition of mc_sweep's two-wave walker launch (LaunchOpts::split) for B walkers
bool sweep_split(const aiqmc_ctx* c, int B);
int ecp_quadrature(aiqmc_ctx* c, const ShapeOps& ops, const void* pos, int B, int rng_mode, const void* rot,
                   uint64_t seed, uint64_t offset, void* logabs_q, void* phase_q, aq::EcpArgs& ea, hipStream_t s);
// k_taueff<dtype> (one workgroup of 1024) over the n sums of squares x: the limdrift factor to *out
void launch_taueff(int dtype, const void* x, int n, double tstep, double* out, hipStream_t s);
// k_taueff_part (TPART workgroups of 256) over the n float sums of squares x: one kind's [4][TPART]
void launch_taueff_part(const float* x, int n, unsigned long long* part, hipStream_t s);

// ---- dmc.hip
double* dmc_scratch(aiqmc_ctx* c);
// dscr: dmc_scratch; the sum of the n proposed coordinates (g1 given) to dmc[0], or of the moved
// ones (g1 == nullptr) to dmc[1] and tdamp to dmc[2], in block order
void dmc_coord_sum(aiqmc_ctx* c, const void* pos, const void* g1, double tstep, int n, double* dscr, double* dmc,
                   hipStream_t s);

// ---- observables.hip
// the d_obs_* workspace of one chunk of nconf configurations (x, log|psi|, phase, walker cache)
int ensure_obs(aiqmc_ctx* c, int nconf, const ShapeOps& ops);
// the value launch over the nconf configurations in d_obs_x: log|psi| to d_obs_lp, the phase to
// d_obs_ph, with aiqmc_logpsi's arguments (the same kernels and bits)
void obs_values(aiqmc_ctx* c, const ShapeOps& ops, int nconf, hipStream_t s);

#pragma GCC visibility pop
}  // namespace aq_host
