/*
 * aiqmc.h -- C-ABI of the MI355X-native AIQMC VMC inner loop.
 *
 * The reference (Yongda1/AIQMC, AIQMCrelease3) is pure Python/JAX and has no
 * FFI; the entry points below replace the JAX-traced hot path one for one:
 *
 *   aiqmc_logpsi        <- network.apply / signed_network, vmapped
 *                          (AIQMCrelease3/wavefunction_Ynlm/nn.py:545-551,
 *                           network_blocks.py:161-206)
 *   aiqmc_logpsi_grad   <- vmap(jax.grad(logabs_f))   (VMC/VMCmcstep.py:41-53)
 *   aiqmc_local_energy  <- vmap(hamiltonian.local_energy(...)) with
 *                          complex_output=False (Energy/hamiltonian.py:236-260,
 *                          kinetic part :77-132)
 *   aiqmc_mc_step       <- VMCmcstep.main_monte_carlo(...) -> mc_step
 *                          (VMC/VMCmcstep.py:121-140, walkers_update :28-111)
 *   aiqmc_set_params    <- the params pytree passed to all of the above;
 *                          `flat` is its jax.tree_util.tree_flatten order
 *                          (dict keys sorted, lists in order, C-order leaves),
 *                          i.e. jax.flatten_util.ravel_pytree(params)[0].
 *
 * Conventions: every array pointer passed to a compute entry point is a DEVICE
 * pointer (HIP) of the context's dtype (float for AIQMC_F32, double for
 * AIQMC_F64); `stream` is a hipStream_t (NULL = default stream).  Host
 * pointers appear only in aiqmc_cfg and aiqmc_set_params.  Functions return
 * 0 on success and a negative AIQMC_E* code on failure; the message is in
 * aiqmc_last_error() (thread-local).  No C++ exception crosses the ABI.
 * A context is bound to one device and is not re-entrant.
 */
#ifndef AIQMC_H_
#define AIQMC_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define AIQMC_F32 0
#define AIQMC_F64 1

#define AIQMC_OK 0
#define AIQMC_EINVAL (-1)
#define AIQMC_EUNSUPPORTED (-2)
#define AIQMC_EHIP (-3)
#define AIQMC_ESTATE (-4)

/* rng_mode of aiqmc_mc_step */
#define AIQMC_RNG_HOST 0    /* gauss1/gauss2/u supplied by the caller (parity mode) */
#define AIQMC_RNG_PHILOX 1  /* drawn on device from (seed, offset)                 */

typedef struct aiqmc_ctx aiqmc_ctx;

/* System + network configuration (make_ai_net arguments, nn.py:511-526). */
typedef struct aiqmc_cfg {
  int32_t nelectrons;            /* N  (2 <= N <= 16)                          */
  int32_t natoms;                /* A  ((N, A) in aiqmc_supported_shapes():   */
                                 /*     every N with A <= 3, and (10,4),(10,5)) */
  int32_t nspins[2];             /* (n_up, n_down); both > 0                   */
  int32_t dtype;                 /* AIQMC_F32 | AIQMC_F64                      */
  int32_t device;                /* HIP device ordinal                         */
  const double* atoms;           /* [A*3] bohr                                 */
  const double* charges;         /* [A]   (Jastrow e-n + potential charges)    */
  const int32_t* spin_up_indices;   /* [n_up]   spin_indices.py:38-45; with    */
  const int32_t* spin_down_indices; /* [n_down] a permutation of 0..N-1        */
  const int32_t* parallel_indices;  /* [2*n_parallel] row-major (2,n_par)      */
  int32_t n_parallel;               /* spin_indices.py:5-19                    */
  const int32_t* antiparallel_indices; /* [2*n_antiparallel]                   */
  int32_t n_antiparallel;              /* == n_up * n_down                     */
  int32_t hidden_dims[3][2];     /* must be ((4,4),(4,4),(4,4)) (nn.py:525)   */
  int32_t hidden_dims_ynlm[3];   /* must be (6,6,6)             (nn.py:526)   */
} aiqmc_cfg;

int aiqmc_create(const aiqmc_cfg* cfg, aiqmc_ctx** out);
int aiqmc_destroy(aiqmc_ctx* ctx);

/* Number of doubles aiqmc_set_params expects (2381 for N2 with defaults). */
int64_t aiqmc_param_count(const aiqmc_ctx* ctx);

/* flat: HOST pointer, `n` doubles in tree_flatten order. Synchronous upload. */
int aiqmc_set_params(aiqmc_ctx* ctx, const double* flat, int64_t n, void* stream);

/* flat: DEVICE pointer (this context's device), `n` doubles in tree_flatten order, repacked into
 * the kernel layout on `stream` (stream-ordered, no host synchronisation): the parameters of an
 * optimiser step that stays on the device (the reference's params are device arrays updated by
 * optax / kfac inside pmap, adam.py:49-59).  The kernel layout equals aiqmc_set_params' bitwise. */
int aiqmc_set_params_device(aiqmc_ctx* ctx, const double* flat, int64_t n, void* stream);

/* pos[B*3N] -> logabs[B], phase[B] (phase may be NULL). */
int aiqmc_logpsi(aiqmc_ctx* ctx, const void* pos, int32_t B, void* logabs, void* phase,
                 void* stream);

/* pos[B*3N] -> logabs[B] (may be NULL), grad[B*3N] = d log|psi| / d pos. */
int aiqmc_logpsi_grad(aiqmc_ctx* ctx, const void* pos, int32_t B, void* logabs, void* grad,
                      void* stream);

/* pos[B*3N] -> e_l[B]; logabs[B] and grad[B*3N] optional (NULL to skip). */
int aiqmc_local_energy(aiqmc_ctx* ctx, const void* pos, int32_t B, void* e_l, void* logabs,
                       void* grad, void* stream);

/* complex_output=True local energy (replaces Energy/hamiltonian.py:100-131 with complex_output
 * True, i.e. local_kinetic_energy's phase branch :110-130, + the potential :236-260):
 * pos[B*3N] -> e_re[B], e_im[B] with
 *   KE = -1/2 [lap log|psi| + i lap theta] - 1/2 |grad log|psi||^2 + 1/2 |grad theta|^2
 *        - i grad log|psi| . grad theta,   theta = arg psi,
 * E_L = V + KE.  Two local-energy launch pairs (log|psi| and theta) and one combining launch. */
int aiqmc_local_energy_complex(aiqmc_ctx* ctx, const void* pos, int32_t B, void* e_re, void* e_im,
                               void* stream);

/* nsteps drift-diffusion Metropolis steps on pos_inout[B*3N] (in place; the
 * donate_argnums=1 analogue).  B is the per-device batch: limdrift's v2 is
 * summed over exactly these B walkers (VMCmcstep.py:12).
 * AIQMC_RNG_HOST: gauss1[nsteps*B*3N] and gauss2[nsteps*B*N*3] standard
 * normals (gauss2 = the electron-diagonal blocks of the reference's
 * [B,N,3N] draw, the only entries it reads, VMCmcstep.py:87-94) and
 * u[nsteps*B*N] uniforms in [0,1).  AIQMC_RNG_PHILOX: the three may be NULL;
 * draws come from Philox4x32-10 keyed by seed, counter offset+step.
 * accept_out (optional, int32[B]) accumulates accepted single-electron moves. */
int aiqmc_mc_step(aiqmc_ctx* ctx, void* pos_inout, int32_t B, int32_t nsteps, double tstep,
                  int32_t rng_mode, const void* gauss1, const void* gauss2, const void* u,
                  uint64_t seed, uint64_t offset, int32_t* accept_out, void* stream);

/* Parameter gradient of log|psi| (the psi_tangent of the energy-gradient custom JVP,
 * Loss/loss.py:242-265, differentiated wrt params as jax.value_and_grad does in
 * Optimizer/adam.py:51-54).  Output in the canonical tree_flatten order of
 * aiqmc_set_params (aiqmc_param_count entries; unused leaves eplion/mu/nu get 0):
 *   weights == NULL: out[B][P] = d log|psi(x_b)| / d theta      (per walker)
 *   weights != NULL: out[P]    = sum_b weights[b] d log|psi(x_b)| / d theta
 * weights/out/logabs are device arrays of the context dtype; logabs[B] optional. */
int aiqmc_logpsi_param_grad(aiqmc_ctx* ctx, const void* pos, int32_t B, const void* weights, void* out,
                            void* logabs, void* stream);

/* Parameter gradient of the phase of psi (arg det A; the Jastrows are real), the imaginary
 * part of psi_tangent when the driver differentiates the complex log
 * log|psi| + i phase (Loss/loss.py:256-265 with complex_output=True, network = log_network
 * of main_pp_adam_muti_GPU.py:119-121).  Same layout and weights convention as
 * aiqmc_logpsi_param_grad; phase[B] (optional) receives the phase at the walkers. */
int aiqmc_phase_param_grad(aiqmc_ctx* ctx, const void* pos, int32_t B, const void* weights, void* out,
                           void* phase, void* stream);

/* Several weighted sums from ONE per-walker gradient pass: out[k][P] = sum_b weights[k][b]
 * d f(x_b) / d theta for k < nw (1..8), f = log|psi| (phase == 0) or the phase (phase != 0);
 * vals[B] (optional) receives f at the walkers.  (The multi-rank energy gradient needs the
 * clipping-weighted sum and the plain sum of d log|psi| together, aiqmc_loss_level.) */
int aiqmc_param_grad_weighted(aiqmc_ctx* ctx, const void* pos, int32_t B, int32_t phase, const void* weights,
                              int32_t nw, void* out, void* vals, void* stream);

/* The orbital matrix of B walkers (Network.orbitals = make_orbitals.apply, nn.py:409-506,553):
 * orbitals[B][N][N][2] (re, im; ctx dtype) = Phi * Yt * exp(J_ee/N) exp(J_ae/N), rows = up
 * electrons then down electrons (spin_up_indices / spin_down_indices order), row r's envelope
 * and y row those of electron r (quirk Q1).  logabs / phase (optional, [B]) as aiqmc_logpsi. */
int aiqmc_orbitals(aiqmc_ctx* ctx, const void* pos, int32_t B, void* orbitals, void* logabs, void* phase,
                   void* stream);

/* DMC drift-diffusion step (DMC/drift_diffusion.py:25-107): one Metropolis sweep
 * exactly as aiqmc_mc_step with nsteps = 1 (same draws, in place), plus
 *   grad_eff_old[B*3N]  limdrift(grad log|psi|) at the walkers before the move (:60-61),
 *   grad_new_eff[B*3N]  limdrift(grad log|psi|) at the moved walkers (:103-104),
 *   tdamp[3]            device doubles: [sum of proposed coordinates, sum of new
 *                       coordinates, tdamp = their ratio] (walkers_accept :21). */
int aiqmc_dmc_drift_diffusion(aiqmc_ctx* ctx, void* pos_inout, int32_t B, double tstep, int32_t rng_mode,
                              const void* gauss1, const void* gauss2, const void* u, uint64_t seed, uint64_t offset,
                              void* grad_eff_old, void* grad_new_eff, double* tdamp, void* stream);

/* DMC weight update (DMC/S_matrix.py:4-24, dmc.py:80-92): with S from the real
 * local energies eloc_old/eloc_new [B], v2 = |grad_eff|^2 per walker and the tdamp[3]
 * array of aiqmc_dmc_drift_diffusion (its entry 2 is used),
 * weights[B] *= exp(tstep tdamp (S_new + S_old)/2). */
int aiqmc_dmc_weights(aiqmc_ctx* ctx, int32_t B, const void* eloc_old, const void* eloc_new, const void* grad_eff_old,
                      const void* grad_new_eff, const double* tdamp, double tstep, double e_trial, double e_est,
                      double branchcut, void* weights_inout, void* stream);

/* aiqmc_dmc_weights with the general arguments of comput_S as main_dmc.py drives it:
 *   e_trial_b / e_est_b (optional, device [B], ctx dtype): per-walker e_trial / e_est -- the
 *     driver's first block passes the per-walker pp energies of total_e (main_dmc.py:115-116);
 *     NULL: the scalars e_trial / e_est;
 *   cut_minima (optional, device double[2]): the e_cut minima for eloc_old / eloc_new
 *     (S_matrix.py:21-22: ONE jnp.min over the stacked arrays of ALL devices and the branch
 *     cut) -- a multi-GPU run all-reduces aiqmc_dmc_cut_minima with MIN and passes the result;
 *     NULL: computed from this batch. */
int aiqmc_dmc_weights_ex(aiqmc_ctx* ctx, int32_t B, const void* eloc_old, const void* eloc_new,
                         const void* grad_eff_old, const void* grad_new_eff, const double* tdamp, double tstep,
                         const void* e_trial_b, const void* e_est_b, double e_trial, double e_est, double branchcut,
                         const double* cut_minima, void* weights_inout, void* stream);

/* This batch's e_cut minima (S_matrix.py:21-22) for eloc_old / eloc_new: out (device
 * double[2]) = min(branchcut, min_b |e_est_b - eloc_b|) (e_est_b optional as above). */
int aiqmc_dmc_cut_minima(aiqmc_ctx* ctx, int32_t B, const void* eloc_old, const void* eloc_new, const void* e_est_b,
                         double e_est, double branchcut, double* out, void* stream);

/* Stochastic comb (DMC/branch.py:10-33) with the uniform draw u in [0,1):
 * newinds[B] (int32, device) = searchsorted(cumsum(w), (u wtot + j wtot/B) mod wtot),
 * weight_out[1] = wtot / B (device, ctx dtype). */
int aiqmc_dmc_branch(aiqmc_ctx* ctx, int32_t B, const void* weights, double u, int32_t* newinds, void* weight_out,
                     void* stream);

/* Pseudopotential tables (pphamiltonian.local_energy arguments,
 * Energy/pphamiltonian.py:130-146; shapes as the example drivers pass them,
 * example/single_atom_C/single_atom_C.py:13-23).  All HOST pointers; the
 * nonlocal arrays have list_l + 1 angular channels (P_l of
 * pseudopotential.py:250-269 returns list_l + 1 terms). */
typedef struct aiqmc_ecp {
  int32_t list_l;               /* 0..3                                       */
  int32_t n_local;              /* KL = Rn_local.shape[1]                     */
  int32_t n_nonlocal;           /* KN = Rn_non_local.shape[2]                 */
  const double* rn_local;       /* [A][KL]  (r**(n-2), pseudopotential.py:95) */
  const double* local_coes;     /* [A][KL]                                    */
  const double* local_exps;     /* [A][KL]                                    */
  const double* rn_non_local;   /* [A][list_l+1][KN]  (r**n, :150)            */
  const double* non_local_coes; /* [A][list_l+1][KN]                          */
  const double* non_local_exps; /* [A][list_l+1][KN]                          */
} aiqmc_ecp;

/* Attach pseudopotential tables to the context (replaces the closure
 * arguments of pphamiltonian.local_energy).  The potential charges of the
 * context (aiqmc_cfg.charges) are the effective core charges Z_eff. */
int aiqmc_set_ecp(aiqmc_ctx* ctx, const aiqmc_ecp* ecp);

/* Complex pseudopotential local energy of B walkers (the reference's
 * pphamiltonian.local_energy(...) -> _e_l(params, key, data), vmapped with one
 * key per walker, loss.py:203-204):
 *   e_re + i e_im = V_ee + V_nn + KE + local pp + nonlocal pp
 * with the nonlocal quadrature over the 50-point grid rotated by one random
 * orthogonal matrix per walker (pseudopotential.py:233-241).
 * rng_mode AIQMC_RNG_HOST: rot = device [B][3][3] (row-major, ctx dtype), the
 *   matrix jax.random.orthogonal would return; AIQMC_RNG_PHILOX: rot may be
 *   NULL, Haar O(3) matrices are drawn from (seed, offset).
 * logabs_q / phase_q (optional, [B][N][A][50]): log|psi| and phase at the
 * quadrature configurations, electron i moved to r_ia * (p_q R). */
int aiqmc_local_energy_ecp(aiqmc_ctx* ctx, const void* pos, int32_t B, int32_t rng_mode, const void* rot,
                           uint64_t seed, uint64_t offset, void* e_re, void* e_im, void* logabs_q,
                           void* phase_q, void* stream);

/* The same with complex_output=True (pphamiltonian.local_energy(..., complex_output=True),
 * Energy/pphamiltonian.py:84-104, whose kinetic phase branch is hamiltonian.py:110-130): the
 * kinetic energy's phase terms + 1/2 |grad theta|^2 - i (lap theta / 2 + grad log|psi| . grad theta)
 * are added to e_re / e_im, theta = arg psi.  Two local-energy launch pairs (log|psi|, theta). */
int aiqmc_local_energy_ecp_complex(aiqmc_ctx* ctx, const void* pos, int32_t B, int32_t rng_mode, const void* rot,
                                   uint64_t seed, uint64_t offset, void* e_re, void* e_im, void* stream);

/* DMC T-moves (DMC/Tmoves.py:32-225, called per walker by dmc.py:79 before the
 * drift-diffusion step), in place on pos_inout [B][3N]: for every electron the
 * pp quadrature configurations of aiqmc_local_energy_ecp give the amplitudes
 * ratio * sum_l (exp(-tstep v_l) - 1) P_l(cos); one configuration per electron
 * is selected with the reference's cdf / searchsorted rule and accepted with
 * Re(norm / back_norm) > u (quirks T1-T8, oracle/dmc.py).  Needs aiqmc_set_ecp.
 * rng_mode AIQMC_RNG_HOST: rot [B][3][3] (get_rot's matrix), u_sel [B]
 *   (select_walker's uniform, one per walker, shared by its electrons) and
 *   u_acc [B][N] (the acceptance uniforms), device arrays of the ctx dtype;
 * AIQMC_RNG_PHILOX: all three drawn from (seed, offset).
 * acceptance (optional, [B][N], ctx dtype): Re(norm / back_norm). */
int aiqmc_dmc_tmoves(aiqmc_ctx* ctx, void* pos_inout, int32_t B, double tstep, int32_t rng_mode, const void* rot,
                     const void* u_sel, const void* u_acc, uint64_t seed, uint64_t offset, void* acceptance,
                     void* stream);

/* Energy statistics of one VMC iteration (constants.pmean_stats; the reference's two pmeans,
 * AIQMCrelease3 Loss/loss.py:206-208).  e_l[n] (dtype AIQMC_F32 | AIQMC_F64, device memory) is
 * reduced in fp64 into out[0..3] = [sum |e - m|^2, n m, n m^2, n] (m = the mean of these n
 * energies), one workgroup; the 4-vectors of all ranks sum (one all-reduce) to the pooled
 * statistics.  finalize != 0 also writes out[4..5] = [mean, variance] of these n energies.
 * aiqmc_energy_stats_final writes out[4..5] from a summed out[0..3].  out: >= 6 device doubles. */
int aiqmc_energy_stats(const void* e_l, int32_t dtype, int64_t n, double* out, int32_t finalize, void* stream);
int aiqmc_energy_stats_final(double* out, void* stream);

/* The energy-gradient weights of make_loss on ONE rank (Loss/loss.py:73-135 clipping with the
 * mean as centre, :206-208 statistics, :256-265 tangent weights), one launch: for local energies
 * e = e_re + i e_im (e_im NULL: real) of n walkers,
 *   stats[0..4] = [Re mean, Im mean, variance mean|e - mean|^2, Re centre, Im centre],
 *   w_re[b] = wscale Re(diff_b),  w_im[b] = wscale Im(diff_b + aux_b)  (w_im may be NULL),
 *   clipped_re/im[b] = aux.clipped_energy (may be NULL),
 * with clip_scale > 0: total-variation window around the mean per component, diff = clipped -
 * centre, centre = mean(clipped) (center_at_clipped) or the mean, aux = centre; clip_scale <= 0:
 * diff = e - mean, aux = e.  Sums in double, fixed order.  (Several ranks: the statistics need
 * all-reduces between the stages; the Python layer keeps its torch path there.) */
int aiqmc_loss_weights(const void* e_re, const void* e_im, int32_t dtype, int64_t n, double clip_scale,
                       int32_t center_at_clipped, double wscale, void* w_re, void* w_im, void* clipped_re,
                       void* clipped_im, double* stats, void* stream);

/* The same statistics, clipping and gradient weights over SEVERAL ranks, as three levels whose
 * rank partials sum with one all-reduce each (Loss/loss.py:107,206,208 and the gradient pmean of
 * Optimizer/adam.py:55).  aiqmc_loss_level(level, ...) for this rank's n energies:
 *   level 1: out[0..5] = L1 = [sum |e - m|^2, n Re m, n Im m, n |m|^2, n, #(Im e != 0)]  (m: rank mean)
 *   level 2: out[0..1] = L2 = [sum |Re e - Re E|, sum |Im e - Im E|]  from the SUMMED L1 (clipping only)
 *   level 3: from the summed L1 (and L2 when clip_scale > 0): the clipped energies xc (the total-
 *            variation window around the mean, clipped_re/im, may be NULL), the gradient weights
 *            w[0][b] = wscale (Re xc_b - Re E), w[1][b] = wscale (g0 != 0; centre at the clipped mean),
 *            wp[b] = the phase weight (wscale Im xc clipping, wscale (2 Im e - Im E) without; may be NULL),
 *            and out[0..1] = [sum Re xc, sum Im xc].
 * The caller then forms G = w[0]-weighted d log|psi| + wp-weighted d phase and G0 = w[1]-weighted
 * d log|psi| (aiqmc_param_grad_weighted), packs L3 = [out[0..1], G, G0] (aiqmc_loss_pack: double
 * L3[2 + 2P]), all-reduces it, and aiqmc_loss_final writes the pmean'd gradient
 * grad = (G - (Re dc - Re E) G0) / world (ctx dtype) and stats[0..5] = [Re E, Im E, variance,
 * Re dc, Im dc, #(Im e != 0) over all ranks] (dc: the clipped mean when center_at_clipped, else E).
 * L1/L2/L3/out/stats are device doubles; weights and energies of `dtype`. */
int aiqmc_loss_level(int32_t level, const void* e_re, const void* e_im, int32_t dtype, int64_t n,
                     const double* L1, const double* L2, double clip_scale, double wscale, int32_t g0, void* w,
                     void* wp, void* clipped_re, void* clipped_im, double* out, void* stream);
int aiqmc_loss_pack(const void* g, const void* gp, const void* g0, int32_t dtype, int32_t P, double* L3,
                    void* stream);
int aiqmc_loss_final(const double* L1, const double* L3, int32_t P, int32_t g0, int32_t center_at_clipped,
                     int32_t world, int32_t dtype, void* grad, double* stats, void* stream);

/* The centred Gram product of stochastic reconfiguration (aiqmc/Optimizer/sr.py): for the
 * per-walker Jacobians o_re = d log|psi| / d theta and o_im = d phase / d theta ([B][P] row-major
 * device arrays of `dtype`, as aiqmc_logpsi_param_grad / aiqmc_phase_param_grad return them
 * without weights; o_im NULL = absent) and a centre c (center_re / center_im: [P] device arrays
 * of the same `dtype`, NULL = 0), out (device fp64, P*P + 2P + 1 entries, the vector for ONE sum
 * all-reduce) receives
 *   G[P][P] = sum_b (o_re_b - c_re)(o_re_b - c_re)^T + (o_im_b - c_im)(o_im_b - c_im)^T   (full, symmetric)
 *   s_re[P] = sum_b (o_re_b - c_re),  s_im[P] = sum_b (o_im_b - c_im),  n = B,
 * from which the covariance for ANY centre is G/n - (s_re s_re^T + s_im s_im^T)/n^2.
 * accumulate != 0 adds into out instead of overwriting it (walker blocks).  Context-free; runs on
 * the current device.  One workgroup owns a 64 x 64 tile of G for all walkers (no atomics: the
 * same bits run to run, G == G^T bitwise); sums run in `dtype` on the matrix cores over chunks of
 * AIQMC_SR_CHUNK walkers (re and im apart), the chunks are added in fp64 in ascending order.
 * B == 0 writes (or adds) zeros. */
#define AIQMC_SR_CHUNK 256
int aiqmc_sr_gram(const void* o_re, const void* o_im, int32_t dtype, int64_t B, int32_t P,
                  const void* center_re, const void* center_im, double* out, int32_t accumulate, void* stream);

/* Spin-squared estimator for the fixed spin assignment of the context (the assign_spin=True
 * branch of ferminet/observables.py:98-227 make_s2, restated for the slot-based spin tables):
 *   S2_L(x) = (na - nb)/2 ((na - nb)/2 + 1) + nb - sum_{i in up} sum_{j in down} psi(x_{i<->j}) / psi(x),
 * na = max(n_up, n_down), nb = min(n_up, n_down), x_{i<->j} = x with the coordinates of electron
 * slots i and j exchanged (the spin labels stay on the slots).  psi is complex, so the ratio is
 * exp(dlogabs) (cos dphase + i sin dphase): s2_re[B], s2_im[B] (ctx dtype) receive the real and
 * imaginary parts (the latter averages to zero).  dlogabs / dphase (optional, [B][n_up][n_down],
 * i over spin_up_indices in the outer index, j over spin_down_indices in the inner one): log|psi|
 * and phase at the exchanged configuration minus those at the walker.  Nothing is clamped: a
 * walker on a node gives an infinite or NaN ratio.  Cost: n_up n_down + 1 value forwards per
 * walker, launched in chunks whose workspace does not depend on B; sums in a fixed order (the
 * same bits run to run).  B == 0 writes nothing.  Needs aiqmc_set_params. */
int aiqmc_spin_squared(aiqmc_ctx* ctx, const void* pos, int32_t B, void* s2_re, void* s2_im, void* dlogabs,
                       void* dphase, void* stream);

/* Dipole moment of B configurations in atomic units (ferminet/observables.py:230-272 make_dipole
 * with the nuclear term): mu[B][3] = sum_a Z_a R_a - sum_i r_i, Z_a the context charges (Z_eff
 * under an ECP). */
int aiqmc_dipole(aiqmc_ctx* ctx, const void* pos, int32_t B, void* mu, void* stream);

/* What the local energy is made of: out[k][b] (AIQMC_NCOMPONENTS rows of B, ctx dtype, real), one
 * sample x[K][B] for aiqmc_blocking_update (K = 8 = AIQMC_BLOCKING_MAX_SERIES):
 *   AIQMC_COMP_TOTAL          Re E_L: written by aiqmc_local_energy (complex_output != 0:
 *                             aiqmc_local_energy_complex), under an ECP by aiqmc_local_energy_ecp
 *                             (aiqmc_local_energy_ecp_complex), called as they are -- their bits;
 *                             rng_mode, rot, seed and offset are theirs and ignored without an ECP
 *   AIQMC_COMP_KINETIC        T_L = the all-electron E_L of this context - (v_ee + v_en + v_nn)
 *                             = -1/2 (lap log|psi| + |grad log|psi||^2), with complex_output plus the
 *                             phase term 1/2 |grad theta|^2.  Under an ECP the all-electron entry is
 *                             called as well as the ECP one.
 *   AIQMC_COMP_KINETIC_GRAD   T_G = 1/2 sum |grad log|psi||^2 from the gradient of that launch.
 *                             <T_G> = <T_L> over |psi|^2 for a wavefunction whose phase is piecewise
 *                             constant (integration by parts); their gap is the standard check of
 *                             the sample's equilibration and of the Laplacian.
 *   AIQMC_COMP_V_EE           sum_{i<j} 1 / r_ij
 *   AIQMC_COMP_V_EN           -sum_{i,a} Z_a / r_ia, Z the context charges (Z_eff under an ECP: part1
 *                             of local_pp_energy, pseudopotential.py:111)
 *   AIQMC_COMP_V_NN           sum_{a<b} Z_a Z_b / R_ab, summed on the host in double and rounded to the
 *                             dtype: the same value for every walker
 *   AIQMC_COMP_V_PP_LOCAL     sum_{i,a,k} c_ak r^(n_ak - 2) exp(-alpha_ak r^2) (pseudopotential.py:86-117
 *                             without part1); 0 without aiqmc_set_ecp
 *   AIQMC_COMP_V_PP_NONLOCAL  total - (kinetic + v_ee + v_en + v_nn + v_pp_local); 0 without an ECP
 * One launch after the energy launches, a group of 16 lanes per walker; distances and terms in the
 * ctx dtype, each walker summed in a fixed order (csrc/components.hip), no atomics: rows 3..6 of a
 * walker depend on its coordinates alone and are the same bits for any B, batching or position in
 * the batch.  Nothing is clamped: coincident particles give +-inf in that walker only, NaN
 * propagates.  The scratch (one or two energy vectors, the gradient) is reserved at the first call.
 * Non-zero, before any device work, with a message naming the field: a null context, parameters
 * not set (AIQMC_ESTATE), B < 0, a null pos / out with B > 0, under an ECP an unknown rng_mode or
 * AIQMC_RNG_HOST with a null rot.  B == 0 returns AIQMC_OK and writes nothing. */
#define AIQMC_NCOMPONENTS 8
#define AIQMC_COMP_TOTAL 0
#define AIQMC_COMP_KINETIC 1
#define AIQMC_COMP_KINETIC_GRAD 2
#define AIQMC_COMP_V_EE 3
#define AIQMC_COMP_V_EN 4
#define AIQMC_COMP_V_NN 5
#define AIQMC_COMP_V_PP_LOCAL 6
#define AIQMC_COMP_V_PP_NONLOCAL 7
int aiqmc_energy_components(aiqmc_ctx* ctx, const void* pos, int32_t B, int32_t complex_output,
                            int32_t rng_mode, const void* rot, uint64_t seed, uint64_t offset,
                            void* out /* [8][B], ctx dtype */, void* stream);

/* Electron density and pair-correlation histograms, accumulated on the device across sweeps.
 * This is the DIAGONAL of the one-body density matrix (the matrix itself on a Gaussian basis is
 * aiqmc_rdm_accumulate): it needs only the walkers.
 * One call bins B walkers into the caller-owned device accumulator acc (int64 words, zeroed by
 * the caller before the first call, then only added to).  Three optional families; a family with
 * zero bins is absent together with its outside words:
 *   grid    [2][nx][ny][nz]  spin-resolved density on the box [grid_lo, grid_hi)
 *   radial  [2][A][rad_n]    distances to each of the context's atoms over [0, rad_max)
 *   pair    [3][pair_n]      electron-electron distances over pairs i < j over [0, pair_max)
 * Channels: grid / radial 0 = the up slots, 1 = the down slots of the context's spin tables
 * (spin_up_indices / spin_down_indices, not position order); pair 0 = up-up, 1 = down-down,
 * 2 = up-down.  Accumulator layout, offsets8 of aiqmc_density_layout in this order:
 *   total[1] skipped[1] grid[2 nx ny nz] grid_out[2] radial[2 A rad_n] radial_out[2 A]
 *   pair[3 pair_n] pair_out[3]
 * Bin rule, the same for every axis, in the context dtype T: f = (x - lo) * inv_h with
 * inv_h = n / (hi - lo) formed in double and rounded to T once (distances: f = r * inv_h); a sample
 * is inside iff f >= 0 && f < n, its bin is (int)floor(f); everything else (NaN and infinite
 * coordinates included) is tallied in the channel's word of the family's `_out` array (a grid
 * sample is inside iff all three axes are).
 * Fixed point: the words count in units of 2^-32.  A sample of a walker of weight w (weights: T[B]
 * or NULL) adds llrint((double)w * 4294967296.0), exactly 1 << 32 without weights; `total`
 * accumulates the walker weights in the same units.  A walker whose weight is negative, not
 * finite or >= 2^31 adds nothing and is counted in the plain integer `skipped`.  Capacity: 2^31
 * units of weight per word before the int64 overflows.  All updates are integer adds: the words
 * are the same bits for any launch shape, any chunking of the batch, any walker order and any
 * number of ranks (sum the words).
 * radial + radial_out + pair + pair_out are privatised per workgroup in LDS when they hold at most
 * AIQMC_DENSITY_LDS_WORDS words (*privatised = 1), and go to global atomics above that; the words
 * do not depend on the path.  One launch on `stream`, no workspace.  Needs no parameters.
 * AIQMC_EINVAL, before any device work, with a message naming the field: a null context or
 * configuration, B < 0, a negative count or one above AIQMC_DENSITY_MAX_BINS, grid_hi <= grid_lo
 * (or not finite) on a present grid, rad_max / pair_max not positive and finite when its count is
 * non-zero, more than AIQMC_DENSITY_MAX_WORDS words, a null pos / acc with B > 0.  B == 0 is a
 * no-op. */
#define AIQMC_DENSITY_LDS_WORDS 4096          /* 32 KiB of LDS per workgroup */
#define AIQMC_DENSITY_MAX_BINS (1 << 20)      /* per count: exact in float */
#define AIQMC_DENSITY_MAX_WORDS (1 << 28)     /* 2 GiB accumulator */
typedef struct aiqmc_density_cfg {
  double grid_lo[3], grid_hi[3];
  int32_t grid_n[3];             /* any n == 0: no grid */
  double rad_max;
  int32_t rad_n;                 /* 0: none */
  double pair_max;
  int32_t pair_n;                /* 0: none */
} aiqmc_density_cfg;
int aiqmc_density_layout(const aiqmc_ctx* ctx, const aiqmc_density_cfg* cfg, int64_t* offsets8, int64_t* n_words,
                         int32_t* privatised);
int aiqmc_density_accumulate(aiqmc_ctx* ctx, const aiqmc_density_cfg* cfg, const void* pos, int32_t B,
                             const void* weights, int64_t* acc, void* stream);

/* Diagnostics: configurations per value launch of aiqmc_spin_squared (default 4096; nconf <= 0
 * restores it).  A chunk holds whole walkers, at least one.  Results do not depend on it. */
int aiqmc_debug_set_obs_chunk(aiqmc_ctx* ctx, int32_t nconf);

/* One-body reduced density matrix in a caller-supplied Gaussian basis (the quantity of
 * ferminet/observables.py make_density_matrix; the basis is the caller's instead of an SCF run's).
 * For each spin channel s (0 = the up slots, 1 = the down slots of the context's spin tables),
 * functions phi_1..phi_K, walkers x_b ~ |psi|^2 with weights w_b and S points r'_bs per walker
 * drawn from a known density q,
 *   rho^s_ij = 1/(W S) sum_b w_b sum_s' sum_{e in s} phi_i(r_e) phi_j(r'_bs') psi(x_b; r_e -> r'_bs') / psi(x_b) / q(r'_bs'),
 * W = sum_b w_b, summed over EVERY electron of the channel (this ansatz is not antisymmetric under
 * same-spin exchange, so the first electron alone would not give its density matrix).  psi is
 * complex, so rho is.
 *
 * Basis (aiqmc_set_rdm_basis; NULL clears it): contracted Cartesian Gaussian shells with l in
 * {0, 1, 2}, each with its own centre, functions in the order 1 | x y z | xx xy xz yy yz zz; a
 * function's value is x^a y^b z^c sum_p coefs[p] exp(-exps[p] r^2), coefficients as given (no
 * norm is folded in).  mo_coeff (optional, [2][nao][norb] row-major, spin-major) makes
 * phi^s_j = sum_a ao_a C[s][a][j]; NULL: the functions themselves (norb is ignored and is nao).
 * q is a mixture of nq <= AIQMC_RDM_MAX_Q isotropic Gaussians,
 *   q(r) = sum_k q_prob[k] (2 pi q_sigma[k]^2)^-3/2 exp(-|r - q_center[k]|^2 / (2 q_sigma[k]^2)),
 * q_prob > 0 summing to 1 within 1e-12, q_sigma > 0.  phi_j / q stays bounded iff
 * q_sigma^2 >= 1 / (2 alpha_min) for the smallest exponent of the basis.  AIQMC_EINVAL with a
 * message naming the field: l > 2, nao > AIQMC_RDM_MAX_AO, norb > AIQMC_RDM_MAX_ORB, more than
 * AIQMC_RDM_MAX_PRIM primitives, a shell without primitives, nq outside [1, AIQMC_RDM_MAX_Q], a
 * bad q_prob / q_sigma, a null table.  The context keeps device copies; the call synchronises.
 *
 * aiqmc_rdm_accumulate: acc (device fp64, 1 + 2 K K 2 entries, K = norb) receives SUMS, not means:
 * acc[0] = W and acc[1 + ((s K + i) K + j) 2 + {0, 1}] = Re, Im of W S rho^s_ij; accumulate != 0
 * adds into acc instead of overwriting it.  rng_mode AIQMC_RNG_HOST: rprime_in [B][S][3] (ctx
 * dtype) are the points; AIQMC_RNG_PHILOX: point (b, s) is drawn from q with stream id b S + s of
 * (seed, step): kind 25's first uniform u picks the smallest k with u < q_prob[0] + .. + q_prob[k]
 * (partial sums in fp64; the last component takes what is left), kind 24's three normals g give
 * r' = fma(sigma_k, g, c_k) in the ctx dtype.  weights: [B] ctx dtype or NULL (all 1).  Optional
 * outputs: rprime_out [B][S][3], ratio_out [B][S][N][2] = (log|psi|, phase) at the walker with
 * electron slot e at r'_bs minus those at the walker -- bit for bit differences of aiqmc_logpsi
 * values, the moved configurations go through its launch.  Cost: N S + 1 value forwards per
 * walker in chunks of the aiqmc_debug_set_obs_chunk size (a chunk is a whole number of groups of
 * AIQMC_RDM_GROUP walkers, or the whole batch).  Summation order, a function of (B, S, K) and the
 * channel sizes only: rows (walker, point, electron of the channel) ascending within a group of
 * AIQMC_RDM_GROUP walkers (by index within the call) in the ctx dtype on the matrix cores
 * (v_mfma_{f32,f64}_16x16x4), the group tiles added into acc in fp64, groups ascending; no
 * atomics, the same bits run to run and for any chunking.  The Gaussians and q are evaluated in
 * fp64 for both dtypes and rounded once.  Nothing is clamped.  B == 0 returns AIQMC_OK and writes
 * nothing.  AIQMC_ESTATE without parameters or without a basis; AIQMC_EINVAL for S < 1, an
 * unknown rng_mode, AIQMC_RNG_HOST with a null rprime_in, a null acc.
 *
 * aiqmc_rdm_basis_values: out[M][K] (ctx dtype) = phi^spin_j(points[m]) for points [M][3] (ctx
 * dtype), the basis evaluator alone.  Needs the basis, not the parameters. */
#define AIQMC_RDM_GROUP 32
#define AIQMC_RDM_MAX_AO 128
#define AIQMC_RDM_MAX_ORB 64
#define AIQMC_RDM_MAX_PRIM 512
#define AIQMC_RDM_MAX_Q 16
typedef struct aiqmc_rdm_basis {
  int32_t nshell;
  const int32_t* shell_l;       /* [nshell] */
  const int32_t* shell_nprim;   /* [nshell] */
  const double* shell_center;   /* [nshell][3] */
  const double* exps;           /* [sum shell_nprim], shell after shell */
  const double* coefs;          /* the same layout */
  int32_t norb;
  const double* mo_coeff;       /* [2][nao][norb] or NULL */
  int32_t nq;
  const double* q_center;       /* [nq][3] */
  const double* q_sigma;        /* [nq] */
  const double* q_prob;         /* [nq] */
} aiqmc_rdm_basis;
int aiqmc_set_rdm_basis(aiqmc_ctx* ctx, const aiqmc_rdm_basis* basis);
int aiqmc_rdm_accumulate(aiqmc_ctx* ctx, const void* pos, int32_t B, int32_t S, int32_t rng_mode,
                         const void* rprime_in, uint64_t seed, uint64_t step, const void* weights, double* acc,
                         int32_t accumulate, void* rprime_out, void* ratio_out, void* stream);
int aiqmc_rdm_basis_values(aiqmc_ctx* ctx, const void* points, int32_t M, int32_t spin, void* out, void* stream);

/* Space-warp transform between nuclear geometries with its Jacobian (correlated sampling: the
 * walkers of one run at the context's atoms R evaluated at M nearby geometries R'_m).  The warp is
 * the reference's correlatedsamples/corrsamples.py:23-47 (Filippi-Umrigar), per electron r:
 *   d_a = r - R_a, r_a = |d_a|, w_a = q_a / sum_b q_b, q_a = (r_min / r_a)^4  (= r_a^-4 / sum r_b^-4,
 *   scaled so that nothing overflows; r_min = 0: 1/k on the k atoms at zero distance),
 *   r' = r + sum_a w_a dR_a, dR_a = R'_a - R_a, evaluated as r + dR_n + sum_a w_a (dR_a - dR_n) with n
 *   the nearest atom (sum_a w_a = 1; a rigid translation is reproduced exactly).
 * logjac[m][b] = sum_i log|det J_i|, J_i[k][l] = delta_kl + sum_a dR_a[k] d_l w_a(r_i) with
 * grad w_a = 4 w_a sum_{b != a} w_b (g_b - g_a), g_a = d_a / r_a^2 (0 for r_min = 0), the 3x3
 * determinant in closed form, electrons added in ascending slot order.  This is the Jacobian
 * that correlatedsamples/jacobianWeights.py:22-51 leaves unfinished ("to be continued"; its
 * 1 - atoms per Cartesian component is not a derivative).  Nothing is clamped: a singular J_i
 * gives -inf.  pos [B][3N], newpos [M][B][3N] and logjac [M][B] (may be NULL) are of the ctx
 * dtype; new_atoms is a DEVICE double [M][A][3]; dR is formed in double, the rest in the ctx
 * dtype.  One launch, no workspace; a (m, b) row depends on nothing else, so the results are the
 * same bits from run to run and for any B, M or chunking.  B == 0 or M == 0 writes nothing.
 * AIQMC_EINVAL for a null context, negative B or M, or null pos / new_atoms / newpos, before the
 * GPU is touched.  Needs no parameters. */
int aiqmc_space_warp(aiqmc_ctx* ctx, const void* pos, int32_t B, const double* new_atoms, int32_t M,
                     void* newpos, void* logjac, void* stream);

/* The reweighted energy-difference estimator of correlated sampling as three levels whose rank
 * partials combine in one all-reduce each (context-free, as aiqmc_loss_level).  The walkers x_b
 * are drawn from |psi_R|^2; for geometry m, with T_m the space warp,
 *   lw_b = 2 (logabs1[m][b] - logabs0[b]) + logjac[m][b]     (logabs1 = log|psi_R'm(T_m x_b)|),
 * the probability ratio the reference's driver replaces by |log psi_R - log psi_R'|^2 at the
 * un-warped positions (VMC/VMC_energy_correlated_samples.py:184).  Inputs of `dtype`:
 * logabs0 [n], e0 [n] (Re E_L at (x_b; R)), logabs1 / logjac / e1 [M][n] (e1 = Re E_L at
 * (T_m x_b; R'_m)); L1, L2, out are device doubles.  One workgroup per geometry, sums in double
 * in a fixed tree order, no atomics:
 *   level 1  out[m]       = max_b lw_b                                        (ranks: MAX)
 *   level 2  out[m][0..4] = [n, sum e0, sum w, sum w e1, sum w^2], w_b = exp(lw_b - L1[m])  (SUM)
 *   level 3  out[m][0..1] = [sum d, sum d^2],
 *            d_b = (w_b n / sum w)(e1_b - E_m) - (e0_b - E_0), from L1 and the summed L2      (SUM)
 * e0 / e1 may be NULL at level 1.  NaN and inf propagate (the maximum too). */
int aiqmc_corr_level(int32_t level, int32_t dtype, int64_t n, int32_t M, const void* logabs0, const void* e0,
                     const void* logabs1, const void* logjac, const void* e1, const double* L1, const double* L2,
                     double* out, void* stream);

/* res[m][0..4] = [E_0, E_m, E_m - E_0, err_m, ESS_m] from the summed L2 [M][5] and L3 [M][2]:
 * E_0 = sum e0 / n, E_m = sum w e1 / sum w, ESS_m = (sum w)^2 / sum w^2 and the delta-method error
 * err_m = sqrt((sum d^2 - (sum d)^2 / n) / (n (n - 1))) (NaN for n = 1). */
int aiqmc_corr_final(const double* L2, const double* L3, int32_t M, double* res, void* stream);

/* Error bars for serially correlated series: the Flyvbjerg-Petersen blocking analysis in its
 * online form, accumulated on the device across sweeps (context-free, as aiqmc_sr_gram).  A sample
 * is one call's values x[K][B] (`dtype`): K series over the SAME B Markov chains in the same order
 * at every call.  With t the number of samples taken so far (0-based index of this one):
 *   v_0 = x - shift completes level 0;  for k = 0, 1, ..: stop if k + 1 == L; if bit k of t is set,
 *   v_{k+1} = (pend[k+1] + v_k) / 2 completes level k + 1, go on; otherwise pend[k+1] = v_k, stop.
 * A level-k block is thus the mean of 2^k consecutive samples of one chain, blocks aligned to the
 * first sample; the top level L - 1 keeps receiving blocks of 2^(L-1) samples for ever.  Every level
 * that completes adds, over all chains, n += B, S[i] += v_i, Q[i][j] += v_i v_j (i <= j).
 * Buffers (device doubles, owned and zeroed by the caller before the first call; sizes from
 * aiqmc_blocking_layout), M = 1 + K + K (K + 1) / 2:
 *   acc      [t, shift[K], level 0 words[M], .., level L-1 words[M]], a level's words = [n, S[K],
 *            Q upper triangle row-major]; t is a double (exact to 2^53), read AND incremented on
 *            the device (the host never needs it); shift is written once by the caller after the
 *            zeroing and keeps sum v^2 well conditioned
 *   pend     [L][K][B], the blocks waiting for their partner (pend[0] is unused)
 *   scratch  the partial sums of one call
 * Nothing is clamped: NaN and inf propagate into exactly the levels they reach.  All arithmetic is
 * fp64; fp32 samples are widened exactly.  No atomics: the chains are summed in fixed chunks of 256
 * (a butterfly over each wave, then the four waves in order), the chunk partials in ascending
 * chunk order by one workgroup of a second launch, so the words are a function of (B, samples)
 * only, the same bits from run to run.  Two launches on `stream`, no host synchronisation.
 * AIQMC_EINVAL, before any device work, with a message naming the field: a null x / acc / pend /
 * scratch, B < 1 (or above 2^38), K outside 1..AIQMC_BLOCKING_MAX_SERIES, L outside
 * 1..AIQMC_BLOCKING_MAX_LEVELS, an unknown dtype. */
#define AIQMC_BLOCKING_MAX_SERIES 8
#define AIQMC_BLOCKING_MAX_LEVELS 32
int aiqmc_blocking_layout(int64_t B, int32_t K, int32_t L, int64_t* acc_words, int64_t* pend_words,
                          int64_t* scratch_words);
int aiqmc_blocking_update(const void* x, int32_t dtype, int64_t B, int32_t K, int32_t L, double* acc, double* pend,
                          double* scratch, void* stream);

/* Optional HIP-event timing of the hot kernels, recorded on the caller's
 * stream around each launch while enabled.  Slots: 0 = proposal
 * value+gradient launches of aiqmc_mc_step, 1 = walker gradient launches of
 * aiqmc_mc_step, 2 = aiqmc_local_energy launches, 3 = value-only launches of
 * the ECP quadrature configurations.  aiqmc_profile_read waits
 * for the recorded events, returns the summed kernel time in ms and the launch
 * count of one slot, and clears it. */
int aiqmc_profile_enable(aiqmc_ctx* ctx, int32_t on);
int aiqmc_profile_read(aiqmc_ctx* ctx, int32_t slot, double* total_ms, int64_t* launches);

/* Diagnostics: aiqmc_logpsi_grad through the forward-mode kernel (the
 * production gradient is reverse mode); used to cross-check the two
 * derivative implementations at full batch size. */
int aiqmc_debug_logpsi_grad_forward(aiqmc_ctx* ctx, const void* pos, int32_t B, void* logabs, void* grad,
                                    void* stream);

/* Diagnostics: aiqmc_local_energy through the single-launch forward-Laplacian
 * kernel (second-order jets carried through the whole network).  The production
 * path (adjoint pass + first-derivative pass) must agree with it to rounding. */
int aiqmc_debug_local_energy_forward(aiqmc_ctx* ctx, const void* pos, int32_t B, void* e_l, void* logabs,
                                     void* grad, void* stream);

/* Diagnostics: aiqmc_mc_step evaluates each single-electron proposal from the
 * walker's cached electron stage and pair sums, recomputing only the moved
 * electron and its 2(N-1) pairs (default, on = 1).  on = 0 recomputes every
 * proposal from scratch; both must agree to rounding. */
int aiqmc_debug_set_proposal_reuse(aiqmc_ctx* ctx, int32_t on);

/* Waves per walker of the local energy's first-derivative pass (k_walker_lap): 1, 2 or 4, or
 * 0 (default) = the fewest that give >= 2 waves per SIMD for the batch (small per-GPU batches
 * under strong scaling split each walker over more waves).  Results agree to rounding. */
int aiqmc_debug_set_lap_waves(aiqmc_ctx* ctx, int32_t waves);

/* Diagnostics: aiqmc_mc_step applies the acceptance of every sweep but the last inside the
 * next sweep's walker launch (default, on = 1); on = 0 runs a separate acceptance launch per
 * sweep.  Both are bitwise identical (same arithmetic, same order). */
int aiqmc_debug_set_fuse_accept(aiqmc_ctx* ctx, int32_t on);

/* Diagnostics: from the second sweep of an aiqmc_mc_step call on, the walker launch's
 * Gauss-Jordan elimination takes the walker's pivot order of the previous sweep (default,
 * reuse = 1; partial pivoting only when a pivot comes out below 0.1 of the previous one);
 * reuse = 0 runs partial pivoting in every sweep.  Results agree to rounding. */
int aiqmc_debug_set_walker_pivots(aiqmc_ctx* ctx, int32_t reuse);

/* Diagnostics (host only, no GPU call): dynamic LDS bytes per workgroup and waves per workgroup
 * of the launches of shape (N, A) that size their LDS at launch time -- the part of a kernel's
 * LDS that a profiler's dispatch record does not report.  kind: AIQMC_LDS_*; dtype AIQMC_F32 /
 * AIQMC_F64.  waves = 0: chosen per launch (the first-derivative pass: 1, 2 or 4 by batch size).
 * (profiles/summarize.py joins this with the code objects' register counts.) */
#define AIQMC_LDS_PROPOSAL 0   /* k_walker_rev, Metropolis proposals from the walker cache */
#define AIQMC_LDS_WALKER 1     /* k_walker_rev, walker launches / value + gradient */
#define AIQMC_LDS_ADJOINT 2    /* k_walker_rev<PREP>, local energy adjoint pass */
#define AIQMC_LDS_LAP 3        /* k_walker_lap, local energy first-derivative pass */
#define AIQMC_LDS_PGRAD 4      /* k_param_grad */
#define AIQMC_LDS_FWDLAP 5     /* k_walker<LAP>, forward-Laplacian diagnostics */
int aiqmc_debug_launch_lds(int32_t nelectrons, int32_t natoms, int32_t dtype, int32_t kind, int32_t* bytes,
                           int32_t* waves);

/* Diagnostics (host only, launches nothing): the kernel a walker launch of `kind` over nconf
 * configurations reaches with this context's shape, dtype and current aiqmc_debug_set_* switches,
 * as the row number (1..8) of the table above walker_launch in csrc/shape.hip.  kind:
 * AIQMC_LAUNCH_* (aq::Launch of csrc/launch_route.h, which holds the routing); nconf matters to
 * AIQMC_LAUNCH_SWEEP_WALKER alone (small fp32 batches run two waves per walker). */
#define AIQMC_LAUNCH_WALKER_VALUE 0     /* aiqmc_logpsi, the observables' and the ECP quadrature's walker launch */
#define AIQMC_LAUNCH_WALKER_ORBITALS 1  /* aiqmc_orbitals */
#define AIQMC_LAUNCH_WALKER_GRAD 2      /* aiqmc_logpsi_grad, the DMC drift-diffusion's post-move gradient */
#define AIQMC_LAUNCH_SWEEP_WALKER 3     /* the walker launch of a Metropolis sweep */
#define AIQMC_LAUNCH_PROPOSAL 4         /* the proposal launch of a Metropolis sweep */
#define AIQMC_LAUNCH_QUADRATURE 5       /* the ECP quadrature's value launch */
#define AIQMC_LAUNCH_LAP_FORWARD 6      /* aiqmc_debug_local_energy_forward */
#define AIQMC_LAUNCH_GRAD_FORWARD 7     /* aiqmc_debug_logpsi_grad_forward */
int aiqmc_debug_launch_row(aiqmc_ctx* ctx, int32_t kind, int32_t nconf, int32_t* row);

/* Diagnostics: walker launches of systems with N <= 8 electrons run several walkers per wave
 * (default, on = 1: four for N <= 4, two for N <= 8); on = 0 runs one wave per walker.
 * Results agree to rounding. */
int aiqmc_debug_set_packed_walkers(aiqmc_ctx* ctx, int32_t on);

/* Diagnostics: the ECP quadrature's value launch for N <= 8 (k_quad_value) factors each displaced
 * configuration's matrix in its walker's recorded pivot order and re-runs partial pivoting only for
 * a configuration whose pivot falls below 0.1 of the walker's; on = 1 takes partial pivoting for
 * every configuration (the fallback path everywhere).  Results agree to rounding. */
int aiqmc_debug_set_quad_pivoted(aiqmc_ctx* ctx, int32_t on);

/* Diagnostics: in fp32, aiqmc_mc_step can sum the two limdrift reductions of each sweep
 * (|grad|^2 over the walkers, over the proposals; VMCmcstep.py:11-14) inside the walker and
 * proposal launches, as exact 64-bit integer sums of |grad|^2 in units of 2^-16: no reduction
 * launches, and the same bits in any arrival order.  mode 1 (default) and 2 = always (mode 1
 * limited it to batches of at most 1,024 walkers before round 4), 0 = never: reduction launches that sum the same
 * integers in 32 workgroups (k_taueff_part; the same bits as the fused sums), 3 = never, with the
 * single-workgroup fp64 tree sum (k_taueff; fp64 always uses it; results agree with the integer
 * sums to the float rounding of v2). */
int aiqmc_debug_set_fuse_reduce(aiqmc_ctx* ctx, int32_t on);

/* Diagnostics: the fp32 limdrift factor (VMCmcstep.py:11-14) of n per-configuration |grad|^2
 * values (device floats `sumsq`) through one of the reductions aiqmc_mc_step uses: mode 0 = the
 * fused integer accumulators (tacc_add + taueff_wave), 1 = k_taueff_part + taueff_wave, 2 = the
 * fp64 tree sum (k_taueff).  Writes the factor to the HOST double *out (synchronises `stream`).
 * Non-finite values give NaN, as the reference's float sum does; huge ones a small factor. */
int aiqmc_debug_limdrift_factor(aiqmc_ctx* ctx, const void* sumsq, int32_t n, double tstep, int32_t mode,
                                double* out, void* stream);

/* Diagnostics: read back the draws the last AIQMC_RNG_PHILOX call left in the context, to compare
 * them with a host replica of the generator (oracle/philox.py).  which: 0 = gauss1 [B][3N],
 * 1 = gauss2 [B][N][3], 2 = u [B][N] (the last sweep of aiqmc_mc_step / aiqmc_dmc_drift_diffusion),
 * 3 = the rotations [B][3][3] of aiqmc_local_energy_ecp* / aiqmc_dmc_tmoves.  A stream-ordered
 * device-to-device copy of `count` elements of the context's dtype to the device buffer dst; no
 * kernel is launched and no state changes.  AIQMC_EINVAL for a null context or destination, a
 * negative count, an unknown `which`, or more elements than the buffer holds (an unallocated
 * buffer holds none). */
int aiqmc_debug_read_draws(aiqmc_ctx* ctx, int32_t which, void* dst, int64_t count, void* stream);

/* Development builds (-DAQ_ABLATE) only: skip proposal-kernel phases (bit mask, walker_rev.h) to
 * time their marginal cost; results are meaningless.  No effect in product builds. */
int aiqmc_debug_set_ablate(aiqmc_ctx* ctx, int32_t mask);

/* Diagnostics: shader-clock cycles per phase of the reverse-mode kernel, summed
 * over waves since the last call ([0..15] walker, [16..31] proposal launches);
 * all zero unless the library was built with -DAQ_PHASE_PROF. */
int aiqmc_debug_phase_cycles(aiqmc_ctx* ctx, uint64_t* out32);

/* Bytes of device workspace the context holds (for memory planning). */
int64_t aiqmc_workspace_bytes(const aiqmc_ctx* ctx);

const char* aiqmc_last_error(void);

/* Compile-time list of supported (N, A) shapes, as "N:A,N:A,...". */
const char* aiqmc_supported_shapes(void);

#ifdef __cplusplus
}
#endif
#endif /* AIQMC_H_ */
