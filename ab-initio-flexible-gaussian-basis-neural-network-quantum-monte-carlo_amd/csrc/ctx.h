// ctx.h -- host-side context + per-shape dispatch table.  It includes the launch ABI (kargs.h) and
// no header with a kernel or device function in it, so a unit sees the kernels it includes itself
// and no others.  Of the kernels' side it brings layout.h alone (through param_map.h: the offsets
// of Lay<N,A>, plain constants that the parameter map walks), so a layout change still rebuilds
// every unit.
//
// Who includes what (the one list; api_util.h, host_shared.h and the Makefile point here):
//   api_util.h (which includes this file, and with it devbuf.h, kargs.h, launch_route.h,
//   param_map.h and layout.h): every unit
//     with a context     aiqmc, dmc, debug, observables, rdm, components, density, corrsamples
//     context-free       loss, sr_gram, blocking
//     per shape          shape.hip
//   host_shared.h        aiqmc, dmc, debug, observables, rdm (it brings ecp_args.h)
//   reduce.h             aiqmc, dmc, loss, corrsamples
//   kernel headers       jets.h: aiqmc, observables, rdm (and dmc through ecp.h); limdrift.h: aiqmc,
//                        debug; ecp.h: aiqmc, dmc; walker_fwd.h, walker_rev.h, walker_lap.h,
//                        walker_pgrad.h, quad_small.h (with gj.h, electron.h): shape.hip alone
//   none of them         components, density, corrsamples, loss, sr_gram, blocking
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>
#include <string>
#include <utility>
#include <vector>

#include "aiqmc.h"
#include "devbuf.h"
#include "kargs.h"
#include "launch_route.h"
#include "param_map.h"

using aq::KArgs;
// aiqmc_profile_read's slots: the launches that timed() brackets (the numbers are the C-ABI's)
enum ProfSlot { PROF_PROPOSAL = 0, PROF_SWEEP_WALKER = 1, PROF_LOCAL_ENERGY = 2, PROF_QUADRATURE = 3, AIQMC_PROF_SLOTS };

struct aiqmc_ctx {
  int N = 0, A = 0, nup = 0, ndn = 0, dtype = 0, device = 0;
  int npar = 0, nanti = 0;
  std::vector<double> atoms, charges;
  std::vector<int> up, dn, par, anti;
  // the canonical <-> kernel-layout parameter map (param_map.h), built once by aiqmc_create: the
  // program of both parameter uploads and the index map of the parameter gradient
  ParamMap pmap;
  int64_t ncanon = 0, nkern = 0, nprm = 0;   // pmap's; nprm: device parameter buffer (nkern + lane-order copies)
  // Device memory: every buffer is a DevBuf (devbuf.h), sized where it is used by reserve() and
  // freed with the context.  aiqmc_workspace_bytes counts the groups marked [counted].
  DevBuf d_prm, d_rowsrc;
  bool params_set = false;
  // [counted] sweep workspace (ensure_ws), per batch: these twelve
  DevBuf d_grad, d_lp, d_sq, d_lpn, d_gown, d_sqn;
  DevBuf d_g1, d_g2, d_u;                                   // per-sweep Philox draws
  DevBuf d_wc, d_ec;                                        // Metropolis caches (walker_rev.h WCache/ECache)
  DevBuf d_taueff;                                          // the two limdrift factors (double[2])
  DevBuf d_lc;                                              // [counted] local-energy LapCache [B][lcache_n]
  DevBuf d_wcp;                                             // per-proposal cache scratch (reuse off)
  DevBuf d_cx;                                              // complex E_L scratch [B][6N+1]: grad log|psi|,
                                                            // grad theta, lap theta
  bool reuse = true;                                        // proposals reuse the walker's cached stage
  int ablate = 0;                                           // AQ_ABLATE development builds (walker_rev.h)
  int fuse_accept = 1;                                      // acceptance fused into the next walker launch
  int walker_fixed_gj = 1;                                  // walker launches re-use the previous sweep's pivot order
  int quad_pivoted = 0;                                     // k_quad_value: partial pivoting for every slot (test)
  int packed_walkers = 1;                                   // N <= 8 walker launches several per wave
  int fuse_reduce = 1;                                      // fp32 mc_step: limdrift sums by integer atomics
  int wide_reduce = 1;                                      // unfused fp32 sweeps: k_taueff_part (0: k_taueff)
  DevBuf d_tpart;                                           // their per-sweep partial sums [nsteps][2][TPART]
  DevBuf d_tacc;                                            // their per-sweep accumulators [2 banks][tacc_n][2]
  int tacc_n = 0;                                           // sweeps per bank: d_tacc's bank stride (layout
                                                            // state, set when d_tacc is reallocated)
  int tacc_bank = 0;                                        // the bank the next mc_step call uses
  bool tacc_clean[2] = {false, false};                      // bank zeroed (by the last k_accept of a call)
  int lap_waves = 0;                                        // waves per walker of k_walker_lap (0: by batch)
  int ncu = 256;                                            // compute units of the device
  bool env_walk_split = true, env_quad_grad = true;         // AIQMC_WALK_SPLIT / AIQMC_QUAD_GRAD not 0 (aiqmc_create)
  // pseudopotential (aiqmc_set_ecp / aiqmc_local_energy_ecp, ecp.h)
  bool ecp_set = false;
  int ecp_KL = 0, ecp_KN = 0, ecp_L = 0;
  bool ecp_nl_zero = false;   // every nonlocal coefficient 0 (all-electron through the pp path)
  DevBuf d_ecp_tab;
  // [counted] ECP workspace (ensure_ecp_ws), per batch
  DevBuf d_ecp_rot, d_ecp_x, d_ecp_lq, d_ecp_pq, d_ecp_ec, d_ecp_el, d_ecp_lp0, d_ecp_ph0;
  DevBuf d_tm_scr;                 // T-moves per-walker amplitudes [B][N*A*50][4]
  DevBuf d_dscr;                   // DMC reduction scratch: block partial sums / cut minima [2*64]
  // parameter gradients (aiqmc_logpsi_param_grad, walker_pgrad.h)
  DevBuf d_gmap;                   // int [ncanon] pmap.gmap, uploaded on first use
  DevBuf d_wnorm;                  // double [6] |W_y row| of the current parameters
  // device copy of pmap.op / src / cval [nprm], uploaded by the first aiqmc_set_params_device:
  // per kernel-layout entry an op (0 constant, 1 copy, 2 row-normalised y coefficient), its
  // canonical source index and its constant value
  DevBuf d_pk_op, d_pk_src, d_pk_cval;
  DevBuf d_pg;                     // [B][nkern] per-walker kernel-layout gradients
  DevBuf d_pgr;                    // [max(nw, 2)][nkern] weighted sums, then k_grad_partial's chunk sums
  // [counted] observables (aiqmc_spin_squared, observables.hip): one chunk of exchanged
  // configurations [n][3N], their log|psi| and phase [n], and the value launch's walker cache
  DevBuf d_obs_x, d_obs_lp, d_obs_ph, d_obs_wc;
  int obs_chunk = 4096;              // configurations per value launch (aiqmc_debug_set_obs_chunk)
  // one-body density matrix (aiqmc_set_rdm_basis / aiqmc_rdm_accumulate, rdm.hip).  The tables
  // are the context's, as the ECP table is: d_rdm_tab doubles (shell centres [nshell][3], primitive
  // exponents and coefficients [nprim] each, MO coefficients [2][nao][norb] when rdm_mo, then q:
  // centres [nq][3], 1 / (2 sigma^2), p (2 pi sigma^2)^-3/2, sigma, cumulative p: [nq] each),
  // d_rdm_shell ints [nshell][4] = (l, first primitive, primitives, first function)
  bool rdm_set = false, rdm_mo = false;
  int rdm_nshell = 0, rdm_nprim = 0, rdm_nao = 0, rdm_norb = 0, rdm_nq = 0;
  DevBuf d_rdm_tab, d_rdm_shell;
  // its chunk workspace beside d_obs_*: points r' [W][S][3] and 1/q [W][S], basis values at the
  // electrons [W][N][K] and at the points [2][W][S][K], ratio factors [W][S][N][2], the group
  // tiles [groups][2][K][K][2] (all in the context dtype) and the group weight sums (double)
  DevBuf d_rdm_rp, d_rdm_iq, d_rdm_pe, d_rdm_pp, d_rdm_f, d_rdm_tile, d_rdm_wsum;
  // [counted] energy components (aiqmc_energy_components, components.hip), per batch: the
  // all-electron E_L [B], an imaginary part [B], grad log|psi| [B][3N]
  DevBuf d_comp;
  // optional per-kernel HIP-event timing (aiqmc_profile_*): slot -> recorded (start, stop) pairs
  bool prof = false;
  std::vector<hipEvent_t> ev_free;
  std::vector<std::pair<hipEvent_t, hipEvent_t>> ev_used[AIQMC_PROF_SLOTS];
};

// bytes per element of the context's dtype
inline size_t elem_size(const aiqmc_ctx* c) { return c->dtype == AIQMC_F32 ? 4 : 8; }

// One walker launch: what it is, the host's options of the routing (launch_route.h) and the kernel
// arguments.  Built by launch_args (api_util.h); a call site adds its outputs to ka.
struct WalkerCall {
  aq::Launch kind;
  aq::LaunchOpts opts;
  KArgs ka;
};

struct ShapeOps {
  int (*set_lds)();
  void (*walker)(int dtype, const WalkerCall& w, int nconf, hipStream_t s);   // the kernel of route(w.kind, ..., w.opts)
  void (*accept)(int dtype, void* pos, const aq::AccArgs& a, int B, hipStream_t s);
  void (*moved)(int dtype, const KArgs& ka, hipStream_t s);   // k_moved_electron over ka.nconf proposals
  // local energy: adjoint pass (k1) + first-derivative pass (k2), walker_lap.h
  void (*lap)(int dtype, const KArgs& k1, const KArgs& k2, int nconf, int waves, int phase, hipStream_t s);
  void (*phase_read)(unsigned long long* out32);               // AQ_PHASE_PROF builds only
  int wcache_n, ecache_n;                                      // cache entries per walker / per proposal
  int lcache_n;                                                // LapCache entries per walker
  void (*param_map)(const aiqmc_ctx* c, ParamMap& m);          // build_param_map from the context's tables
  int (*pgrad)(int dtype, const KArgs& ka, int nconf, hipStream_t s);   // k_param_grad
  // dynamic LDS bytes per workgroup of the launches that take it, [dtype f32, f64][kind]
  // (kind: AIQMC_LDS_* of aiqmc.h), and the waves per workgroup of each: what a profiler's
  // dispatch record does not show (rocprofv3 reports the static group segment only)
  int dyn_lds[2][6];
  int wg_waves[2][6];
};

// aiqmc.hip: the dispatch table of a built shape
bool aiqmc_shape_ops(int N, int A, ShapeOps* ops);
