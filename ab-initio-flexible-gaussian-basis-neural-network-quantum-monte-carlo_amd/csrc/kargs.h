// kargs.h -- the launch ABI: the plain structs the host fills and every wavefront kernel takes by
// value (KArgs, with the acceptance's AccArgs inside it), and the word layout of the limdrift
// accumulators both sides index.  Nothing of HIP: the host compiler checks the frozen layout
// (tests/host/launch_abi_check.cpp).  EcpArgs, the pp kernels' struct, is in ecp_args.h.
#pragma once
#include <cstddef>
#include <cstdint>

namespace aq {

// Fused limdrift accumulators: per sweep and kind (0: walkers, 1: proposals) TACC_STRIDE 64-bit
// words, TACC_SLOTS "lo" slots in units of 1 / TACC_SCALE (a configuration adds to slot
// configuration mod TACC_SLOTS), then the shared words mid, hi and bad, then zeros.  What the words
// hold, their range and the functions that add to and read them are in limdrift.h.
constexpr double TACC_SCALE = 65536.0;
#ifndef AQ_TACC_SLOTS
#define AQ_TACC_SLOTS 256
#endif
constexpr int TACC_SLOTS = AQ_TACC_SLOTS;      // a power of two >= 64
static_assert(TACC_SLOTS >= 64 && (TACC_SLOTS & (TACC_SLOTS - 1)) == 0, "TACC_SLOTS");
constexpr int TACC_STRIDE = TACC_SLOTS + 64;   // per kind: lo slots, then [mid, hi, bad, 0 ...]
constexpr int TACC_MID = TACC_SLOTS, TACC_HI = TACC_SLOTS + 1, TACC_BAD = TACC_SLOTS + 2;
constexpr int TACC_MAX_CONF = 1 << 24;          // configurations per reduction (lo / mid headroom)
// Unfused fp32 sweeps: the TPART partial sums of k_taueff_part, per kind [4][TPART] = lo, mid, hi,
// bad (the same integers as the fused accumulators; limdrift.h taueff_wave sums them)
constexpr int TPART = 32;
constexpr int TPART_KIND = 4 * TPART;

// What the acceptance of one sweep reads (limdrift.h accept_one), by k_accept or, fused, by the next
// sweep's walker launch (KArgs::acc)
struct AccArgs {
  const void* grad;       // [B][3N]
  const void* lp;         // [B]
  const void* lpn;        // [B][N]
  const void* gown;       // [B][N][3]
  const void* gauss1;     // [B][3N]
  const void* gauss2;     // [B][N][3]
  const void* u;          // [B][N]
  const double* taueff;   // [2]
  const unsigned long long* tacc;   // [2][TACC_STRIDE] fused accumulators of the sweep (nullptr: taueff)
  const unsigned long long* tpart;  // [2][TPART_KIND] k_taueff_part sums of the sweep (unfused fp32), or nullptr
  double tstep;
  int32_t* count;         // [B] accepted moves (optional)
  // k_accept only (the last sweep of aiqmc_mc_step): words of the OTHER bank of fused limdrift
  // accumulators to zero for the next call (no memset launch per call; aiqmc.hip tacc banks)
  unsigned long long* zero = nullptr;
  int32_t nzero = 0;
};
// The layout the kernels were compiled against (it is embedded in KArgs)
static_assert(sizeof(AccArgs) == 112 && offsetof(AccArgs, grad) == 0 && offsetof(AccArgs, lp) == 8 &&
                  offsetof(AccArgs, lpn) == 16 && offsetof(AccArgs, gown) == 24 && offsetof(AccArgs, gauss1) == 32 &&
                  offsetof(AccArgs, gauss2) == 40 && offsetof(AccArgs, u) == 48 && offsetof(AccArgs, taueff) == 56 &&
                  offsetof(AccArgs, tacc) == 64 && offsetof(AccArgs, tpart) == 72 && offsetof(AccArgs, tstep) == 80 &&
                  offsetof(AccArgs, count) == 88 && offsetof(AccArgs, zero) == 96 && offsetof(AccArgs, nzero) == 104,
              "AccArgs layout changed");

struct KArgs {
  int nconf;
  int nup;
  const int* rowsrc;      // [N]: electron feeding determinant row r (up rows then down rows)
  const void* prm;        // kernel parameter layout (Lay<N,A>)
  const void* pos;        // direct: [nconf][3N]; proposal: walkers [B][3N]
  // proposal mode: configuration conf = b*N + i is walker b with electron i moved
  // by  grad_eff*tstep + sqrt(tstep)*gauss1  (VMCmcstep.py:58-78)
  int proposal;
  const void* pgrad;      // [B][3N] grad log|psi| at the walkers
  const void* gauss1;     // [B][3N] standard normals (host draws or k_draws output)
  const double* taueff;   // device scalar: limdrift factor of pgrad (VMCmcstep.py:11-14)
  // fused limdrift accumulators of the sweep [2][TACC_STRIDE] (fp32 mc_step; nullptr elsewhere):
  // walker launches add their |grad|^2 to kind 0, proposal launches to kind 1; readers of the
  // walker factor (moved electron, proposals from scratch) sum kind 0 (taueff_wave)
  unsigned long long* tacc;
  const unsigned long long* tpart;   // [2][TPART_KIND] partial sums of k_taueff_part (read by taueff_wave)
  double tstep;
  uint64_t seed, step;
  // single-electron-move layout (proposal != 0, k_walker_rev / k_moved_electron): configuration
  // conf is walker conf / mper with electron (conf % mper) / mdiv moved; 0 means mper = N,
  // mdiv = 1 (the Metropolis proposals).  xnew [nconf][3]: the moved electron's position
  // (ECP quadrature points); nullptr: x + limdrift(grad) tstep + sqrt(tstep) gauss1.
  int mper, mdiv;
  const void* xnew;
  int value_only;         // k_walker_rev: log|psi| and phase only (no backward pass)
  void* orb;              // k_walker_rev value_only: the orbital matrix [nconf][N][N][re,im] (nn.py:409-506)
  int ablate;             // -DAQ_ABLATE development builds only: proposal phases to skip (walker_rev.h)
  int phase_grad;         // k_param_grad: d phase / d theta instead of d log|psi| / d theta
  // walker launch of a Metropolis sweep (k_walker_rev, PROP = false): dg1/dg2/du != nullptr:
  // lanes e < N of wave b write the sweep's Philox draws of walker b exactly as k_draws would
  // (one launch fewer per sweep).  (Fusing the limdrift reduction the same way, by the last wave
  // to finish, was measured 3.5x slower: every wave's device-scope fence writes back its L2.)
  void *dg1, *dg2, *du;
  // walker launch of a Metropolis sweep: acc.lpn != nullptr: first apply the PREVIOUS sweep's
  // acceptance to walker conf (fused k_accept; one launch fewer per sweep)
  AccArgs acc;
  // walker launch of a Metropolis sweep after the first of an mc_step call: the walker cache holds
  // this walker's pivot record of the previous sweep; the Gauss-Jordan re-uses that order (the
  // pivoted elimination only if a pivot comes out small)
  int pvok;
  // reserved: no kernel reads these two ints and the host leaves them 0 (they held host-side routing
  // switches, now LaunchOpts of launch_route.h).  They keep the offsets of the fields below, which
  // the static_assert under this struct freezes; a kernel-side change may drop them.
  int reserved0;
  int reserved1;
  // k_quad_value: every slot takes the partial-pivoting LU, not the walker's order (aiqmc_debug_set_quad_pivoted)
  int quad_pivoted;
  // Metropolis caches (walker_rev.h WCache / ECache); nullptr outside aiqmc_mc_step
  void* wcache;
  void* ecache;
  // local-energy launch pair (walker_lap.h LapCache); nullptr elsewhere
  void* lapcache;
  // outputs (nullable)
  void* logabs;           // [nconf]
  void* phase;            // [nconf]
  void* grad;             // [nconf][3N]
  void* el;               // [nconf]
  void* sumsq;            // [nconf] |grad|^2
  void* gown;             // [nconf][3]  proposal: gradient components of the moved electron
};
// The layout the kernels were compiled against: KArgs keeps its size and the offsets of what follows
// its reserved pair until a kernel-side change moves them on purpose.
static_assert(sizeof(KArgs) == 368 && offsetof(KArgs, reserved0) == 284 && offsetof(KArgs, reserved1) == 288 &&
                  offsetof(KArgs, quad_pivoted) == 292 && offsetof(KArgs, wcache) == 296 && offsetof(KArgs, ecache) == 304 &&
                  offsetof(KArgs, lapcache) == 312 && offsetof(KArgs, logabs) == 320 && offsetof(KArgs, phase) == 328 &&
                  offsetof(KArgs, grad) == 336 && offsetof(KArgs, el) == 344 && offsetof(KArgs, sumsq) == 352 &&
                  offsetof(KArgs, gown) == 360,
              "KArgs layout changed");

}  // namespace aq
