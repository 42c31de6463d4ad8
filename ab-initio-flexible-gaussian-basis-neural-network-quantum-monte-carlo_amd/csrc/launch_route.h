// launch_route.h -- which wavefront kernel a walker launch (ShapeOps::walker) reaches, as a function
// of what the call site means (Launch) and a few host options (LaunchOpts).  Nothing of HIP: the
// host compiler checks it against the field-pattern predicate it replaced
// (tests/host/launch_route_check.cpp).  The kernels, grids and LDS sizes of the rows are in
// shape.hip (walker_launch), one case each.
#pragma once

namespace aq {

// What a call site launches.  The KArgs builder (api_util.h launch_args) sets the fields a kind implies.
enum class Launch : int {
  WalkerValue = 0,   // log|psi| (+ phase) at the walkers: aiqmc_logpsi, obs_values, ecp_quadrature's walker launch
  WalkerOrbitals,    // ... value only, with the orbital matrix: aiqmc_orbitals
  WalkerGrad,        // log|psi| and its gradient: aiqmc_logpsi_grad, the post-move gradient of the DMC drift-diffusion
  SweepWalker,       // step (1) of mc_sweep: the gradient + draws, fused acceptance, pivot re-use
  Proposal,          // step (3) of mc_sweep: the B*N single-electron moves, value + own gradient
  Quadrature,        // ecp_quadrature: single-electron moves to the quadrature points, value only
  LapForward,        // forward-mode Laplacian (aiqmc_debug_local_energy_forward)
  GradForward,       // forward-mode gradient (aiqmc_debug_logpsi_grad_forward)
};
constexpr int LAUNCH_KINDS = 8;

// The kernels of shape.hip's walker_launch; the numbers are what aiqmc_debug_launch_row reports.
enum class Row : int {
  QuadValue = 1,    // k_quad_value<T>: packed quadrature values
  QuadGrad = 2,     // k_quad_grad<T>: packed proposals
  QuadWalker = 3,   // k_quad_grad<T, walker>: packed walkers
  LapFwd = 4,       // k_walker<T, MODE_LAP>
  RevProp = 5,      // k_walker_rev<T, PROP>: proposals from the walker cache
  RevSplit = 6,     // k_walker_rev<float, SPL>: two waves per walker (instantiated for float alone)
  Rev = 7,          // k_walker_rev<T>
  GradFwd = 8,      // k_walker<T, MODE_GRAD>
};

// The host's side of the choice; travels beside KArgs, no kernel sees it.
struct LaunchOpts {
  bool packed = true;          // aiqmc_debug_set_packed_walkers: N <= 8 walkers several per wave
  bool reuse = true;           // aiqmc_debug_set_proposal_reuse: single-electron moves from the walker cache
  bool ablate = false;         // aiqmc_debug_set_ablate mask != 0 (AQ_ABLATE builds: k_walker_rev<PROP> alone skips phases)
  bool split = false;          // mc_sweep: the batch leaves SIMDs idle (fp32 and B <= AQ_WALK_SPLIT_PER_CU * ncu)
  bool env_split = true;       // AIQMC_WALK_SPLIT not 0
  bool env_quad_grad = true;   // AIQMC_QUAD_GRAD not 0
};

//  kind                        options, N                                                row
//  LapForward                  --                                                        4 LapFwd
//  GradForward                 --                                                        8 GradFwd
//  WalkerOrbitals              --                                                        7 Rev
//  Quadrature                  reuse off                                                 7 Rev
//                              N <= 8                                                    1 QuadValue
//                              otherwise                                                 5 RevProp
//  Proposal                    reuse off                                                 7 Rev
//                              N <= 8, no ablate, not (N > 4 and AIQMC_QUAD_GRAD=0)      2 QuadGrad
//                              otherwise                                                 5 RevProp
//  WalkerValue, WalkerGrad,    N <= 8, packed                                            3 QuadWalker
//  SweepWalker
//  SweepWalker                 fp32, split, not AIQMC_WALK_SPLIT=0                       6 RevSplit
//  the walker kinds            otherwise                                                 7 Rev
// (Quadrature has no ablate or AIQMC_QUAD_GRAD exception; packed is tested before split, so sweep
// walkers of N <= 8 are packed, not split.)
inline Row route(Launch kind, bool is_f32, int N, const LaunchOpts& o) {
  switch (kind) {
    case Launch::LapForward: return Row::LapFwd;
    case Launch::GradForward: return Row::GradFwd;
    case Launch::WalkerOrbitals: return Row::Rev;
    case Launch::Quadrature:
      if (!o.reuse) return Row::Rev;
      return N <= 8 ? Row::QuadValue : Row::RevProp;
    case Launch::Proposal:
      if (!o.reuse) return Row::Rev;
      return (N <= 8 && !o.ablate && (N <= 4 || o.env_quad_grad)) ? Row::QuadGrad : Row::RevProp;
    case Launch::SweepWalker:
      if (N <= 8 && o.packed) return Row::QuadWalker;
      return (is_f32 && o.split && o.env_split) ? Row::RevSplit : Row::Rev;
    case Launch::WalkerValue:
    case Launch::WalkerGrad: break;
  }
  return (N <= 8 && o.packed) ? Row::QuadWalker : Row::Rev;
}

}  // namespace aq
