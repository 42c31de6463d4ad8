// launch_route_check.cpp -- stand-alone host check of csrc/launch_route.h (built and run by
// tests/test_capi_cpu.py::test_launch_route_host_check under -fsanitize=address,undefined).
// route(kind, dtype, N, options) against the first-match predicate over KArgs fields that chose the
// kernel before the launch kind was named: old_row below is that `if` chain as it stood in
// shape.hip (quad_small, then walker_launch), and mock_of the field pattern each kind's call
// site produced (base_args / walker_args / proposal_args and what the call site added).
#include <cstdio>

#include "launch_route.h"

using namespace aq;

static int g_bad = 0;
#define REQ(cond, ...)                           \
  do {                                           \
    if (!(cond)) {                               \
      if (++g_bad <= 40) {                       \
        std::printf("FAIL %s: ", #cond);         \
        std::printf(__VA_ARGS__);                \
        std::printf("\n");                       \
      }                                          \
    }                                            \
  } while (0)

enum { MODE_GRAD = 1, MODE_LAP = 2, MODE_GRAD_FWD = 3 };

// the fields the old dispatch read: the mode argument of ops.walker and the KArgs members
struct Mock {
  int mode = MODE_GRAD;
  bool proposal = false, ecache = false, wcache = false, value_only = false, orb = false, lapcache = false;
  bool ablate = false, one_wave = false, walk_split = false;
};

static Mock mock_of(Launch kind, const LaunchOpts& o) {
  Mock m;
  m.one_wave = !o.packed;   // base_args: every launch
  switch (kind) {
    case Launch::WalkerValue:   // aiqmc_logpsi, obs_values, ecp_quadrature's walker launch: walker_args + phase
    case Launch::WalkerGrad:    // aiqmc_logpsi_grad, the DMC post-move gradient: walker_args + grad
      m.wcache = true;
      break;
    case Launch::WalkerOrbitals:   // aiqmc_orbitals
      m.wcache = m.value_only = m.orb = true;
      break;
    case Launch::SweepWalker:   // mc_sweep (1): walker_args, walk_split by the batch (and fp32)
      m.wcache = true;
      m.walk_split = o.split;
      break;
    case Launch::Proposal:   // mc_sweep (3): proposal_args, kp.ablate = c->ablate
      m.proposal = m.wcache = true;
      m.ecache = o.reuse;
      m.ablate = o.ablate;
      break;
    case Launch::Quadrature:   // ecp_quadrature: proposal_args, value_only; ablate stays 0
      m.proposal = m.wcache = m.value_only = true;
      m.ecache = o.reuse;
      break;
    case Launch::LapForward:   // conf_args, MODE_LAP
      m.mode = MODE_LAP;
      break;
    case Launch::GradForward:   // conf_args, MODE_GRAD_FWD
      m.mode = MODE_GRAD_FWD;
      break;
  }
  return m;
}

static int old_row(const Mock& ka, bool f32, int N, bool env_split, bool env_quad_grad) {
  const bool quad_grad_off = !env_quad_grad && N > 4;
  if (ka.mode == MODE_GRAD) {   // quad_small
    if (N <= 8 && ka.proposal && ka.ecache && ka.value_only && !ka.orb) return 1;
    if (N <= 8 && ka.proposal && ka.ecache && !ka.value_only && !ka.orb && !ka.ablate && !quad_grad_off) return 2;
    if (N <= 8 && !ka.proposal && ka.wcache && !ka.value_only && !ka.orb && !ka.lapcache && !ka.one_wave) return 3;
  }
  if (ka.mode == MODE_LAP) return 4;
  if (ka.mode == MODE_GRAD && ka.proposal && ka.ecache) return 5;
  if (ka.mode == MODE_GRAD) {
    if (f32 && ka.walk_split && !ka.proposal && !ka.value_only && env_split) return 6;
    return 7;
  }
  return 8;
}

int main() {
  int reached[9] = {0};
  long cases = 0;
  for (int k = 0; k < LAUNCH_KINDS; ++k)
    for (int N = 2; N <= 16; ++N)
      for (int f32 = 0; f32 < 2; ++f32)
        for (int bits = 0; bits < 64; ++bits) {
          LaunchOpts o;
          o.packed = bits & 1;
          o.reuse = bits & 2;
          o.ablate = bits & 4;
          o.split = bits & 8;
          o.env_split = bits & 16;
          o.env_quad_grad = bits & 32;
          const Launch kind = (Launch)k;
          const int got = (int)route(kind, f32 != 0, N, o);
          const int want = old_row(mock_of(kind, o), f32 != 0, N, o.env_split, o.env_quad_grad);
          REQ(got == want, "kind %d N %d f32 %d options %d: route %d, the field predicate %d", k, N, f32, bits, got, want);
          REQ(got >= 1 && got <= 8, "kind %d N %d f32 %d options %d: row %d", k, N, f32, bits, got);
          if (got >= 1 && got <= 8) ++reached[got];
          REQ(!(N > 8 && got >= 1 && got <= 3), "kind %d N %d: packed row %d for N > 8", k, N, got);
          REQ(!(got == 6 && !f32), "kind %d N %d: the fp32-only row for fp64", k, N);
          ++cases;
        }
  for (int r = 1; r <= 8; ++r) REQ(reached[r] > 0, "row %d is never reached", r);
  // the corners of the table, by hand
  LaunchOpts d;
  LaunchOpts abl = d, noqg = d, nore = d, unpacked = d, split = d, split_env0 = d;
  abl.ablate = true;
  noqg.env_quad_grad = false;
  nore.reuse = false;
  unpacked.packed = false;
  split.split = true;
  split_env0.split = true, split_env0.env_split = false;
  REQ(route(Launch::Proposal, true, 8, abl) == Row::RevProp, "ablated proposals take row 5");
  REQ(route(Launch::Proposal, true, 4, noqg) == Row::QuadGrad && route(Launch::Proposal, true, 5, noqg) == Row::RevProp &&
          route(Launch::Proposal, true, 8, noqg) == Row::RevProp && route(Launch::Proposal, true, 9, noqg) == Row::RevProp,
      "AIQMC_QUAD_GRAD=0 moves 5 <= N <= 8 alone");
  REQ(route(Launch::Quadrature, false, 8, abl) == Row::QuadValue && route(Launch::Quadrature, false, 8, noqg) == Row::QuadValue,
      "the quadrature has no ablate / AIQMC_QUAD_GRAD exception");
  REQ(route(Launch::SweepWalker, true, 8, split) == Row::QuadWalker, "N <= 8 sweep walkers are packed, not split");
  REQ(route(Launch::SweepWalker, true, 9, split) == Row::RevSplit && route(Launch::SweepWalker, false, 9, split) == Row::Rev &&
          route(Launch::SweepWalker, true, 9, split_env0) == Row::Rev && route(Launch::SweepWalker, true, 9, d) == Row::Rev &&
          route(Launch::WalkerGrad, true, 9, split) == Row::Rev,
      "row 6: fp32, SweepWalker, split, AIQMC_WALK_SPLIT not 0");
  unpacked.split = true;
  REQ(route(Launch::SweepWalker, true, 8, unpacked) == Row::RevSplit, "unpacked N <= 8 sweep walkers may split");
  REQ(route(Launch::Proposal, true, 4, nore) == Row::Rev && route(Launch::Quadrature, true, 14, nore) == Row::Rev,
      "reuse off: row 7");
  REQ(route(Launch::WalkerOrbitals, true, 4, d) == Row::Rev && route(Launch::WalkerOrbitals, false, 14, d) == Row::Rev,
      "orbitals: row 7");
  std::printf("launch_route_check: %d failures (%ld cases)\n", g_bad, cases);
  return g_bad ? 1 : 0;
}
