// ecp_args.h -- the launch struct of the pseudopotential and T-move kernels (ecp.h), which the host
// fills and every one of them takes by value.  Nothing of HIP, like kargs.h; the host compiler checks
// the frozen layout (tests/host/launch_abi_check.cpp).
#pragma once
#include <cstddef>
#include <cstdint>

namespace aq {

// Device tables (double): atoms [A][3], charges [A], then per atom KL local triplets
// (n, coefficient, exponent) and L*KN nonlocal triplets.
struct EcpArgs {
  int B, N, A, KL, KN, L;
  const double* tab;
  const void* pos;      // [B][3N]
  const void* rot;      // [B][9]
  const void* lp0;      // [B] log|psi| at the walker
  const void* ph0;      // [B] phase at the walker
  const void* lpq;      // [B][N][A][50] log|psi| at the quadrature configurations
  const void* phq;      // [B][N][A][50] phase
  const void* eall;     // [B] all-electron local energy (V_ee + V_en + V_nn + KE)
  void* e_re;           // [B] outputs
  void* e_im;
  void* xnew;           // k_ecp_points output [B*N*A*50][3]
  uint64_t seed, step;  // k_ecp_rot
  int skip_nl;          // k_ecp_energy: nonlocal coefficients all zero -- no quadrature was run
  int cdf_lds;          // k_tmove: dynamic LDS holds every electron's cdf row [N][A*50+1][2]
  // T-moves (k_tmove)
  double tstep;
  const void* usel;     // [B] selection uniform (NULL: Philox)
  const void* uacc;     // [B][N] acceptance uniforms (NULL: Philox)
  void* acc;            // [B][N] acceptance out (optional)
  void* pos_out;        // [B][3N] positions, updated in place
  double* scr;          // [B][N*A*50][4] forward amplitude (re, im), ratio (re, im)
};
// The layout the kernels were compiled against
static_assert(sizeof(EcpArgs) == 184 && offsetof(EcpArgs, B) == 0 && offsetof(EcpArgs, N) == 4 && offsetof(EcpArgs, A) == 8 &&
                  offsetof(EcpArgs, KL) == 12 && offsetof(EcpArgs, KN) == 16 && offsetof(EcpArgs, L) == 20 &&
                  offsetof(EcpArgs, tab) == 24 && offsetof(EcpArgs, pos) == 32 && offsetof(EcpArgs, rot) == 40 &&
                  offsetof(EcpArgs, lp0) == 48 && offsetof(EcpArgs, ph0) == 56 && offsetof(EcpArgs, lpq) == 64 &&
                  offsetof(EcpArgs, phq) == 72 && offsetof(EcpArgs, eall) == 80 && offsetof(EcpArgs, e_re) == 88 &&
                  offsetof(EcpArgs, e_im) == 96 && offsetof(EcpArgs, xnew) == 104 && offsetof(EcpArgs, seed) == 112 &&
                  offsetof(EcpArgs, step) == 120 && offsetof(EcpArgs, skip_nl) == 128 && offsetof(EcpArgs, cdf_lds) == 132 &&
                  offsetof(EcpArgs, tstep) == 136 && offsetof(EcpArgs, usel) == 144 && offsetof(EcpArgs, uacc) == 152 &&
                  offsetof(EcpArgs, acc) == 160 && offsetof(EcpArgs, pos_out) == 168 && offsetof(EcpArgs, scr) == 176,
              "EcpArgs layout changed");

}  // namespace aq
