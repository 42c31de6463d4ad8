// components.hip -- what the local energy is made of (aiqmc_energy_components): per walker
//   out[k][b], k = AIQMC_COMP_*:  total, kinetic, kinetic_grad, v_ee, v_en, v_nn, v_pp_local, v_pp_nonlocal
//
// The energies come from the existing entry points, called as they are: out[0] is written by
// aiqmc_local_energy / _complex (no ECP) or aiqmc_local_energy_ecp / _ecp_complex (ECP) straight into
// row 0, so it is their bits.  With an ECP the all-electron local energy of the same context
// (aiqmc_local_energy / _complex) is evaluated as well: the ECP entry's own all-electron intermediate
// (d_ecp_el) comes without the gradient, and with complex_output without the phase term of the
// kinetic energy, so both entry points are called.  The gradient of log|psi| is the one the
// local-energy launch returns (complex_output: the one it leaves in the d_cx scratch).
//
// One launch follows (k_energy_components): a group of 16 lanes per walker, 16 walkers per workgroup
// of 256.  The workgroup stages its walkers' pos and grad rows (one contiguous span) in LDS with
// coalesced reads; lane e of a group owns electron e:
//   v_ee        sum_{j > e} 1 / r_ej, j ascending
//   v_en        sum_a -Z_a / r_ea, a ascending
//   v_pp_local  sum_a sum_k c_ak r^(n_ak - 2) exp(-alpha_ak r^2), (a, k) ascending; r^2 the sum of squares
//   kin_grad    gx^2 + gy^2 + gz^2 of its electron
// with r = sqrt(dx^2 + dy^2 + dz^2), all in the context dtype; lanes e >= N hold 0.  An xor butterfly
// (8, 4, 2, 1) sums the group in a fixed order, so the four sums are a function of the walker's own
// coordinates alone: the same bits for any B, any batching and any position in the batch.  Lane 0
// then forms, in this order,
//   kinetic       = e_all - ((v_ee + v_en) + v_nn)
//   kinetic_grad  = 0.5 * kin_grad
//   v_pp_nonlocal = total - ((((kinetic + v_ee) + v_en) + v_nn) + v_pp_local)     (0 without an ECP)
// and the workgroup writes rows 1..7 through LDS, 16 consecutive walkers per row.  v_nn is summed on
// the host in double over a < b ascending and rounded to the dtype once.  No atomics; nothing is
// clamped: coincident particles give +-inf in that walker's columns only, NaN propagates.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <string>

#include "aiqmc.h"
#include "api_util.h"

namespace {

constexpr int COMP_G = 16;          // lanes per walker (N <= 16)
constexpr int COMP_WPB = 16;        // walkers per workgroup
constexpr int COMP_MAX_ATOMS = 5;   // the largest A of the shape list

// atoms and charges of the context, by value (A <= COMP_MAX_ATOMS)
struct CompSys {
  double atoms[COMP_MAX_ATOMS][3];
  double z[COMP_MAX_ATOMS];
};

__device__ __forceinline__ float c_sqrt(float x) { return sqrtf(x); }
__device__ __forceinline__ double c_sqrt(double x) { return sqrt(x); }
__device__ __forceinline__ float c_pow(float x, float y) { return powf(x, y); }
__device__ __forceinline__ double c_pow(double x, double y) { return pow(x, y); }
__device__ __forceinline__ float c_exp(float x) { return expf(x); }
__device__ __forceinline__ double c_exp(double x) { return exp(x); }

// e_tot = out row 0 (already written), e_all = the all-electron E_L (nullptr: e_tot), ecp_tab = the
// context's pseudopotential table (nullptr: none; per atom `stride` doubles after 4 A, the KL local
// triplets (n, c, alpha) first)
template <typename T>
__global__ __launch_bounds__(256) void k_energy_components(const T* __restrict__ pos, const T* __restrict__ grad,
                                                           const T* e_all, CompSys sys, const double* __restrict__ ecp_tab,
                                                           int KL, int stride, int N, int A, int B, T vnn, T* out) {
  __shared__ T s_pos[COMP_WPB * 3 * COMP_G];
  __shared__ T s_grad[COMP_WPB * 3 * COMP_G];
  __shared__ T s_out[AIQMC_NCOMPONENTS][COMP_WPB];
  const int tid = threadIdx.x;
  const int w0 = blockIdx.x * COMP_WPB;
  const int nwb = B - w0 < COMP_WPB ? B - w0 : COMP_WPB;   // walkers of this workgroup (>= 1)
  const int n3 = 3 * N, span = nwb * n3;
  const size_t base = (size_t)w0 * n3;
  for (int i = tid; i < span; i += 256) {
    s_pos[i] = pos[base + i];
    s_grad[i] = grad[base + i];
  }
  __syncthreads();
  const int g = tid / COMP_G, e = tid % COMP_G;
  const bool act = g < nwb && e < N;
  T vee = T(0), ven = T(0), vpl = T(0), tg = T(0);
  if (act) {
    const T* xw = s_pos + g * n3;
    const T x = xw[3 * e], y = xw[3 * e + 1], z = xw[3 * e + 2];
    for (int j = e + 1; j < N; ++j) {
      const T dx = xw[3 * j] - x, dy = xw[3 * j + 1] - y, dz = xw[3 * j + 2] - z;
      vee += T(1) / c_sqrt(dx * dx + dy * dy + dz * dz);
    }
    for (int a = 0; a < A; ++a) {
      const T dx = x - (T)sys.atoms[a][0], dy = y - (T)sys.atoms[a][1], dz = z - (T)sys.atoms[a][2];
      const T r2 = dx * dx + dy * dy + dz * dz, r = c_sqrt(r2);
      ven -= (T)sys.z[a] / r;
      if (ecp_tab) {
        const double* t = ecp_tab + 4 * A + (size_t)a * stride;
        for (int k = 0; k < KL; ++k)
          vpl += (T)t[3 * k + 1] * c_pow(r, (T)(t[3 * k] - 2.0)) * c_exp(-(T)t[3 * k + 2] * r2);
      }
    }
    const T* gw = s_grad + g * n3 + 3 * e;
    tg = gw[0] * gw[0] + gw[1] * gw[1] + gw[2] * gw[2];
  }
  // every lane of the wave takes part; the partner lane ^ m stays inside the group of 16
#pragma unroll
  for (int m = COMP_G / 2; m >= 1; m >>= 1) {
    vee += __shfl_xor(vee, m);
    ven += __shfl_xor(ven, m);
    vpl += __shfl_xor(vpl, m);
    tg += __shfl_xor(tg, m);
  }
  if (g < nwb && e == 0) {
    const T tot = out[w0 + g];
    const T eall = e_all ? e_all[w0 + g] : tot;
    const T kin = eall - ((vee + ven) + vnn);
    s_out[AIQMC_COMP_KINETIC][g] = kin;
    s_out[AIQMC_COMP_KINETIC_GRAD][g] = T(0.5) * tg;
    s_out[AIQMC_COMP_V_EE][g] = vee;
    s_out[AIQMC_COMP_V_EN][g] = ven;
    s_out[AIQMC_COMP_V_NN][g] = vnn;
    s_out[AIQMC_COMP_V_PP_LOCAL][g] = ecp_tab ? vpl : T(0);
    s_out[AIQMC_COMP_V_PP_NONLOCAL][g] = ecp_tab ? tot - ((((kin + vee) + ven) + vnn) + vpl) : T(0);
  }
  __syncthreads();
  // rows 1..7, 16 consecutive walkers each
  const int k = 1 + tid / COMP_WPB, i = tid % COMP_WPB;
  if (k < AIQMC_NCOMPONENTS && i < nwb) out[(size_t)k * B + w0 + i] = s_out[k][i];
}

}  // namespace

extern "C" {

int aiqmc_energy_components(aiqmc_ctx* c, const void* pos, int32_t B, int32_t complex_output, int32_t rng_mode,
                            const void* rot, uint64_t seed, uint64_t offset, void* out, void* stream) {
  AIQMC_CHECK(c, pos, B);
  if (!out && B > 0) return fail(AIQMC_EINVAL, "null out");
  if (c->ecp_set) {
    if (rng_mode != AIQMC_RNG_HOST && rng_mode != AIQMC_RNG_PHILOX) return fail(AIQMC_EINVAL, "rng_mode");
    if (rng_mode == AIQMC_RNG_HOST && B > 0 && !rot) return fail(AIQMC_EINVAL, "AIQMC_RNG_HOST needs rot");
  }
  if (c->N > COMP_G || c->A > COMP_MAX_ATOMS)
    return fail(AIQMC_EUNSUPPORTED, "aiqmc_energy_components: nelectrons <= 16 and natoms <= 5");
  if (B == 0) return AIQMC_OK;
  HIPCHK(hipSetDevice(c->device));
  // scratch [B] all-electron E_L, [B] imaginary part, [B][3N] grad log|psi|
  const size_t es = elem_size(c), n3 = (size_t)3 * c->N;
  HIPCHK(c->d_comp.reserve((size_t)B * (2 + n3) * es));
  char* e_all = c->d_comp.as<char>();
  char* e_im = e_all + (size_t)B * es;
  const void* grad = e_im + (size_t)B * es;
  const bool ecp = c->ecp_set, cplx = complex_output != 0;
  int rc;
  if (ecp) {
    rc = cplx ? aiqmc_local_energy_ecp_complex(c, pos, B, rng_mode, rot, seed, offset, out, e_im, stream)
              : aiqmc_local_energy_ecp(c, pos, B, rng_mode, rot, seed, offset, out, e_im, nullptr, nullptr, stream);
    if (rc) return rc;
  }
  void* e_ae = ecp ? (void*)e_all : out;   // the all-electron E_L: row 0 itself without an ECP
  rc = cplx ? aiqmc_local_energy_complex(c, pos, B, e_ae, e_im, stream)
            : aiqmc_local_energy(c, pos, B, e_ae, nullptr, (void*)grad, stream);
  if (rc) return rc;
  if (cplx) grad = c->d_cx.as();   // [B][3N] grad log|psi| of aiqmc_local_energy_complex (ctx.h)
  CompSys sys = {};
  double vnn = 0.0;
  for (int a = 0; a < c->A; ++a) {
    for (int d = 0; d < 3; ++d) sys.atoms[a][d] = c->atoms[3 * a + d];
    sys.z[a] = c->charges[a];
    for (int b = a + 1; b < c->A; ++b) {
      double r2 = 0.0;
      for (int d = 0; d < 3; ++d) {
        const double dd = c->atoms[3 * a + d] - c->atoms[3 * b + d];
        r2 += dd * dd;
      }
      vnn += c->charges[a] * c->charges[b] / std::sqrt(r2);
    }
  }
  const double* tab = ecp ? c->d_ecp_tab.as<double>() : nullptr;
  const int stride = 3 * (c->ecp_KL + c->ecp_L * c->ecp_KN);
  by_dtype(c->dtype, [&](auto t) {
    using T = decltype(t);
    k_energy_components<T><<<blocks(B, COMP_WPB), dim3(256), 0, (hipStream_t)stream>>>(
        (const T*)pos, (const T*)grad, ecp ? (const T*)e_all : nullptr, sys, tab, c->ecp_KL, stride, c->N, c->A, B,
        (T)vnn, (T*)out);
  });
  HIPCHK(hipGetLastError());
  return AIQMC_OK;
}

}  // extern "C"
