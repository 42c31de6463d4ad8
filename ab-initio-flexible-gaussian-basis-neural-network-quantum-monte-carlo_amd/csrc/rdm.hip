// rdm.hip -- the one-body reduced density matrix in a caller-supplied Gaussian basis
// (aiqmc_set_rdm_basis, aiqmc_rdm_accumulate, aiqmc_rdm_basis_values; include/aiqmc.h has the
// estimator and the table formats).
//
//   acc[1 + ((sigma K + i) K + j) 2 + part] (+)= sum_b w_b sum_s sum_{e in sigma}
//        phi_i(r_e) phi_j(r'_bs) [psi(x_b; r_e -> r'_bs) / psi(x_b)]_part / q(r'_bs),     acc[0] (+)= sum_b w_b
//
// Per chunk of W walkers (W (N S + 1) <= obs_chunk configurations, a whole number of groups of
// AIQMC_RDM_GROUP walkers or the whole batch), on the caller's stream:
//   k_rdm_points    r'_ws (copied, or drawn from q: Philox kinds 24 / 25, stream id b S + s) and
//                   1 / q(r'_ws), q in fp64
//   k_rdm_build     the W (N S + 1) configurations [w][p][3N]: p = 0 the walker, p = 1 + s N + e the
//                   walker with electron slot e at r'_ws (k_s2_exchange's layout)
//   value launch    ShapeOps::walker with aiqmc_logpsi's arguments, as aiqmc_spin_squared
//   k_rdm_ratio     F[w][s][e] = exp(dl) (cos dp, sin dp) / q(r'_ws) w_b, and ratio_out
//   k_rdm_basis     phi at the W N electron positions (each slot with its channel's MO coefficients)
//                   and, for both channels, at the W S points: Gaussians in fp64, rounded once to
//                   the operand dtype; the MO coefficients sit in LDS, the contraction over the
//                   functions is an fma chain in ascending order
//   k_rdm_contract  one workgroup per (group, sigma): rho = A^T Bm over the rows c = (w, s, e in sigma)
//                   ascending, A[c][i] = phi_i(r_e), Bm[c][j] = phi_j(r'_ws) F[w][s][e] (re and im
//                   apart), on v_mfma_{f32,f64}_16x16x4 with the row as the MFMA's k; K and row
//                   tails are zero-padded when the panel is staged.  The group's K x K tile leaves
//                   in the operand dtype.  Wave 0 of sigma = 0 also sums the group's weights.
//   k_rdm_fold      acc += the group tiles (and weight sums), fp64, groups ascending
// The order of every sum is a function of (B, S, K, n_up, n_down) alone, and folding group after
// group in fp64 does not see where a chunk ends: the same bits for any chunking.  No atomics.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <string>
#include <vector>

#include "aiqmc.h"
#include "host_shared.h"
#include "jets.h"

using namespace aq;

namespace {

constexpr uint32_t KIND_RDM_NORMAL = 24, KIND_RDM_COMPONENT = 25;
constexpr int RDM_PT = 32;                   // points per tile of k_rdm_basis
constexpr int RDM_PANEL = 16;                // contraction rows staged per barrier pair
constexpr int RDM_STRIDE = AIQMC_RDM_MAX_ORB + 16;   // the 4 rows one MFMA operand reads: disjoint banks
static_assert(AIQMC_RDM_MAX_ORB == 64, "k_rdm_contract: 4 waves x 16 tile rows, one staged column per lane");

// device views of the context's tables (ctx.h: d_rdm_tab, d_rdm_shell)
struct RdmTab {
  const double *cen, *ex, *co, *mo, *qc, *qh, *qn, *qs, *qcum;
  const int* shell;   // [nshell][4]: l, first primitive, primitives, first function
  int nshell, nao, norb, nq, mo_set;
};

RdmTab rdm_tab(const aiqmc_ctx* c) {
  RdmTab t;
  const double* p = c->d_rdm_tab.as<double>();
  t.cen = p, p += 3 * c->rdm_nshell;
  t.ex = p, p += c->rdm_nprim;
  t.co = p, p += c->rdm_nprim;
  t.mo = p, p += c->rdm_mo ? (size_t)2 * c->rdm_nao * c->rdm_norb : 0;
  t.qc = p, p += 3 * c->rdm_nq;
  t.qh = p, p += c->rdm_nq;
  t.qn = p, p += c->rdm_nq;
  t.qs = p, p += c->rdm_nq;
  t.qcum = p;
  t.shell = c->d_rdm_shell.as<int>();
  t.nshell = c->rdm_nshell, t.nao = c->rdm_nao, t.norb = c->rdm_norb, t.nq = c->rdm_nq, t.mo_set = c->rdm_mo;
  return t;
}

// rp[w][s][3], iq[w][s] = 1 / q(r') of walkers b0 .. b0 + nw; rprime_in / rprime_out are the call's [B][S][3]
template <typename T>
__global__ __launch_bounds__(256) void k_rdm_points(RdmTab tab, int philox, const T* __restrict__ rprime_in,
                                                    uint64_t seed, uint64_t step, int S, int b0, int nw,
                                                    T* __restrict__ rp, T* __restrict__ iq,
                                                    T* __restrict__ rprime_out) {
  const int t = blockIdx.x * 256 + threadIdx.x;
  if (t >= nw * S) return;
  const int64_t g = (int64_t)b0 * S + t;   // b S + s
  T r[3];
  if (philox) {
    float n[3], u[4];
    philox_normal3f(seed, step, (uint32_t)g, KIND_RDM_NORMAL, n);
    philox_u4(seed, step, (uint32_t)g, KIND_RDM_COMPONENT, u);
    int k = 0;
    while (k < tab.nq - 1 && !((double)u[0] < tab.qcum[k])) ++k;
#pragma unroll
    for (int d = 0; d < 3; ++d) r[d] = fma((T)tab.qs[k], (T)n[d], (T)tab.qc[3 * k + d]);
  } else {
#pragma unroll
    for (int d = 0; d < 3; ++d) r[d] = rprime_in[g * 3 + d];
  }
  double q = 0.0;
  for (int k = 0; k < tab.nq; ++k) {
    const double dx = (double)r[0] - tab.qc[3 * k], dy = (double)r[1] - tab.qc[3 * k + 1],
                 dz = (double)r[2] - tab.qc[3 * k + 2];
    q += tab.qn[k] * exp(-tab.qh[k] * (dx * dx + dy * dy + dz * dz));
  }
  iq[t] = (T)(1.0 / q);
#pragma unroll
  for (int d = 0; d < 3; ++d) {
    rp[(size_t)t * 3 + d] = r[d];
    if (rprime_out) rprime_out[g * 3 + d] = r[d];
  }
}

// x[q][3N] for q = w (N S + 1) + p < nconf
template <typename T>
__global__ __launch_bounds__(256) void k_rdm_build(const T* __restrict__ pos, const T* __restrict__ rp, int N, int S,
                                                   int b0, int nconf, T* __restrict__ x) {
  const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (t >= (int64_t)nconf * N) return;
  const int q = (int)(t / N), e = (int)(t - (int64_t)q * N);
  const int K1 = N * S + 1;
  const int w = q / K1, p = q - w * K1;
  const T* xs = pos + (size_t)(b0 + w) * 3 * N + 3 * e;
  if (p > 0 && (p - 1) % N == e) xs = rp + ((size_t)w * S + (p - 1) / N) * 3;
  T* xd = x + (size_t)q * 3 * N + 3 * e;
#pragma unroll
  for (int c = 0; c < 3; ++c) xd[c] = xs[c];
}

// f[w][s][e][2] = exp(dl) (cos dp, sin dp) / q(r'_ws) w_b; ratio_out[b0 + w][s][e][2] = (dl, dp)
template <typename T>
__global__ __launch_bounds__(256) void k_rdm_ratio(const T* __restrict__ lp, const T* __restrict__ ph,
                                                   const T* __restrict__ iq, const T* __restrict__ weights, int N,
                                                   int S, int b0, int nw, T* __restrict__ f,
                                                   T* __restrict__ ratio_out) {
  const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const int SN = S * N;
  if (t >= (int64_t)nw * SN) return;
  const int w = (int)(t / SN), r = (int)(t - (int64_t)w * SN);
  const size_t q0 = (size_t)w * (SN + 1);
  const T dl = lp[q0 + 1 + r] - lp[q0], dp = ph[q0 + 1 + r] - ph[q0];
  T re, im;
  unit_ratio(dl, dp, re, im);
  const T sc = iq[w * S + r / N], wg = weights ? weights[b0 + w] : T(1);
  f[2 * t] = re * sc * wg;
  f[2 * t + 1] = im * sc * wg;
  if (ratio_out) {
    const size_t o = ((size_t)(b0 + w) * SN + r) * 2;
    ratio_out[o] = dl;
    ratio_out[o + 1] = dp;
  }
}

// out[(pi / per) out_per + idx][K] = phi^spin(point), point = src + (pi / per) stride_w + 3 idx,
// idx = sel ? sel[pi % per] : pi % per.  Dynamic LDS: the MO coefficients [nao][norb] (when set)
// and the tile's function values [RDM_PT][nao], both T.
template <typename T>
__global__ __launch_bounds__(256) void k_rdm_basis(RdmTab tab, const T* __restrict__ src, int npts, int per,
                                                   int64_t stride_w, const int* __restrict__ sel, int spin,
                                                   T* __restrict__ out, int out_per) {
  extern __shared__ __attribute__((aligned(16))) unsigned char rdm_smem[];
  const int nao = tab.nao, K = tab.norb, t = (int)threadIdx.x;
  T* cm = (T*)rdm_smem;
  T* ao = cm + (tab.mo_set ? nao * K : 0);
  if (tab.mo_set) {
    const double* __restrict__ mo = tab.mo + (size_t)spin * nao * K;
    for (int i = t; i < nao * K; i += 256) cm[i] = (T)mo[i];
  }
  for (int tile0 = blockIdx.x * RDM_PT; tile0 < npts; tile0 += gridDim.x * RDM_PT) {
    __syncthreads();   // cm is there; the previous tile's ao has been read
    for (int idx = t; idx < RDM_PT * tab.nshell; idx += 256) {
      const int p = idx / tab.nshell, sh = idx - p * tab.nshell, pi = tile0 + p;
      if (pi >= npts) continue;
      const int w = pi / per, i = pi - w * per;
      const T* __restrict__ xs = src + (size_t)w * stride_w + 3 * (sel ? sel[i] : i);
      const int l = tab.shell[4 * sh], p0 = tab.shell[4 * sh + 1], np = tab.shell[4 * sh + 2],
                a0 = tab.shell[4 * sh + 3];
      const double dx = (double)xs[0] - tab.cen[3 * sh], dy = (double)xs[1] - tab.cen[3 * sh + 1],
                   dz = (double)xs[2] - tab.cen[3 * sh + 2];
      const double r2 = dx * dx + dy * dy + dz * dz;
      double R = 0.0;
      for (int k = p0; k < p0 + np; ++k) R += tab.co[k] * exp(-tab.ex[k] * r2);
      T* o = ao + p * nao + a0;
      if (l == 0) {
        o[0] = (T)R;
      } else if (l == 1) {
        o[0] = (T)(dx * R), o[1] = (T)(dy * R), o[2] = (T)(dz * R);
      } else {
        o[0] = (T)(dx * dx * R), o[1] = (T)(dx * dy * R), o[2] = (T)(dx * dz * R);
        o[3] = (T)(dy * dy * R), o[4] = (T)(dy * dz * R), o[5] = (T)(dz * dz * R);
      }
    }
    __syncthreads();
    for (int idx = t; idx < RDM_PT * K; idx += 256) {
      const int p = idx / K, j = idx - p * K, pi = tile0 + p;
      if (pi >= npts) continue;
      const int w = pi / per, i = pi - w * per;
      T v;
      if (tab.mo_set) {
        v = T(0);
        for (int a = 0; a < nao; ++a) v = fma(ao[p * nao + a], cm[a * K + j], v);
      } else {
        v = ao[p * nao + j];
      }
      out[((size_t)w * out_per + (sel ? sel[i] : i)) * K + j] = v;
    }
  }
}

template <typename T> struct RdmMfma;
template <> struct RdmMfma<float> {
  typedef float v4 __attribute__((ext_vector_type(4)));
  static __device__ __forceinline__ v4 mma(float a, float b, v4 c) {
    return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0);
  }
  // accumulator register v of lane group q holds row 4q + v (column = lane & 15)
  static constexpr __device__ int row(int q, int v) { return 4 * q + v; }
};
template <> struct RdmMfma<double> {
  typedef double v4 __attribute__((ext_vector_type(4)));
  static __device__ __forceinline__ v4 mma(double a, double b, v4 c) {
    return __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, c, 0, 0, 0);
  }
  static constexpr __device__ int row(int q, int v) { return q + 4 * v; }   // f64 C/D map
};

// grid (groups of the chunk, 2): tile[g][sigma][K][K][2] and, from sigma = 0, wsum[g].
// pe [nw][N][K], pp [2][nw][S][K], f [nw][S][N][2] of the chunk; weights of the call, b0 the chunk's first walker
template <typename T>
__global__ __launch_bounds__(256) void k_rdm_contract(const T* __restrict__ pe, const T* __restrict__ pp,
                                                      const T* __restrict__ f, const int* __restrict__ rowsrc,
                                                      const T* __restrict__ weights, int N, int S, int nup, int ndn,
                                                      int K, int b0, int nw, T* __restrict__ tile,
                                                      double* __restrict__ wsum) {
  using M = RdmMfma<T>;
  using V4 = typename M::v4;
  __shared__ T pa[RDM_PANEL * RDM_STRIDE], pre[RDM_PANEL * RDM_STRIDE], pim[RDM_PANEL * RDM_STRIDE];
  const int g = blockIdx.x, sg = blockIdx.y;
  const int t = (int)threadIdx.x, lane = t & 63, wave = t >> 6;
  const int q = lane >> 4, e16 = lane & 15;
  const int w0 = g * AIQMC_RDM_GROUP;
  const int ng = nw - w0 < AIQMC_RDM_GROUP ? nw - w0 : AIQMC_RDM_GROUP;
  const int ns = sg ? ndn : nup;
  const int* __restrict__ slots = rowsrc + (sg ? nup : 0);
  const int R = ng * S * ns, nt = (K + 15) / 16;
  const T* __restrict__ pps = pp + (size_t)sg * nw * S * K;

  if (sg == 0 && wave == 0) {   // the group's weights: one per lane, an xor butterfly in fp64
    double v = 0.0;
    if (lane < ng) v = weights ? (double)weights[b0 + w0 + lane] : 1.0;
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m);
    if (lane == 0) wsum[g] = v;
  }

  V4 are[4], aim[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) are[j] = aim[j] = V4{T(0), T(0), T(0), T(0)};
  // staging role: column lane of the panel, rows wave, wave + 4, ..
  for (int r0 = 0; r0 < R; r0 += RDM_PANEL) {
    __syncthreads();   // the previous panel has been read
#pragma unroll
    for (int r = 0; r < RDM_PANEL / 4; ++r) {
      const int lr = wave + 4 * r, c = r0 + lr;
      T a = T(0), bre = T(0), bim = T(0);
      if (c < R && lane < K) {
        const int wl = c / (S * ns), rem = c - wl * (S * ns);
        const int s = rem / ns, e = slots[rem - s * ns], w = w0 + wl;
        const size_t fi = (((size_t)w * S + s) * N + e) * 2;
        const T p = pps[((size_t)w * S + s) * K + lane];
        a = pe[((size_t)w * N + e) * K + lane];
        bre = p * f[fi];
        bim = p * f[fi + 1];
      }
      pa[lr * RDM_STRIDE + lane] = a;
      pre[lr * RDM_STRIDE + lane] = bre;
      pim[lr * RDM_STRIDE + lane] = bim;
    }
    __syncthreads();
    if (wave < nt) {
#pragma unroll
      for (int ks = 0; ks < RDM_PANEL / 4; ++ks) {
        const int ro = (ks * 4 + q) * RDM_STRIDE + e16;
        const T a = pa[ro + wave * 16];
#pragma unroll
        for (int j = 0; j < 4; ++j)
          if (j < nt) {
            are[j] = M::mma(a, pre[ro + j * 16], are[j]);
            aim[j] = M::mma(a, pim[ro + j * 16], aim[j]);
          }
      }
    }
  }
  if (wave < nt) {
    T* __restrict__ o = tile + ((size_t)g * 2 + sg) * K * K * 2;
#pragma unroll
    for (int j = 0; j < 4; ++j)
#pragma unroll
      for (int v = 0; v < 4; ++v) {
        const int i = wave * 16 + M::row(q, v), jj = j * 16 + e16;
        if (j < nt && i < K && jj < K) {
          o[((size_t)i * K + jj) * 2] = are[j][v];
          o[((size_t)i * K + jj) * 2 + 1] = aim[j][v];
        }
      }
  }
}

// acc[0] (+)= wsum[g], acc[1 + t] (+)= tile[g][t], groups ascending; first: acc starts from zero
template <typename T>
__global__ __launch_bounds__(256) void k_rdm_fold(const T* __restrict__ tile, const double* __restrict__ wsum,
                                                  int ngroups, int n, int first, double* __restrict__ acc) {
  const int t = blockIdx.x * 256 + threadIdx.x;
  if (t > n) return;
  double s = first ? 0.0 : acc[t];
  if (t == 0) {
    for (int g = 0; g < ngroups; ++g) s += wsum[g];
  } else {
    for (int g = 0; g < ngroups; ++g) s += (double)tile[(size_t)g * n + (t - 1)];
  }
  acc[t] = s;
}

size_t basis_lds(const aiqmc_ctx* c) {
  return ((c->rdm_mo ? (size_t)c->rdm_nao * c->rdm_norb : 0) + (size_t)RDM_PT * c->rdm_nao) * elem_size(c);
}

template <typename T>
void basis_launch(const aiqmc_ctx* c, const RdmTab& tab, const void* src, int npts, int per, int64_t stride_w,
                  const int* sel, int spin, void* out, int out_per, hipStream_t s) {
  if (npts <= 0) return;
  int nb = (npts + RDM_PT - 1) / RDM_PT;
  if (nb > 1024) nb = 1024;
  k_rdm_basis<T><<<dim3(nb), dim3(256), basis_lds(c), s>>>(tab, (const T*)src, npts, per, stride_w, sel, spin, (T*)out,
                                                            out_per);
}

}  // namespace

extern "C" {

int aiqmc_set_rdm_basis(aiqmc_ctx* c, const aiqmc_rdm_basis* b) {
  if (!c) return fail(AIQMC_EINVAL, "null context");
  c->rdm_set = false;
  if (!b) return AIQMC_OK;
  if (b->nshell < 1 || !b->shell_l || !b->shell_nprim || !b->shell_center || !b->exps || !b->coefs)
    return fail(AIQMC_EINVAL, "rdm basis: nshell < 1 or a null shell table");
  if (b->nshell > AIQMC_RDM_MAX_AO) return fail(AIQMC_EINVAL, "rdm basis: nao above " + std::to_string(AIQMC_RDM_MAX_AO));
  int nao = 0, nprim = 0;
  std::vector<int> shell(4 * (size_t)b->nshell);
  for (int i = 0; i < b->nshell; ++i) {
    const int l = b->shell_l[i], np = b->shell_nprim[i];
    if (l < 0 || l > 2) return fail(AIQMC_EINVAL, "rdm basis: shell_l must be 0, 1 or 2");
    if (np < 1) return fail(AIQMC_EINVAL, "rdm basis: a shell without primitives");
    shell[4 * i] = l, shell[4 * i + 1] = nprim, shell[4 * i + 2] = np, shell[4 * i + 3] = nao;
    nao += (l + 1) * (l + 2) / 2;
    if (np > AIQMC_RDM_MAX_PRIM - nprim)
      return fail(AIQMC_EINVAL, "rdm basis: more than " + std::to_string(AIQMC_RDM_MAX_PRIM) + " primitives");
    nprim += np;
  }
  if (nao > AIQMC_RDM_MAX_AO) return fail(AIQMC_EINVAL, "rdm basis: nao above " + std::to_string(AIQMC_RDM_MAX_AO));
  const bool mo = b->mo_coeff != nullptr;
  const int norb = mo ? b->norb : nao;
  if (norb < 1 || norb > AIQMC_RDM_MAX_ORB)
    return fail(AIQMC_EINVAL, "rdm basis: norb must be in [1, " + std::to_string(AIQMC_RDM_MAX_ORB) + "]");
  for (int k = 0; k < nprim; ++k)
    if (!std::isfinite(b->exps[k]) || !std::isfinite(b->coefs[k]))
      return fail(AIQMC_EINVAL, "rdm basis: exps / coefs must be finite");
  const int nq = b->nq;
  if (nq < 1 || nq > AIQMC_RDM_MAX_Q) return fail(AIQMC_EINVAL, "rdm basis: nq must be in [1, " + std::to_string(AIQMC_RDM_MAX_Q) + "]");
  if (!b->q_center || !b->q_sigma || !b->q_prob) return fail(AIQMC_EINVAL, "rdm basis: null q table");
  double psum = 0.0;
  for (int k = 0; k < nq; ++k) {
    if (!(b->q_sigma[k] > 0.0) || !std::isfinite(b->q_sigma[k])) return fail(AIQMC_EINVAL, "rdm basis: q_sigma must be positive");
    if (!(b->q_prob[k] > 0.0)) return fail(AIQMC_EINVAL, "rdm basis: q_prob must be positive");
    psum += b->q_prob[k];
  }
  if (!(std::fabs(psum - 1.0) <= 1e-12)) return fail(AIQMC_EINVAL, "rdm basis: q_prob must sum to 1");

  std::vector<double> tab;
  tab.insert(tab.end(), b->shell_center, b->shell_center + 3 * (size_t)b->nshell);
  tab.insert(tab.end(), b->exps, b->exps + nprim);
  tab.insert(tab.end(), b->coefs, b->coefs + nprim);
  if (mo) tab.insert(tab.end(), b->mo_coeff, b->mo_coeff + (size_t)2 * nao * norb);
  tab.insert(tab.end(), b->q_center, b->q_center + 3 * (size_t)nq);
  const double two_pi = 6.283185307179586476925287;
  for (int k = 0; k < nq; ++k) tab.push_back(0.5 / (b->q_sigma[k] * b->q_sigma[k]));
  for (int k = 0; k < nq; ++k) {
    const double v = two_pi * b->q_sigma[k] * b->q_sigma[k];
    tab.push_back(b->q_prob[k] / (v * std::sqrt(v)));
  }
  tab.insert(tab.end(), b->q_sigma, b->q_sigma + nq);
  double cum = 0.0;
  for (int k = 0; k < nq; ++k) tab.push_back(cum += b->q_prob[k]);

  HIPCHK(hipSetDevice(c->device));
  HIPCHK(c->d_rdm_tab.reserve(tab.size() * sizeof(double)));
  HIPCHK(c->d_rdm_shell.reserve(shell.size() * sizeof(int)));
  HIPCHK(hipMemcpy(c->d_rdm_tab.as(), tab.data(), tab.size() * sizeof(double), hipMemcpyHostToDevice));
  HIPCHK(hipMemcpy(c->d_rdm_shell.as(), shell.data(), shell.size() * sizeof(int), hipMemcpyHostToDevice));
  c->rdm_nshell = b->nshell, c->rdm_nprim = nprim, c->rdm_nao = nao, c->rdm_norb = norb, c->rdm_nq = nq;
  c->rdm_mo = mo;
  // k_rdm_basis above the default 64 KB of dynamic LDS
  const int lds = (int)basis_lds(c);
  if (lds > 65536) {
    const void* fn = c->dtype == AIQMC_F32 ? (const void*)&k_rdm_basis<float> : (const void*)&k_rdm_basis<double>;
    HIPCHK(hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, lds));
  }
  c->rdm_set = true;
  return AIQMC_OK;
}

int aiqmc_rdm_basis_values(aiqmc_ctx* c, const void* points, int32_t M, int32_t spin, void* out, void* stream) {
  if (!c) return fail(AIQMC_EINVAL, "null context");
  if (!c->rdm_set) return fail(AIQMC_ESTATE, "aiqmc_set_rdm_basis has not been called");
  if (M < 0) return fail(AIQMC_EINVAL, "negative point count");
  if (spin != 0 && spin != 1) return fail(AIQMC_EINVAL, "spin must be 0 or 1");
  if (M == 0) return AIQMC_OK;
  if (!points || !out) return fail(AIQMC_EINVAL, "null points / out");
  HIPCHK(hipSetDevice(c->device));
  const RdmTab tab = rdm_tab(c);
  by_dtype(c->dtype, [&](auto t) {
    basis_launch<decltype(t)>(c, tab, points, M, M, 0, nullptr, spin, out, M, (hipStream_t)stream);
  });
  HIPCHK(hipGetLastError());
  return AIQMC_OK;
}

int aiqmc_rdm_accumulate(aiqmc_ctx* c, const void* pos, int32_t B, int32_t S, int32_t rng_mode,
                         const void* rprime_in, uint64_t seed, uint64_t step, const void* weights, double* acc,
                         int32_t accumulate, void* rprime_out, void* ratio_out, void* stream) {
  AIQMC_CHECK(c, pos, B);
  if (!c->rdm_set) return fail(AIQMC_ESTATE, "aiqmc_set_rdm_basis has not been called");
  if (S < 1) return fail(AIQMC_EINVAL, "rdm: S must be at least 1");
  if (rng_mode != AIQMC_RNG_HOST && rng_mode != AIQMC_RNG_PHILOX) return fail(AIQMC_EINVAL, "unknown rng_mode");
  if (B > 0 && rng_mode == AIQMC_RNG_HOST && !rprime_in) return fail(AIQMC_EINVAL, "AIQMC_RNG_HOST needs rprime_in");
  if (B > 0 && !acc) return fail(AIQMC_EINVAL, "null acc");
  AIQMC_BEGIN(c, B, ops);
  const int N = c->N, K = c->rdm_norb;
  if ((int64_t)N * S + 1 > INT32_MAX / AIQMC_RDM_GROUP || (int64_t)B * S * N > INT32_MAX)
    return fail(AIQMC_EINVAL, "too many moved configurations for one call");
  const int K1 = N * S + 1;
  int W = c->obs_chunk / K1;   // walkers per chunk: whole groups, or the whole batch
  if (W >= B) {
    W = B;
  } else {
    W = W / AIQMC_RDM_GROUP * AIQMC_RDM_GROUP;
    if (W < AIQMC_RDM_GROUP) W = AIQMC_RDM_GROUP;
    if (W > B) W = B;
  }
  if ((int64_t)W * K1 > INT32_MAX) return fail(AIQMC_EINVAL, "too many moved configurations for one chunk");
  const size_t es = elem_size(c);
  const int G = (W + AIQMC_RDM_GROUP - 1) / AIQMC_RDM_GROUP, nt = 2 * K * K * 2;
  if (int rc = aq_host::ensure_obs(c, W * K1, ops)) return rc;
  HIPCHK(c->d_rdm_rp.reserve((size_t)W * S * 3 * es));
  HIPCHK(c->d_rdm_iq.reserve((size_t)W * S * es));
  HIPCHK(c->d_rdm_pe.reserve((size_t)W * N * K * es));
  HIPCHK(c->d_rdm_pp.reserve((size_t)2 * W * S * K * es));
  HIPCHK(c->d_rdm_f.reserve((size_t)W * S * N * 2 * es));
  HIPCHK(c->d_rdm_tile.reserve((size_t)G * nt * es));
  HIPCHK(c->d_rdm_wsum.reserve((size_t)G * sizeof(double)));
  const RdmTab tab = rdm_tab(c);
  hipStream_t s = (hipStream_t)stream;
  void *lp = c->d_obs_lp.as(), *ph = c->d_obs_ph.as();
  const int* rowsrc = c->d_rowsrc.as<int>();
  for (int b0 = 0; b0 < B; b0 += W) {
    const int nw = B - b0 < W ? B - b0 : W;
    const int nconf = nw * K1, ng = (nw + AIQMC_RDM_GROUP - 1) / AIQMC_RDM_GROUP;
    by_dtype(c->dtype, [&](auto t) {
      using T = decltype(t);
      T *rp = c->d_rdm_rp.as<T>(), *pe = c->d_rdm_pe.as<T>(), *pp = c->d_rdm_pp.as<T>(), *f = c->d_rdm_f.as<T>();
      k_rdm_points<T><<<blocks((int64_t)nw * S, 256), dim3(256), 0, s>>>(
          tab, rng_mode == AIQMC_RNG_PHILOX, (const T*)rprime_in, seed, step, S, b0, nw, rp, c->d_rdm_iq.as<T>(),
          (T*)rprime_out);
      k_rdm_build<T><<<blocks((int64_t)nconf * N, 256), dim3(256), 0, s>>>((const T*)pos, rp, N, S, b0, nconf,
                                                                           c->d_obs_x.as<T>());
      aq_host::obs_values(c, ops, nconf, s);
      k_rdm_ratio<T><<<blocks((int64_t)nw * S * N, 256), dim3(256), 0, s>>>(
          (const T*)lp, (const T*)ph, c->d_rdm_iq.as<T>(), (const T*)weights, N, S, b0, nw, f, (T*)ratio_out);
      const T* xw = (const T*)pos + (size_t)b0 * 3 * N;
      basis_launch<T>(c, tab, xw, nw * c->nup, c->nup, 3 * N, rowsrc, 0, pe, N, s);
      basis_launch<T>(c, tab, xw, nw * c->ndn, c->ndn, 3 * N, rowsrc + c->nup, 1, pe, N, s);
      for (int sg = 0; sg < 2; ++sg)
        basis_launch<T>(c, tab, rp, nw * S, S, 3 * S, nullptr, sg, pp + (size_t)sg * nw * S * K, S, s);
      k_rdm_contract<T><<<dim3(ng, 2), dim3(256), 0, s>>>(pe, pp, f, rowsrc, (const T*)weights, N, S, c->nup, c->ndn,
                                                         K, b0, nw, c->d_rdm_tile.as<T>(),
                                                         c->d_rdm_wsum.as<double>());
      k_rdm_fold<T><<<blocks(nt + 1, 256), dim3(256), 0, s>>>(c->d_rdm_tile.as<T>(), c->d_rdm_wsum.as<double>(), ng,
                                                             nt, b0 == 0 && !accumulate, acc);
    });
  }
  HIPCHK(hipGetLastError());
  return AIQMC_OK;
}

}  // extern "C"
