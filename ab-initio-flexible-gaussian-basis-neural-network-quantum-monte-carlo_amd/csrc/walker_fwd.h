// walker_fwd.h -- one wavefront evaluates log|psi|, its gradient and
// (MODE == MODE_LAP) its Laplacian for ONE electron configuration of the AIQMC
// wavefunction (AIQMCrelease3/wavefunction_Ynlm/nn.py:106-553), then the local
// energy (Energy/hamiltonian.py:236-260, complex_output=False).
//
// Derivatives are forward-mode: direction lane (c,e) propagates the first and
// diagonal-second derivative along x_{e,c} (see jets.h).  Sparsity is used
// structurally: per-electron quantities (ae features, Ylm stream, envelope,
// e-n Jastrow) depend on x_e only and are computed as PJ jets by the lanes of
// electron e; pair quantities h2[k,i] (never mixed across pairs, nn.py:305-309)
// depend on x_k, x_i only.  Only the mean-field h stream is carried as dense
// wave-shared DJ jets, stored lane-private in LDS between layers.
//
// Determinant derivatives use the low-rank structure of the orbital matrix
//   A[r,c] = Phi[r,c] * Yt[r,c],   Phi[r,:] = H[r,:] W_{s(r)} + b_{s(r)}  (complex)
//   Yt[r,c] = env_r * Y[r,c]  (real, depends on x_r only),
// with B = A^{-1}, Q_f = P_f B, P_f[r,c] = W_{s(r)}[f,c] Yt[r,c]:
//   d_k log|det A| = sum_{r,f} U[r,f] Re Q_f[r,r] + Re(w.b_e)
//   d2_k log|det A| = Re[ sum U2 Q_f[r,r] + (2 dPhi_e.Yt' + Phi_e.Yt'') b_e
//                       - sum_{r,s} S_rs S_sr - 2 sum_{r,f} U z Q_f[r,e] - (w.b_e)^2 ]
// where U = d_k H, U2 = d2_k H, S = sum_f diag(U_f) Q_f, w = Phi[e,:] * d_k Yt[e,:],
// z = B^T w, b_e = B[:,e], e = electron of direction k.  The Jastrow factors
// scale every element (Q11) and enter log|psi| additively.
//
// The diagnostic kernel of the library (aiqmc_debug_local_energy_forward, _logpsi_grad_forward):
// shape.hip alone includes this file.
#pragma once
#include "jets.h"
#include "layout.h"
#include "gj.h"
#include "electron.h"
#include "kargs.h"

namespace aq {

constexpr int MODE_GRAD = 1;
constexpr int MODE_LAP = 2;
constexpr int MODE_GRAD_FWD = 3;   // forward-mode gradient (diagnostics / cross-check)

template <typename T, int N, bool LAP>
struct Smem {
  static constexpr int NC = LAP ? 2 : 1;
  static constexpr int xs = 0;
  static constexpr int hb = 48;
  static constexpr int yv = hb + N * 4 * NC * 64;
  static constexpr int ph = yv + N * N;
  static constexpr int mx = ph + N * N * 2;
  static constexpr int fac = mx + N * N * 2;
  static constexpr int qs = fac + N * 2;
  static constexpr int end = qs + (LAP ? N * N * 8 : N * 8);
  static constexpr int bytes = ((end * (int)sizeof(T)) + 15) & ~15;
};

template <typename T, int N, int A, bool LAP, int L>
__device__ __forceinline__ void h_layer(cptr<T> P, const T* xs, T* hb, const PJ<T>* hf,
                                        int lane, int lc, int er, int le, bool val, bool dir, bool live,
                                        int nup, T& jd1, T& jd2, T& jv, T& vv) {
  using Ly = Lay<N, A>;
  constexpr int NC = LAP ? 2 : 1;
  constexpr int DIN = (L == 0) ? 4 * A : NH;
  constexpr int DF = 3 * DIN + 2 * NH2;
  constexpr int Q = DF / 4;
  const cptr<T> convw = P + (L == 0 ? Ly::conv_w0 : (L == 1 ? Ly::conv_w1 : Ly::conv_w2));
  const cptr<T> convb = P + (L == 0 ? Ly::conv_b0 : (L == 1 ? Ly::conv_b1 : Ly::conv_b2));
  const cptr<T> sngw = P + (L == 0 ? Ly::sng_w0 : (L == 1 ? Ly::sng_w1 : Ly::sng_w2));
  const cptr<T> sngb = P + (L == 0 ? Ly::sng_b0 : (L == 1 ? Ly::sng_b1 : Ly::sng_b2));
  const int glo[2] = {0, nup};
  const int ghi[2] = {nup, N};
  const T ginv[2] = {T(1) / T(nup), T(1) / T(N - nup)};
  const T RSQ2 = T(0.70710678118654752);  // residual (x+y)/sqrt(2), nn.py:284

  // ---- g1: spin-group means of h (construct_symmetric_features, nn.py:142-150)
  DJ<T> g1[2][DIN];
#pragma unroll
  for (int G = 0; G < 2; ++G) {
    const bool inG = live && er >= glo[G] && er < ghi[G];
    if constexpr (L == 0) {
#pragma unroll
      for (int m = 0; m < DIN; ++m) {
        const T S = rowsum16((val && inG) ? hf[m].v : T(0));
        g1[G][m].d1 = val ? S * ginv[G] : ((dir && inG) ? hf[m].d1 * ginv[G] : T(0));
        g1[G][m].d2 = (dir && inG) ? hf[m].d2 * ginv[G] : T(0);
      }
    } else {
#pragma unroll
      for (int m = 0; m < DIN; ++m) g1[G][m] = dj_zero<T>();
      for (int k = glo[G]; k < ghi[G]; ++k) {
#pragma unroll
        for (int m = 0; m < DIN; ++m) {
          g1[G][m].d1 += hb[((k * 4 + m) * NC + 0) * 64 + lane];
          if constexpr (LAP) g1[G][m].d2 += hb[((k * 4 + m) * NC + 1) * 64 + lane];
        }
      }
#pragma unroll
      for (int m = 0; m < DIN; ++m) {
        g1[G][m].d1 *= ginv[G];
        g1[G][m].d2 *= ginv[G];
      }
    }
  }

  // ---- column loop: electron i's new h (nn.py:280-311)
#pragma unroll 1
  for (int i = 0; i < N; ++i) {
    // pair (le, i): ee[le,i] = x_i - x_le, r_ee (nn.py:111-115); lane direction is x_{le,lc}
    // dead lanes (er >= N) compute the clamped pair (N-1, i) and treat it as diagonal when i == N-1,
    // so no lane ever evaluates sqrt'(0)
    const bool diag = (le == i);
    PJ<T> d[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) d[c] = PJ<T>{xs[i * 3 + c] - xs[le * 3 + c], (lc == c) ? T(-1) : T(0), T(0)};
    PJ<T> r2 = d[0] * d[0] + d[1] * d[1] + d[2] * d[2];
    r2 = pj_sel(diag, pjc(T(1)), r2);
    const PJ<T> r = pj_sqrt(r2);
    PJ<T> p[4];
    p[0] = pj_sel(diag, pjc(T(0)), r);
#pragma unroll
    for (int c = 0; c < 3; ++c) p[1 + c] = pj_sel(diag, pjc(T(0)), d[c]);

    if constexpr (L == 0) {
      // Pade e-e Jastrow pair term r*cusp/(1+alpha r) (Jastrow.py:51-52) and V_ee (hamiltonian.py:177-187)
      const T cusp = P[Ly::jee_c + le * N + i];
      const T al = P[Ly::jee_a + le * N + i];
      const PJ<T> fj = (cusp * r) / (al * r + T(1));
      const bool pd = dir && !diag;
      jd1 += pd ? fj.d1 : T(0);
      jd2 += pd ? fj.d2 : T(0);
      const bool pv = val && live && er < i;
      jv += pv ? fj.v : T(0);
      vv += pv ? f_rcp(r.v) : T(0);
    }
    // pair stream: L double layers, tanh + residual (nn.py:305-309)
#pragma unroll
    for (int j = 0; j < L; ++j) {
      const cptr<T> dw = P + (j == 0 ? Ly::dbl_w0 : Ly::dbl_w1);
      const cptr<T> db = P + (j == 0 ? Ly::dbl_b0 : Ly::dbl_b1);
      PJ<T> q[4];
#pragma unroll
      for (int o = 0; o < 4; ++o) {
        PJ<T> s = dw[0 * 4 + o] * p[0];
#pragma unroll
        for (int m = 1; m < 4; ++m) s = s + dw[m * 4 + o] * p[m];
        q[o] = pj_tanh(s + db[o]);
      }
#pragma unroll
      for (int o = 0; o < 4; ++o) p[o] = (p[o] + q[o]) * RSQ2;
    }
    // g2: column means of h2 over spin groups (nn.py:151); 8 (16) independent row sums interleaved
    DJ<T> g2[2][4];
    {
      T X[8], X2[8];
      bool inGs[2], mps[2];
#pragma unroll
      for (int G = 0; G < 2; ++G) {
        inGs[G] = live && er >= glo[G] && er < ghi[G];
        mps[G] = inGs[G] && !diag;
#pragma unroll
        for (int f = 0; f < 4; ++f) {
          X[G * 4 + f] = val ? (inGs[G] ? p[f].v : T(0)) : (mps[G] ? p[f].d1 : T(0));
          X2[G * 4 + f] = (!val && mps[G]) ? p[f].d2 : T(0);
        }
      }
      rowsum16_multi<T, 8>(X);
      if constexpr (LAP) rowsum16_multi<T, 8>(X2);
      // d1 = cS * S + cP * p.d1  (value row: S/|G|; electron i's lanes: -S/|G|; other members: p.d1/|G|)
#pragma unroll
      for (int G = 0; G < 2; ++G) {
        const T cS = val ? ginv[G] : ((diag && dir) ? -ginv[G] : T(0));
        const T cS2 = (diag && dir) ? ginv[G] : T(0);
        const T cP = (mps[G] && dir) ? ginv[G] : T(0);
#pragma unroll
        for (int f = 0; f < 4; ++f) {
          g2[G][f].d1 = cS * X[G * 4 + f] + cP * p[f].d1;
          g2[G][f].d2 = LAP ? (cS2 * X2[G * 4 + f] + cP * p[f].d2) : T(0);
        }
      }
    }
    // h_i as wave-shared jets
    DJ<T> hi[DIN];
    if constexpr (L == 0) {
      const T cD = (diag && dir) ? T(1) : T(0);
      const T cV = val ? T(1) : T(0);
#pragma unroll
      for (int m = 0; m < DIN; ++m) {
        const T hv = rdlane(hf[m].v, 48 + i);
        hi[m].d1 = cD * hf[m].d1 + cV * hv;
        hi[m].d2 = cD * hf[m].d2;
      }
    } else {
#pragma unroll
      for (int m = 0; m < DIN; ++m) {
        hi[m].d1 = hb[((i * 4 + m) * NC + 0) * 64 + lane];
        hi[m].d2 = LAP ? hb[((i * 4 + m) * NC + (LAP ? 1 : 0)) * 64 + lane] : T(0);
      }
    }
    // convolutional layer: tanh(mean_4(f * w) + b)  (network_blocks.py:106-116)
    DJ<T> cq[Q];
#pragma unroll
    for (int q = 0; q < Q; ++q) {
      DJ<T> z = dj_zero<T>();
#pragma unroll
      for (int s = 0; s < 4; ++s) {
        const int idx = 4 * q + s;
        DJ<T> F;
        if (idx < DIN) F = hi[idx];
        else if (idx < 2 * DIN) F = g1[0][idx - DIN];
        else if (idx < 3 * DIN) F = g1[1][idx - 2 * DIN];
        else if (idx < 3 * DIN + 4) F = g2[0][idx - 3 * DIN];
        else F = g2[1][idx - 3 * DIN - 4];
        dj_axpy(z, convw[i * DF + idx] * T(0.25), F);
      }
      const T bq = convb[i * Q + q];
      z.d1 += val ? bq : T(0);
      cq[q] = dj_tanh(z, val);
    }
    // single linear + tanh + residual (nn.py:296-300)
#pragma unroll
    for (int f = 0; f < 4; ++f) {
      DJ<T> s = dj_zero<T>();
#pragma unroll
      for (int q = 0; q < Q; ++q) dj_axpy(s, sngw[q * 4 + f], cq[q]);
      const T bf = sngb[f];
      s.d1 += val ? bf : T(0);
      s = dj_tanh(s, val);
      DJ<T> nh;
      if constexpr (DIN == NH) {
        nh.d1 = (hi[f].d1 + s.d1) * RSQ2;
        nh.d2 = (hi[f].d2 + s.d2) * RSQ2;
      } else {
        nh = s;
      }
      hb[((i * 4 + f) * NC + 0) * 64 + lane] = nh.d1;
      if constexpr (LAP) hb[((i * 4 + f) * NC + 1) * 64 + lane] = nh.d2;
    }
  }
}

template <typename T, int N, int A, int MODE>
// Diagnostics-only kernels (forward-mode gradient and Laplacian).  The fp64 Laplacian
// instantiations use 256 VGPRs + 256 AGPRs and spill to scratch (N = 10: 1,980 B/lane, all
// constant-offset spill slots; DESIGN.md "GPU fault audit").
__global__ __launch_bounds__(64) void k_walker(KArgs ka) {
  constexpr bool LAP = (MODE == MODE_LAP);
  using Ly = Lay<N, A>;
  using SM = Smem<T, N, LAP>;
  constexpr int NC = SM::NC;
  const cptr<T> P = param_ptr<T>(ka.prm);
  extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
  T* sm = (T*)smem_raw;
  T* xs = sm + SM::xs;
  T* hb = sm + SM::hb;
  T* Yv = sm + SM::yv;
  T* Ph = sm + SM::ph;
  T* Mx = sm + SM::mx;
  T* Qs = sm + SM::qs;

  const int conf = blockIdx.x;
  const int lane = threadIdx.x;
  const int lc = lane >> 4;
  const int er = lane & 15;
  const int le = er < N ? er : N - 1;
  const bool val = (lc == 3);
  const bool live = er < N;
  const bool dir = (lc < 3) && live;
  const int nup = ka.nup;
  const T tstep = (T)ka.tstep;

  // ------------------------------------------------------------------ positions
  int pb = conf, pi = -1;
  if (ka.proposal) {
    pb = conf / N;
    pi = conf - pb * N;
  }
  if (lane < 3 * N) {
    T x = ((const T*)ka.pos)[(size_t)pb * 3 * N + lane];
    if (ka.proposal && lane / 3 == pi) {
      const T z = ((const T*)ka.gauss1)[(size_t)pb * 3 * N + lane];   // drawn by the host or k_draws
      const T ge = ((const T*)ka.pgrad)[(size_t)pb * 3 * N + lane] * (T)(*ka.taueff);   // never fused (not mc_step)
      x = x + (ge * tstep + f_sqrt(tstep) * z);
    }
    xs[lane] = x;
  }
  __syncthreads();

  // ------------------------------------------------------------------ per-electron stage (electron.h)
  ElecOut<T, A> eo;
  electron_stage<T, N, A>(P, xs + le * 3, le, lc, eo);
  const PJ<T>* hf = eo.hf;
  const PJ<T>* yst = eo.yst;
  const PJ<T> env = eo.env, jae = eo.jae;
  T vv = (val && live) ? eo.ven : T(0);
  // Yt row of electron le: env * (y . What)   (nn.py:449-452, 479-485)
  T Yd1[N], Yd2[N];
#pragma unroll
  for (int col = 0; col < N; ++col) {
    PJ<T> s = P[Ly::wy + col] * yst[0];
#pragma unroll
    for (int m = 1; m < NYW; ++m) s = s + P[Ly::wy + m * N + col] * yst[m];
    const PJ<T> yt = env * s;
    Yd1[col] = yt.d1;
    Yd2[col] = yt.d2;
    if (val && live) Yv[er * N + col] = yt.v;
  }
  T jd1 = dir ? jae.d1 : T(0);
  T jd2 = dir ? jae.d2 : T(0);
  T jv = (val && live) ? jae.v : T(0);

  // ------------------------------------------------------------------ h stream (3 layers)
  h_layer<T, N, A, LAP, 0>(P, xs, hb, hf, lane, lc, er, le, val, dir, live, nup, jd1, jd2, jv, vv);
  h_layer<T, N, A, LAP, 1>(P, xs, hb, hf, lane, lc, er, le, val, dir, live, nup, jd1, jd2, jv, vv);
  h_layer<T, N, A, LAP, 2>(P, xs, hb, hf, lane, lc, er, le, val, dir, live, nup, jd1, jd2, jv, vv);
  __syncthreads();

  // ------------------------------------------------------------------ orbital matrix A = Phi * Yt, [A | I]
  const int* rowsrc = ka.rowsrc;
  for (int idx = lane; idx < N * N; idx += 64) {
    const int r = idx / N, col = idx - r * N;
    const int src = rowsrc[r];
    const int sp = r < nup ? 0 : 1;
    T re = T(0), im = T(0);
#pragma unroll
    for (int f = 0; f < 4; ++f) {
      const T hv = hb[((src * 4 + f) * NC + 0) * 64 + 48];
      re += hv * P[Ly::orb_w + ((sp * 4 + f) * N + col) * 2 + 0];
      im += hv * P[Ly::orb_w + ((sp * 4 + f) * N + col) * 2 + 1];
    }
    re += P[Ly::orb_b + (sp * N + col) * 2 + 0];
    im += P[Ly::orb_b + (sp * N + col) * 2 + 1];
    Ph[idx * 2 + 0] = re;
    Ph[idx * 2 + 1] = im;
  }
  __syncthreads();

  // ------------------------------------------------------------------ Gauss-Jordan with partial pivoting
  // (replaces jnp.linalg.slogdet, network_blocks.py:156; pivot = first max |re|+|im| as LAPACK izamax)
  T logdet, phr, phi;
  gj_inverse<T, N>(Ph, Yv, Mx, lane, logdet, phr, phi);   // Mx now holds B = A^{-1} [N][N][2]
  __syncthreads();
#define BINV_RE(c, s) Mx[((c) * N + (s)) * 2]
#define BINV_IM(c, s) Mx[((c) * N + (s)) * 2 + 1]

  // ------------------------------------------------------------------ Q_f = P_f B  (diagonal only for gradients)
  if constexpr (LAP) {
    for (int idx = lane; idx < 4 * N * N; idx += 64) {
      const int f = idx / (N * N);
      const int rs = idx - f * N * N;
      const int r = rs / N, s = rs - r * N;
      const int sp = r < nup ? 0 : 1;
      T qr = T(0), qi = T(0);
      for (int c = 0; c < N; ++c) {
        const T yv = Yv[r * N + c];
        const T wr = P[Ly::orb_w + ((sp * 4 + f) * N + c) * 2] * yv;
        const T wi = P[Ly::orb_w + ((sp * 4 + f) * N + c) * 2 + 1] * yv;
        const T br = BINV_RE(c, s), bi = BINV_IM(c, s);
        qr += wr * br - wi * bi;
        qi += wr * bi + wi * br;
      }
      Qs[((r * N + s) * 4 + f) * 2] = qr;
      Qs[((r * N + s) * 4 + f) * 2 + 1] = qi;
    }
  } else {
    if (lane < 4 * N) {
      const int f = lane / N, r = lane - f * N;
      const int sp = r < nup ? 0 : 1;
      T qr = T(0), qi = T(0);
      for (int c = 0; c < N; ++c) {
        const T yv = Yv[r * N + c];
        const T wr = P[Ly::orb_w + ((sp * 4 + f) * N + c) * 2] * yv;
        const T wi = P[Ly::orb_w + ((sp * 4 + f) * N + c) * 2 + 1] * yv;
        const T br = BINV_RE(c, r), bi = BINV_IM(c, r);
        qr += wr * br - wi * bi;
        qi += wr * bi + wi * br;
      }
      Qs[(r * 4 + f) * 2] = qr;
      Qs[(r * 4 + f) * 2 + 1] = qi;
    }
  }
  __syncthreads();
  auto qdiag_re = [&](int r, int f) -> T {
    return LAP ? Qs[((r * N + r) * 4 + f) * 2] : Qs[(r * 4 + f) * 2];
  };

  // ------------------------------------------------------------------ per-direction contractions
  // gradient: sum_{r,f} U Re Q_f[r,r] + Re(w . b_e) + Jastrow
  T g = jd1;
#pragma unroll
  for (int r = 0; r < N; ++r) {
    const int src = rowsrc[r];
#pragma unroll
    for (int f = 0; f < 4; ++f) g += hb[((src * 4 + f) * NC + 0) * 64 + lane] * qdiag_re(r, f);
  }
  T wbr = T(0), wbi = T(0);
#pragma unroll
  for (int col = 0; col < N; ++col) {
    const T pr = Ph[(le * N + col) * 2], pim = Ph[(le * N + col) * 2 + 1];
    const T wr = pr * Yd1[col], wi = pim * Yd1[col];
    const T br = BINV_RE(col, le), bi = BINV_IM(col, le);
    wbr += wr * br - wi * bi;
    wbi += wr * bi + wi * br;
  }
  g += wbr;

  T lap = T(0);
  if constexpr (LAP) {
    // t1 = sum U2 Re Q_f[r,r]
    T t1 = T(0);
#pragma unroll
    for (int r = 0; r < N; ++r) {
      const int src = rowsrc[r];
#pragma unroll
      for (int f = 0; f < 4; ++f) t1 += hb[((src * 4 + f) * NC + 1) * 64 + lane] * qdiag_re(r, f);
    }
    // U of row le (this direction's electron row of the matrix)
    T Ue[4];
    {
      const int src = rowsrc[le];
#pragma unroll
      for (int f = 0; f < 4; ++f) Ue[f] = hb[((src * 4 + f) * NC + 0) * 64 + lane];
    }
    const int spe = le < nup ? 0 : 1;
    // t2 = Re sum_col (2 dPhi[e,col] Yt'[col] + Phi[e,col] Yt''[col]) B[col,e]
    T t2 = T(0);
#pragma unroll
    for (int col = 0; col < N; ++col) {
      T dpr = T(0), dpi = T(0);
#pragma unroll
      for (int f = 0; f < 4; ++f) {
        dpr += Ue[f] * P[Ly::orb_w + ((spe * 4 + f) * N + col) * 2];
        dpi += Ue[f] * P[Ly::orb_w + ((spe * 4 + f) * N + col) * 2 + 1];
      }
      const T pr = Ph[(le * N + col) * 2], pim = Ph[(le * N + col) * 2 + 1];
      const T xr = T(2) * dpr * Yd1[col] + pr * Yd2[col];
      const T xi = T(2) * dpi * Yd1[col] + pim * Yd2[col];
      t2 += xr * BINV_RE(col, le) - xi * BINV_IM(col, le);
    }
    // cross = Re sum_r z[r] sum_f U[r,f] Q_f[r,e]  with z = B^T w ;  ss = Re sum_{r,s} S_rs S_sr
    T cross = T(0), ss = T(0);
#pragma unroll 1
    for (int r = 0; r < N; ++r) {
      T ur[4];
      {
        const int src = rowsrc[r];
#pragma unroll
        for (int f = 0; f < 4; ++f) ur[f] = hb[((src * 4 + f) * NC + 0) * 64 + lane];
      }
      T zr = T(0), zi = T(0);
#pragma unroll
      for (int col = 0; col < N; ++col) {
        const T pr = Ph[(le * N + col) * 2], pim = Ph[(le * N + col) * 2 + 1];
        const T wr = pr * Yd1[col], wi = pim * Yd1[col];
        const T br = BINV_RE(col, r), bi = BINV_IM(col, r);
        zr += br * wr - bi * wi;
        zi += br * wi + bi * wr;
      }
      {
        T sr = T(0), si = T(0);
#pragma unroll
        for (int f = 0; f < 4; ++f) {
          sr += ur[f] * Qs[((r * N + le) * 4 + f) * 2];
          si += ur[f] * Qs[((r * N + le) * 4 + f) * 2 + 1];
        }
        cross += zr * sr - zi * si;
      }
      {
        T sr = T(0), si = T(0);
#pragma unroll
        for (int f = 0; f < 4; ++f) {
          sr += ur[f] * Qs[((r * N + r) * 4 + f) * 2];
          si += ur[f] * Qs[((r * N + r) * 4 + f) * 2 + 1];
        }
        ss += sr * sr - si * si;
      }
#pragma unroll 1
      for (int s = r + 1; s < N; ++s) {
        const int srcs = rowsrc[s];
        T ar = T(0), ai = T(0), br = T(0), bi = T(0);
#pragma unroll
        for (int f = 0; f < 4; ++f) {
          const T us = hb[((srcs * 4 + f) * NC + 0) * 64 + lane];
          ar += ur[f] * Qs[((r * N + s) * 4 + f) * 2];
          ai += ur[f] * Qs[((r * N + s) * 4 + f) * 2 + 1];
          br += us * Qs[((s * N + r) * 4 + f) * 2];
          bi += us * Qs[((s * N + r) * 4 + f) * 2 + 1];
        }
        ss += T(2) * (ar * br - ai * bi);
      }
    }
    lap = t1 + t2 - (ss + T(2) * cross + (wbr * wbr - wbi * wbi)) + jd2;
  }
#undef BINV_RE
#undef BINV_IM

  // ------------------------------------------------------------------ reductions + outputs
  const T gd = dir ? g : T(0);
  const T sumsq = wave_sum(gd * gd);
  const T lpsi = logdet + wave_sum(jv);
  if (ka.grad && dir) ((T*)ka.grad)[(size_t)conf * 3 * N + 3 * le + lc] = g;
  if (ka.gown && dir && le == pi) ((T*)ka.gown)[(size_t)conf * 3 + lc] = g;
  T el = T(0);
  if constexpr (LAP) {
    const T kin = T(-0.5) * wave_sum(dir ? (lap + g * g) : T(0));    // hamiltonian.py:126-127
    const T pot = wave_sum(vv) + P[Ly::vnn];
    el = pot + kin;
  }
  if (lane == 0) {
    if (ka.logabs) ((T*)ka.logabs)[conf] = lpsi;
    if (ka.phase) ((T*)ka.phase)[conf] = f_atan2(phi, phr);
    if (ka.sumsq) ((T*)ka.sumsq)[conf] = sumsq;
    if constexpr (LAP) {
      if (ka.el) ((T*)ka.el)[conf] = el;
    }
  }
}

}  // namespace aq
