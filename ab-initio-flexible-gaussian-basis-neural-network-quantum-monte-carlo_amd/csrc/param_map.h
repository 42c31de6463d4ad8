// param_map.h -- the correspondence between the canonical tree_flatten parameter vector (see
// include/aiqmc.h) and the kernel layout Lay<N,A> (layout.h), written once.  Host-only plain C++.
//
// build_param_map is the only walk of the canonical order in csrc/.  It yields, per kernel-layout
// entry, the program both parameter uploads run (pack_apply on the host for aiqmc_set_params,
// k_pack_params on the device for aiqmc_set_params_device), and from it the canonical -> kernel
// index map of the parameter gradient (k_grad_canon).
#pragma once
#include <cmath>
#include <cstdint>
#include <vector>

#include "layout.h"

// hidden visibility: the library's dynamic symbol table is the C-ABI of include/aiqmc.h
#pragma GCC visibility push(hidden)

struct ParamMap {
  int64_t ncanon = 0;           // canonical parameters
  int nkern = 0, nprm = 0;      // Lay::total, Lay::total_ext
  int wy_off = 0, wy_src0 = 0;  // Lay::wy; canonical index of W_y[0][0]
  std::vector<int> op;          // [nprm] 0 constant, 1 copy, 2 row-normalised W_y (k_pack_params' codes)
  std::vector<int> src;         // [nprm] canonical source of a copy / W_y entry
  std::vector<double> cval;     // [nprm] value of a constant (padding: 0)
  std::vector<int> gmap;        // [ncanon] canonical -> kernel index; -1 unused; -2-k for W_y (k_grad_canon's codes)
};

// par / anti: [2][npar] / [2][nanti] electron pairs (aiqmc_cfg); atoms [A][3], charges [A].
// The derived constants (Jastrow e-e cusps Jastrow.py:23-41, (2Z)^{3/4}, (2Z)^{1/4} Jastrow.py:95,
// V_nn) are formed here in double.
template <int N, int A>
void build_param_map(int npar, int nanti, const int* par, const int* anti, const double* atoms,
                     const double* charges, ParamMap& m) {
  using namespace aq;
  using Ly = Lay<N, A>;
  m.nkern = Ly::total;
  m.nprm = Ly::total_ext;
  m.wy_off = Ly::wy;
  m.op.assign(Ly::total_ext, 0);
  m.src.assign(Ly::total_ext, 0);
  m.cval.assign(Ly::total_ext, 0.0);
  int j = 0;   // the canonical cursor
  auto copy = [&](int k) { m.op[k] = 1, m.src[k] = j; };   // kernel entry k copies canonical j
  // envelope[i]: alpha, beta, eplion, mu, nu, pi, sigma, xi (sorted keys)
  for (int i = 0; i < N; ++i) {
    copy(Ly::env_alpha + i), ++j;
    for (int a = 0; a < A; ++a, ++j) copy(Ly::env_beta + i * A + a);
    j += 3 * A + A + A;   // eplion, mu, nu (unused by envelope.apply)
    for (int k = 0; k < 3 * A; ++k, ++j) copy(Ly::env_pi + i * A * 3 + k);
    for (int k = 0; k < 3 * A; ++k, ++j) copy(Ly::env_sigma + i * A * 3 + k);
    copy(Ly::env_xi + i), ++j;
  }
  // jastrow_ae
  for (int k = 0; k < N * A; ++k, ++j) copy(Ly::jae_b + k);
  // jastrow_ee: ee_anti, then ee_par; a pair parameter feeds both [i][j] and [j][i]
  auto pairs = [&](const int* t, int n, double cusp) {
    for (int q = 0; q < n; ++q, ++j) {
      const int i = t[q], k = t[n + q];
      m.cval[Ly::jee_c + i * N + k] = m.cval[Ly::jee_c + k * N + i] = cusp;
      copy(Ly::jee_a + i * N + k), copy(Ly::jee_a + k * N + i);
    }
  };
  pairs(anti, nanti, 0.5);
  pairs(par, npar, 0.25);
  // layers.input = {} ; layers.streams[l] = {convolutional{b,w}, double{b,w}, single{b,w}}; a conv
  // or single weight feeds its Lay entry and its lane-order copies (layout.h x* blocks)
  const int D[3] = {Ly::D0, Ly::D1, Ly::D1};
  const int Q[3] = {Ly::Q0, Ly::Q1, Ly::Q1};
  const int cw[3] = {Ly::conv_w0, Ly::conv_w1, Ly::conv_w2};
  const int cb[3] = {Ly::conv_b0, Ly::conv_b1, Ly::conv_b2};
  const int sw[3] = {Ly::sng_w0, Ly::sng_w1, Ly::sng_w2};
  const int sb[3] = {Ly::sng_b0, Ly::sng_b1, Ly::sng_b2};
  const int dw[2] = {Ly::dbl_w0, Ly::dbl_w1};
  const int db[2] = {Ly::dbl_b0, Ly::dbl_b1};
  for (int l = 0; l < 3; ++l) {
    const int QF = Q[l] / 4;   // full quads of conv outputs
    for (int i = 0; i < N; ++i)
      for (int q = 0; q < Q[l]; ++q, ++j) {
        copy(cb[l] + i * Q[l] + q);
        if (q < 4 * QF) copy(Ly::xcb(l) + (i * 4 + q % 4) * Ly::XB + q / 4);
        else
          for (int f = 0; f < 4; ++f) copy(Ly::xcb(l) + (i * 4 + f) * Ly::XB + QF + q - 4 * QF);
      }
    for (int i = 0; i < N; ++i)
      for (int d = 0; d < D[l]; ++d, ++j) {
        copy(cw[l] + i * D[l] + d);
        copy(Ly::xcw(l) + (i * 4 + d % 4) * Ly::XQ + d / 4);
      }
    if (l < 2) {
      for (int k = 0; k < NH2; ++k, ++j) copy(db[l] + k);
      for (int k = 0; k < NH2 * NH2; ++k, ++j) copy(dw[l] + k);
    }
    for (int k = 0; k < NH; ++k, ++j) copy(sb[l] + k);
    for (int q = 0; q < Q[l]; ++q)
      for (int f = 0; f < NH; ++f, ++j) {
        copy(sw[l] + q * NH + f);
        copy(Ly::xsw(l) + f * Ly::XQ + q);
        copy(Ly::xsr(l) + q * 4 + f);
      }
  }
  // layers.streams_y[l].single_Ynlm {b, w}
  const int yin[3] = {Ly::DY0, NYW, NYW};
  const int yw[3] = {Ly::y_w0, Ly::y_w1, Ly::y_w2};
  const int yb[3] = {Ly::y_b0, Ly::y_b1, Ly::y_b2};
  for (int l = 0; l < 3; ++l) {
    for (int k = 0; k < NYW; ++k, ++j) copy(yb[l] + k);
    for (int k = 0; k < yin[l] * NYW; ++k, ++j) copy(yw[l] + k);
  }
  // orbitals[s] {b [2N], w [4][2N]} ; complex = even + i odd (nn.py:456)
  for (int s = 0; s < 2; ++s) {
    for (int col = 0; col < N; ++col)
      for (int ri = 0; ri < 2; ++ri, ++j) copy(Ly::orb_b + (s * N + col) * 2 + ri);
    for (int f = 0; f < NH; ++f)
      for (int col = 0; col < N; ++col)
        for (int ri = 0; ri < 2; ++ri, ++j) copy(Ly::orb_w + ((s * NH + f) * N + col) * 2 + ri);
  }
  // y[0].w [6][N], row-normalised (nn.py:449-451)
  m.wy_src0 = j;
  for (int k = 0; k < NYW * N; ++k, ++j) m.op[Ly::wy + k] = 2, m.src[Ly::wy + k] = j;
  m.ncanon = j;
  // system constants
  for (int a = 0; a < A; ++a) {
    for (int d = 0; d < 3; ++d) m.cval[Ly::atoms + a * 3 + d] = atoms[a * 3 + d];
    m.cval[Ly::charges + a] = charges[a];
    m.cval[Ly::c34 + a] = std::pow(2.0 * charges[a], 0.75);
    m.cval[Ly::c14 + a] = std::pow(2.0 * charges[a], 0.25);
  }
  double vnn = 0.0;
  for (int a = 0; a < A; ++a)
    for (int b = a + 1; b < A; ++b) {
      double r2 = 0.0;
      for (int d = 0; d < 3; ++d) {
        const double t = atoms[a * 3 + d] - atoms[b * 3 + d];
        r2 += t * t;
      }
      vnn += charges[a] * charges[b] / std::sqrt(r2);
    }
  m.cval[Ly::vnn] = vnn;
  // gmap[j]: the lowest kernel index below nkern that copies j (the i < j entry of jee_a; never a
  // lane-order copy, those sit at >= x0 > total), -1 where nothing does, -2-k for the W_y block
  m.gmap.assign(m.ncanon, -1);
  for (int k = m.nkern - 1; k >= 0; --k)
    if (m.op[k] == 1) m.gmap[m.src[k]] = k;
  for (int k = 0; k < NYW * N; ++k) m.gmap[m.wy_src0 + k] = -2 - k;
}

// |W_y row| of N columns: double, ascending columns, the product and the sum rounded apart (no
// fused multiply-add), as k_pack_params forms it, so that host and device agree bitwise
inline double wy_row_norm(const double* row, int N) {
#pragma clang fp contract(off)
  double a = 0.0;
  for (int col = 0; col < N; ++col) {
    const double w = row[col];
    a += w * w;
  }
  return std::sqrt(a);
}

// The host side of the program: out [nprm] in the kernel layout, wnorm the six |W_y row|.  Per
// entry this is k_pack_params' body.
inline void pack_apply(const ParamMap& m, int N, const double* flat, std::vector<double>& out, double wnorm[aq::NYW]) {
  for (int r = 0; r < aq::NYW; ++r) wnorm[r] = wy_row_norm(flat + m.wy_src0 + r * N, N);
  out.resize(m.nprm);
  for (int k = 0; k < m.nprm; ++k) {
    const int o = m.op[k];
    out[k] = o == 0 ? m.cval[k] : o == 1 ? flat[m.src[k]] : flat[m.src[k]] / wnorm[(k - m.wy_off) / N];
  }
}

#pragma GCC visibility pop
