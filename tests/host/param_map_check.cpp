// param_map_check.cpp -- stand-alone host check of csrc/param_map.h (built and run by
// tests/test_capi_cpu.py::test_param_map_host_check under -fsanitize=address,undefined).
// Everything here is restated from the canonical tree_flatten order (include/aiqmc.h) and the
// layout.h comments, not taken from build_param_map.
#include <cstdio>
#include <vector>

#include "param_map.h"

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

// alternating spins (+, -, +, ...): pairs i < j in row-major order, parallel where i + j is even
static void spin_tables(int N, std::vector<int>& par, std::vector<int>& anti) {
  std::vector<int> pi, pj, ai, aj;
  for (int i = 0; i < N; ++i)
    for (int j = i + 1; j < N; ++j) {
      ((i + j) % 2 == 0 ? pi : ai).push_back(i);
      ((i + j) % 2 == 0 ? pj : aj).push_back(j);
    }
  par = pi, par.insert(par.end(), pj.begin(), pj.end());
  anti = ai, anti.insert(anti.end(), aj.begin(), aj.end());
}

template <int N, int A>
static ParamMap make_map() {
  std::vector<int> par, anti;
  spin_tables(N, par, anti);
  std::vector<double> atoms, charges;
  for (int a = 0; a < A; ++a) {
    for (int d = 0; d < 3; ++d) atoms.push_back(0.4 + 1.1 * a - 0.3 * d);
    charges.push_back(1.0 + 2.0 * a);
  }
  ParamMap m;
  build_param_map<N, A>((int)par.size() / 2, (int)anti.size() / 2, par.data(), anti.data(), atoms.data(),
                        charges.data(), m);
  return m;
}

template <int N, int A>
static void check() {
  using Ly = Lay<N, A>;
  const ParamMap m = make_map<N, A>();
  const int before = g_bad;
  // the canonical count, block by block
  const int d0 = 3 * 4 * A + 2 * 4, d1 = 3 * 4 + 2 * 4;   // conv input widths; outputs d / 4
  const long env = (long)N * (1 + A + 3 * A + A + A + 3 * A + 3 * A + 1);
  const long jae = (long)N * A, jee = (long)N * (N - 1) / 2;
  const long s0 = N * (d0 / 4) + N * d0 + (4 + 16) + (4 + d0 / 4 * 4);
  const long s1 = N * (d1 / 4) + N * d1 + (4 + 16) + (4 + d1 / 4 * 4);
  const long s2 = N * (d1 / 4) + N * d1 + (4 + d1 / 4 * 4);
  const long sy = (6 + (4 * A + 2) * 6) + 2 * (6 + 36);
  const long orb = 2 * (2 * N + 4 * 2 * N), y = 6 * N;
  const long want = env + jae + jee + s0 + s1 + s2 + sy + orb + y;
  REQ(m.ncanon == want, "ncanon %lld, counted %ld", (long long)m.ncanon, want);
  REQ(m.nkern == Ly::total && m.nprm == Ly::total_ext && m.wy_off == Ly::wy, "sizes");
  REQ((long)m.op.size() == m.nprm && (long)m.src.size() == m.nprm && (long)m.cval.size() == m.nprm, "vector sizes");
  REQ((long)m.gmap.size() == m.ncanon, "gmap size");
  REQ(m.wy_src0 == m.ncanon - 6 * N, "wy_src0 %d", m.wy_src0);
  if (g_bad != before) return;   // the checks below index by these sizes

  // every canonical index feeds an entry below nkern, except eplion / mu / nu of each electron:
  // exactly the gmap == -1 indices
  std::vector<int> fed(m.ncanon, 0);
  for (int k = 0; k < m.nkern; ++k)
    if (m.op[k] != 0) {
      REQ(m.src[k] >= 0 && m.src[k] < m.ncanon, "src[%d] = %d", k, m.src[k]);
      if (m.src[k] >= 0 && m.src[k] < m.ncanon) ++fed[m.src[k]];
    }
  const int per = 2 + 12 * A;
  int nunused = 0;
  for (int j = 0; j < m.ncanon; ++j) {
    const int r = j % per;
    const bool unused = j < N * per && r >= 1 + A && r < 1 + A + 5 * A;
    nunused += unused;
    REQ((fed[j] == 0) == unused, "canonical %d feeds %d entries", j, fed[j]);
    REQ((m.gmap[j] == -1) == unused, "gmap[%d] = %d", j, m.gmap[j]);
  }
  REQ(nunused == 5 * A * N, "unused %d", nunused);
  // gmap >= 0 names a copy of j; the -2-k codes cover the W_y block once each
  std::vector<int> seen(6 * N, 0);
  for (int j = 0; j < m.ncanon; ++j) {
    const int g = m.gmap[j];
    if (g >= 0) REQ(g < m.nkern && m.src[g] == j && m.op[g] == 1, "gmap[%d] = %d", j, g);
    if (g <= -2) {
      REQ(-2 - g < 6 * N, "gmap[%d] = %d", j, g);
      if (-2 - g < 6 * N) ++seen[-2 - g];
    }
  }
  for (int k = 0; k < 6 * N; ++k) {
    REQ(seen[k] == 1, "W_y code %d seen %d times", k, seen[k]);
    REQ(m.op[m.wy_off + k] == 2 && m.src[m.wy_off + k] == m.wy_src0 + k, "W_y entry %d", k);
    REQ(m.gmap[m.wy_src0 + k] == -2 - k, "gmap of W_y %d", k);
  }
  // lane-order copies mirror their Lay entries (layout.h); everything else past nkern is a constant 0
  std::vector<int> lane(m.nprm, 0);   // 1: checked as a copy
  auto mirrors = [&](int x, int k, const char* what) {
    REQ(m.op[x] == 1 && m.op[k] == 1 && m.src[x] == m.src[k], "%s: entry %d vs Lay entry %d", what, x, k);
    lane[x] = 1;
  };
  const int D[3] = {Ly::D0, Ly::D1, Ly::D1}, Q[3] = {Ly::Q0, Ly::Q1, Ly::Q1};
  const int cw[3] = {Ly::conv_w0, Ly::conv_w1, Ly::conv_w2}, cb[3] = {Ly::conv_b0, Ly::conv_b1, Ly::conv_b2};
  const int sw[3] = {Ly::sng_w0, Ly::sng_w1, Ly::sng_w2};
  for (int l = 0; l < 3; ++l) {
    for (int i = 0; i < N; ++i)
      for (int f = 0; f < 4; ++f) {
        // xcw: w[i][4 q + f]
        for (int q = 0; q < Q[l]; ++q) mirrors(Ly::xcw(l) + (i * 4 + f) * Ly::XQ + q, cw[l] + i * D[l] + 4 * q + f, "xcw");
        // xcb: b[i][4 s + f] for the Q / 4 full quads s, then b[i][q] for the Q mod 4 remainder
        for (int s = 0; s < Q[l] / 4; ++s) mirrors(Ly::xcb(l) + (i * 4 + f) * Ly::XB + s, cb[l] + i * Q[l] + 4 * s + f, "xcb quad");
        for (int r = 0; r < Q[l] % 4; ++r)
          mirrors(Ly::xcb(l) + (i * 4 + f) * Ly::XB + Q[l] / 4 + r, cb[l] + i * Q[l] + Q[l] / 4 * 4 + r, "xcb rem");
      }
    for (int q = 0; q < Q[l]; ++q)
      for (int f = 0; f < 4; ++f) {
        mirrors(Ly::xsw(l) + f * Ly::XQ + q, sw[l] + q * 4 + f, "xsw");   // w[q][f]
        mirrors(Ly::xsr(l) + q * 4 + f, sw[l] + q * 4 + f, "xsr");        // w[q][0..3]
      }
  }
  for (int k = m.nkern; k < m.nprm; ++k)
    if (!lane[k]) REQ(m.op[k] == 0 && m.cval[k] == 0.0, "padding entry %d: op %d cval %g", k, m.op[k], m.cval[k]);
  std::printf("(%d,%d) ncanon %lld nkern %d nprm %d: %s\n", N, A, (long long)m.ncanon, m.nkern, m.nprm,
              g_bad == before ? "ok" : "FAILED");
}

// (2,1) with flat[j] = j + 1: canonical order by hand.  Envelope of electron 0 at 0..13 (alpha 0,
// beta 1, eplion 2-4, mu 5, nu 6, pi 7-9, sigma 10-12, xi 13), of electron 1 at 14..27; jastrow_ae
// 28-29; ee_anti 30 (the one pair is antiparallel); streams[0] conv b 31-40, conv w 41-80, ...;
// orbitals[0] b 419-422, w 423-438; orbitals[1] b 439-442, w 443-458; y 459-470.
static void check_h2_values() {
  using Ly = Lay<2, 1>;
  const ParamMap m = make_map<2, 1>();
  const int before = g_bad;
  REQ(m.ncanon == 471, "ncanon %lld", (long long)m.ncanon);
  if (m.ncanon != 471) return;
  std::vector<double> flat(471), out;
  for (int j = 0; j < 471; ++j) flat[j] = j + 1;
  double wn[NYW];
  pack_apply(m, 2, flat.data(), out, wn);
  auto expect = [&](const char* what, int off, std::vector<double> v) {
    for (size_t k = 0; k < v.size(); ++k) REQ(out[off + k] == v[k], "%s[%zu] = %g, expected %g", what, k, out[off + k], v[k]);
  };
  expect("env_alpha", Ly::env_alpha, {1, 15});
  expect("env_sigma", Ly::env_sigma, {11, 12, 13, 25, 26, 27});
  expect("jee_a", Ly::jee_a, {0, 31, 31, 0});
  expect("jee_c", Ly::jee_c, {0, 0.5, 0.5, 0});
  expect("orb_w", Ly::orb_w, {424, 425, 426, 427, 428, 429, 430, 431, 432, 433, 434, 435, 436, 437, 438, 439,
                              444, 445, 446, 447, 448, 449, 450, 451, 452, 453, 454, 455, 456, 457, 458, 459});
  expect("orb_b", Ly::orb_b, {420, 421, 422, 423, 440, 441, 442, 443});
  expect("xcw record 0", Ly::xcw(0), {42, 46, 50, 54, 58, 0, 0, 0});
  // W_y row 0 = (460, 461): |row| = sqrt(460^2 + 461^2) = sqrt(424121)
  REQ(wn[0] == std::sqrt(424121.0), "wnorm[0] = %.17g", wn[0]);
  REQ(out[Ly::wy] == 460.0 / std::sqrt(424121.0), "wy[0] = %.17g", out[Ly::wy]);
  std::printf("(2,1) values: %s\n", g_bad == before ? "ok" : "FAILED");
}

int main() {
  check<2, 1>();
  check<3, 1>();
  check<4, 2>();
  check<5, 3>();
  check<8, 2>();
  check<10, 5>();
  check<14, 2>();
  check<16, 3>();
  check_h2_values();
  std::printf("param_map_check: %d failures\n", g_bad);
  return g_bad != 0;
}
