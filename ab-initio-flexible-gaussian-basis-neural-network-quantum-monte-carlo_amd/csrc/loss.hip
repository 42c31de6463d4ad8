// loss.hip -- energy statistics and the energy-gradient (loss) levels of one training step:
// context-free kernels over a batch of local energies, each one workgroup with every sum in
// double and in a fixed order.  Entry points: aiqmc_energy_stats, aiqmc_energy_stats_final,
// aiqmc_loss_weights (one rank), aiqmc_loss_level / aiqmc_loss_pack / aiqmc_loss_final (several
// ranks, one all-reduce per level).
#include <hip/hip_runtime.h>

#include <cstdint>
#include <string>

#include "aiqmc.h"
#include "api_util.h"
#include "reduce.h"

using aq::block_sum;   // every sum below: reduce.h's butterfly-then-ordered form

// Energy statistics of one iteration (loss.py:206-208 through constants.pmean_stats), one
// workgroup: out[0..3] = [sum |e - m|^2, n m, n m^2, n] in fp64 (m = the mean of these n
// energies; the summed 4-vector of all ranks gives the pooled mean and variance), and with
// finalize (one rank) out[4..5] = [m, sum |e - m|^2 / n], the reference's two-pass values.
// k_energy_stats_final forms them from a summed 4-vector after the all-reduce (Chan's
// combination; products not contracted into FMAs, so one rank's between-term n m^2 - n m^2 is 0).
__device__ __forceinline__ void energy_stats_final(double* out) {
#pragma clang fp contract(off)
  const double mean = out[1] / out[3];
  double between = out[2] - out[3] * mean * mean;
  between = between > 0.0 ? between : 0.0;
  out[4] = mean;
  out[5] = (out[0] + between) / out[3];
}
template <typename T>
__global__ __launch_bounds__(1024) void k_energy_stats(const T* __restrict__ e, int64_t n, double* __restrict__ out,
                                                       int finalize) {
  __shared__ double red[16];
  double a = 0.0;
  for (int64_t i = threadIdx.x; i < n; i += blockDim.x) a += (double)e[i];
  const double nn = (double)n;
  const double m = block_sum(a, red) / nn;
  double q = 0.0;
  for (int64_t i = threadIdx.x; i < n; i += blockDim.x) {
    const double d = (double)e[i] - m;
    q += d * d;
  }
  q = block_sum(q, red);
  if (threadIdx.x == 0) {
    out[0] = q;
    out[1] = nn * m;
    out[2] = nn * m * m;
    out[3] = nn;
    if (finalize) {
      out[4] = m;
      out[5] = q / nn;
    }
  }
}
__global__ void k_energy_stats_final(double* out) {
  if (threadIdx.x == 0) energy_stats_final(out);
}

// The energy-gradient weights of make_loss on one rank (Loss/loss.py:73-135 clipping, :206-208
// statistics, :256-265 tangent), one workgroup, every sum in double and in a fixed order:
//   m = mean(e) (the loss), variance = mean |e - m|^2;
//   clip (scale > 0, centre m; clip_from_median = False): tv = mean |x - c| per component,
//     clipped x = clamp(x, c - scale tv, c + scale tv); centre of the differences
//     dc = mean(clipped) (center_at_clipped) or m; diff = clipped - dc; aux = dc;
//   no clip: diff = e - m, aux = e (total_energy's clipped_energy, kept as written);
//   w_re = wscale Re diff,  w_im = wscale Im(diff + aux)  (the d log|psi| and d phase weights);
//   clipped_out = dc + diff (aux.clipped_energy; dc = m without clipping);
//   stats = [m_re, m_im, variance, dc_re, dc_im].
// e_im / w_im / clipped_im may be null (real local energies).  Replaces ~25 small torch launches
// per training step (and the host sync of the complex check) on the single-rank path.
template <typename T>
__global__ __launch_bounds__(1024) void k_loss_weights(const T* __restrict__ er, const T* __restrict__ ei, int64_t n,
                                                       double clip, int center_at_clipped, double wscale,
                                                       T* __restrict__ wr, T* __restrict__ wi, T* __restrict__ cr,
                                                       T* __restrict__ ci, double* __restrict__ stats) {
  __shared__ double red[16];
  const double nn = (double)n;
  const bool cplx = ei != nullptr;
  double a = 0.0, b = 0.0;
  for (int64_t i = threadIdx.x; i < n; i += blockDim.x) {
    a += (double)er[i];
    if (cplx) b += (double)ei[i];
  }
  const double mr = block_sum(a, red) / nn;
  const double mi = cplx ? block_sum(b, red) / nn : 0.0;
  double q = 0.0, tr = 0.0, ti = 0.0;
  for (int64_t i = threadIdx.x; i < n; i += blockDim.x) {
    const double dr = (double)er[i] - mr, di = cplx ? (double)ei[i] - mi : 0.0;
    q += dr * dr + di * di;
    tr += fabs(dr);
    ti += fabs(di);
  }
  const double var = block_sum(q, red) / nn;
  const bool clipping = clip > 0.0;
  double lor = 0.0, hir = 0.0, loi = 0.0, hii = 0.0, dcr = mr, dci = mi;
  if (clipping) {
    const double tvr = block_sum(tr, red) / nn;
    const double tvi = cplx ? block_sum(ti, red) / nn : 0.0;
    lor = mr - clip * tvr;
    hir = mr + clip * tvr;
    loi = mi - clip * tvi;
    hii = mi + clip * tvi;
    if (center_at_clipped) {
      double sr = 0.0, si = 0.0;
      for (int64_t i = threadIdx.x; i < n; i += blockDim.x) {
        const double x = (double)er[i];
        sr += x < lor ? lor : (x > hir ? hir : x);
        if (cplx) {
          const double y = (double)ei[i];
          si += y < loi ? loi : (y > hii ? hii : y);
        }
      }
      dcr = block_sum(sr, red) / nn;
      dci = cplx ? block_sum(si, red) / nn : 0.0;
    }
  }
  for (int64_t i = threadIdx.x; i < n; i += blockDim.x) {
    const double x = (double)er[i], y = cplx ? (double)ei[i] : 0.0;
    double fr, fi, ar, ai;
    if (clipping) {
      const double xc = x < lor ? lor : (x > hir ? hir : x), yc = y < loi ? loi : (y > hii ? hii : y);
      fr = xc - dcr;
      fi = yc - dci;
      ar = dcr;
      ai = dci;
    } else {
      fr = x - mr;
      fi = y - mi;
      ar = x;
      ai = y;
    }
    wr[i] = (T)(wscale * fr);
    if (wi) wi[i] = (T)(wscale * (fi + ai));
    if (cr) cr[i] = (T)(dcr + fr);   // centre + diff (= e without clipping: dc = m)
    if (ci) ci[i] = (T)(dci + fi);
  }
  if (threadIdx.x == 0) {
    stats[0] = mr;
    stats[1] = mi;
    stats[2] = var;
    stats[3] = dcr;
    stats[4] = dci;
  }
}

// The energy-gradient statistics of make_loss over several ranks (Loss/loss.py:73-135 clipping,
// :206-208 statistics, :256-265 tangent, Optimizer/adam.py:55 gradient pmean), as three levels
// whose rank partials sum in ONE all-reduce each:
//   level 1  L1 = [sum |e - m_r|^2, n m_re, n m_im, n |m_r|^2, n, #(Im e != 0)]   (m_r: rank mean)
//            -> E = sum n m / sum n, var = (sum M2 + sum n|m_r|^2 - n|E|^2) / n  (Chan et al.)
//   level 2  L2 = [sum |Re e - Re E|, sum |Im e - Im E|]      (clipping only: the TV window)
//   level 3  L3 = [sum Re xc, sum Im xc, G (P), G0 (P)]         (xc = clipped energy)
//            G  = sum_b wscale (Re xc_b - Re E) dlog|psi_b| + sum_b wp_b dphase_b,
//            G0 = sum_b wscale dlog|psi_b|                      (center_at_clipped only)
//            -> dc = sum xc / n,  grad = (G - (Re dc - Re E) G0) / world
// since the weights of the reference, wscale Re(xc_b - dc), differ from G's by the constant
// (Re dc - Re E): the clipped mean rides in the gradient's all-reduce instead of one of its own.
// Phase weights need no centre: wscale Im(diff + aux) = wscale Im xc when clipping (aux = dc),
// wscale (2 Im e - Im E) without (aux = e).  One workgroup per stage, sums in double.
template <typename T>
__global__ __launch_bounds__(1024) void k_lossr_l1(const T* __restrict__ er, const T* __restrict__ ei, int64_t n,
                                                   double* __restrict__ L1) {
  __shared__ double red[16];
  const bool cplx = ei != nullptr;
  const double nn = (double)n;
  double a = 0.0, b = 0.0, z = 0.0;
  for (int64_t i = threadIdx.x; i < n; i += blockDim.x) {
    a += (double)er[i];
    if (cplx) {
      const double y = (double)ei[i];
      b += y;
      z += y != 0.0 ? 1.0 : 0.0;
    }
  }
  const double mr = block_sum(a, red) / nn;
  const double mi = cplx ? block_sum(b, red) / nn : 0.0;
  const double nz = cplx ? block_sum(z, red) : 0.0;
  double q = 0.0;
  for (int64_t i = threadIdx.x; i < n; i += blockDim.x) {
    const double dr = (double)er[i] - mr, di = cplx ? (double)ei[i] - mi : 0.0;
    q += dr * dr + di * di;
  }
  q = block_sum(q, red);
  if (threadIdx.x == 0) {
#pragma clang fp contract(off)
    L1[0] = q;
    L1[1] = nn * mr;
    L1[2] = nn * mi;
    L1[3] = nn * mr * mr + nn * mi * mi;
    L1[4] = nn;
    L1[5] = nz;
  }
}
// [E_re, E_im, variance] from a summed L1 (products not contracted, and the sum n mr^2 + n mi^2
// formed as level 1 forms L1[3] before it is subtracted -- (a + b) - a - b is not 0 in floating
// point: one rank's between-term is 0)
__device__ __forceinline__ void lossr_mean_var(const double* L1, double* er, double* ei, double* var) {
#pragma clang fp contract(off)
  const double ntot = L1[4];
  const double mr = L1[1] / ntot, mi = L1[2] / ntot;
  double between = L1[3] - (ntot * mr * mr + ntot * mi * mi);
  between = between > 0.0 ? between : 0.0;
  *er = mr;
  *ei = mi;
  *var = (L1[0] + between) / ntot;
}
template <typename T>
__global__ __launch_bounds__(1024) void k_lossr_l2(const T* __restrict__ er, const T* __restrict__ ei, int64_t n,
                                                   const double* __restrict__ L1, double* __restrict__ L2) {
  __shared__ double red[16];
  const bool cplx = ei != nullptr;
  double mr, mi, var;
  lossr_mean_var(L1, &mr, &mi, &var);
  double tr = 0.0, ti = 0.0;
  for (int64_t i = threadIdx.x; i < n; i += blockDim.x) {
    tr += fabs((double)er[i] - mr);
    if (cplx) ti += fabs((double)ei[i] - mi);
  }
  tr = block_sum(tr, red);
  ti = cplx ? block_sum(ti, red) : 0.0;
  if (threadIdx.x == 0) {
    L2[0] = tr;
    L2[1] = ti;
  }
}
// weights for the gradient pass: w[0][b] = wscale (Re xc_b - Re E), w[1][b] = wscale (G0, when
// g0), wp[b] = the phase weight (when wp); clipped_re/im = aux.clipped_energy = xc (the centre
// plus diff); L3[0..1] = sum xc.
template <typename T>
__global__ __launch_bounds__(1024) void k_lossr_l3(const T* __restrict__ er, const T* __restrict__ ei, int64_t n,
                                                   const double* __restrict__ L1, const double* __restrict__ L2,
                                                   double clip, double wscale, int g0, T* __restrict__ w,
                                                   T* __restrict__ wp, T* __restrict__ cr, T* __restrict__ ci,
                                                   double* __restrict__ L3) {
  __shared__ double red[16];
  const bool cplx = ei != nullptr;
  double mr, mi, var;
  lossr_mean_var(L1, &mr, &mi, &var);
  const bool clipping = clip > 0.0;
  const double ntot = L1[4];
  const double tvr = clipping ? L2[0] / ntot : 0.0, tvi = clipping ? L2[1] / ntot : 0.0;
  const double lor = mr - clip * tvr, hir = mr + clip * tvr, loi = mi - clip * tvi, hii = mi + clip * tvi;
  double sr = 0.0, si = 0.0;
  for (int64_t i = threadIdx.x; i < n; i += blockDim.x) {
    const double x = (double)er[i], y = cplx ? (double)ei[i] : 0.0;
    const double xc = clipping ? (x < lor ? lor : (x > hir ? hir : x)) : x;
    const double yc = clipping ? (y < loi ? loi : (y > hii ? hii : y)) : y;
    sr += xc;
    si += yc;
    w[i] = (T)(wscale * (xc - mr));
    if (g0) w[n + i] = (T)wscale;
    if (wp) wp[i] = (T)(wscale * (clipping ? yc : (y - mi) + y));
    if (cr) cr[i] = (T)xc;
    if (ci) ci[i] = (T)yc;
  }
  sr = block_sum(sr, red);
  si = cplx ? block_sum(si, red) : 0.0;
  if (threadIdx.x == 0) {
    L3[0] = sr;
    L3[1] = si;
  }
}
// L3[2..2+P) = g (+ gp), L3[2+P..2+2P) = g0 (when given), from the ctx-dtype gradient sums
template <typename T>
__global__ void k_lossr_pack(const T* __restrict__ g, const T* __restrict__ gp, const T* __restrict__ g0, int P,
                             double* __restrict__ L3) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= P) return;
  L3[2 + i] = (double)g[i] + (gp ? (double)gp[i] : 0.0);
  if (g0) L3[2 + P + i] = (double)g0[i];
}
// after the level-3 all-reduce: grad = (G - (Re dc - Re E) G0) / world in the ctx dtype;
// stats = [Re E, Im E, variance, Re dc, Im dc, #(Im e != 0)] (dc = E unless centred at xc)
template <typename T>
__global__ void k_lossr_final(const double* __restrict__ L1, const double* __restrict__ L3, int P, int g0,
                              int center_at_clipped, double inv_world, T* __restrict__ grad,
                              double* __restrict__ stats) {
  double mr, mi, var;
  lossr_mean_var(L1, &mr, &mi, &var);
  const double ntot = L1[4];
  const double dcr = center_at_clipped ? L3[0] / ntot : mr, dci = center_at_clipped ? L3[1] / ntot : mi;
  const double shift = g0 ? dcr - mr : 0.0;
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < P) grad[i] = (T)((L3[2 + i] - (g0 ? shift * L3[2 + P + i] : 0.0)) * inv_world);
  if (i == 0) {
    stats[0] = mr;
    stats[1] = mi;
    stats[2] = var;
    stats[3] = dcr;
    stats[4] = dci;
    stats[5] = L1[5];
  }
}

extern "C" {

int aiqmc_energy_stats(const void* e_l, int32_t dtype, int64_t n, double* out, int32_t finalize, void* stream) {
  if (n <= 0) return fail(AIQMC_EINVAL, "empty batch");
  if (!e_l || !out) return fail(AIQMC_EINVAL, "null argument");
  if (!is_dtype(dtype)) return fail(AIQMC_EINVAL, "dtype must be AIQMC_F32 or AIQMC_F64");
  by_dtype(dtype, [&](auto t) {
    using T = decltype(t);
    k_energy_stats<T><<<dim3(1), dim3(1024), 0, (hipStream_t)stream>>>((const T*)e_l, n, out, finalize != 0);
  });
  HIPCHK(hipGetLastError());
  return AIQMC_OK;
}

int aiqmc_loss_weights(const void* e_re, const void* e_im, int32_t dtype, int64_t n, double clip_scale,
                       int32_t center_at_clipped, double wscale, void* w_re, void* w_im, void* clipped_re,
                       void* clipped_im, double* stats, void* stream) {
  if (n <= 0) return fail(AIQMC_EINVAL, "empty batch");
  if (!e_re || !w_re || !stats) return fail(AIQMC_EINVAL, "null argument");
  if (!is_dtype(dtype)) return fail(AIQMC_EINVAL, "dtype must be AIQMC_F32 or AIQMC_F64");
  by_dtype(dtype, [&](auto t) {
    using T = decltype(t);
    k_loss_weights<T><<<dim3(1), dim3(1024), 0, (hipStream_t)stream>>>(
        (const T*)e_re, (const T*)e_im, n, clip_scale, center_at_clipped, wscale, (T*)w_re, (T*)w_im, (T*)clipped_re,
        (T*)clipped_im, stats);
  });
  HIPCHK(hipGetLastError());
  return AIQMC_OK;
}

int aiqmc_energy_stats_final(double* out, void* stream) {
  if (!out) return fail(AIQMC_EINVAL, "null argument");
  k_energy_stats_final<<<dim3(1), dim3(64), 0, (hipStream_t)stream>>>(out);
  HIPCHK(hipGetLastError());
  return AIQMC_OK;
}

int aiqmc_loss_level(int32_t level, const void* e_re, const void* e_im, int32_t dtype, int64_t n,
                     const double* L1, const double* L2, double clip_scale, double wscale, int32_t g0, void* w,
                     void* wp, void* clipped_re, void* clipped_im, double* out, void* stream) {
  if (n <= 0) return fail(AIQMC_EINVAL, "empty batch");
  if (!e_re || !out) return fail(AIQMC_EINVAL, "null argument");
  if (!is_dtype(dtype)) return fail(AIQMC_EINVAL, "dtype must be AIQMC_F32 or AIQMC_F64");
  if (level == 2 && !L1) return fail(AIQMC_EINVAL, "level 2 needs the summed level-1 vector");
  if (level == 3 && (!L1 || !w || (clip_scale > 0.0 && !L2)))
    return fail(AIQMC_EINVAL, "level 3 needs L1, L2 (clipping) and w");
  if (level < 1 || level > 3) return fail(AIQMC_EINVAL, "level must be 1, 2 or 3");
  by_dtype(dtype, [&](auto t) {
    using T = decltype(t);
    const dim3 one(1), wg(1024);
    hipStream_t s = (hipStream_t)stream;
    const T *er = (const T*)e_re, *ei = (const T*)e_im;
    if (level == 1)
      k_lossr_l1<T><<<one, wg, 0, s>>>(er, ei, n, out);
    else if (level == 2)
      k_lossr_l2<T><<<one, wg, 0, s>>>(er, ei, n, L1, out);
    else
      k_lossr_l3<T><<<one, wg, 0, s>>>(er, ei, n, L1, L2, clip_scale, wscale, g0, (T*)w, (T*)wp, (T*)clipped_re,
                                       (T*)clipped_im, out);
  });
  HIPCHK(hipGetLastError());
  return AIQMC_OK;
}

int aiqmc_loss_pack(const void* g, const void* gp, const void* g0, int32_t dtype, int32_t P, double* L3,
                    void* stream) {
  if (!g || !L3 || P <= 0) return fail(AIQMC_EINVAL, "null argument");
  if (!is_dtype(dtype)) return fail(AIQMC_EINVAL, "dtype must be AIQMC_F32 or AIQMC_F64");
  by_dtype(dtype, [&](auto t) {
    using T = decltype(t);
    k_lossr_pack<T><<<blocks(P, 256), dim3(256), 0, (hipStream_t)stream>>>((const T*)g, (const T*)gp, (const T*)g0, P,
                                                                          L3);
  });
  HIPCHK(hipGetLastError());
  return AIQMC_OK;
}

int aiqmc_loss_final(const double* L1, const double* L3, int32_t P, int32_t g0, int32_t center_at_clipped,
                     int32_t world, int32_t dtype, void* grad, double* stats, void* stream) {
  if (!L1 || !L3 || !grad || !stats || P <= 0 || world <= 0) return fail(AIQMC_EINVAL, "null argument");
  if (!is_dtype(dtype)) return fail(AIQMC_EINVAL, "dtype must be AIQMC_F32 or AIQMC_F64");
  const double iw = 1.0 / (double)world;
  by_dtype(dtype, [&](auto t) {
    using T = decltype(t);
    k_lossr_final<T><<<blocks(P, 256), dim3(256), 0, (hipStream_t)stream>>>(L1, L3, P, g0, center_at_clipped, iw,
                                                                           (T*)grad, stats);
  });
  HIPCHK(hipGetLastError());
  return AIQMC_OK;
}

}  // extern "C"
