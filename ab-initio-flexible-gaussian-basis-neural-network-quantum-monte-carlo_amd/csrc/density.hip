// density.hip -- where the electrons are: spin-resolved density and pair-distance histograms of a
// batch of walkers, added into a caller-owned int64 accumulator that lives on the device across
// sweeps (aiqmc_density_layout, aiqmc_density_accumulate).  This is the DIAGONAL of the one-body
// density matrix; it needs nothing but the walkers.
//
// Accumulator layout (int64 words, aiqmc_density_layout's offsets8 in this order):
//   total[1]  skipped[1]  grid[2 nx ny nz]  grid_out[2]  radial[2 A rad_n]  radial_out[2 A]
//   pair[3 pair_n]  pair_out[3]
// A family with zero bins is absent together with its outside words.  Channels: grid and radial
// 0 = the up slots, 1 = the down slots of the context's spin tables (d_rowsrc: up slots then down
// slots, as k_s2_exchange reads them), pair 0 = up-up, 1 = down-down, 2 = up-down over i < j.
//
// Bin rule, in the context dtype T: f = (x - lo) * inv_h (distances: f = r * inv_h), inv_h =
// n / (hi - lo) formed in double on the host and rounded to T once; inside iff f >= 0 && f < n, bin
// (int)floor(f).  Everything else (NaN and infinite coordinates included: both comparisons fail) is
// tallied in the channel's outside word.  A grid sample is inside iff all three axes are.
//
// Fixed point: the words count in units of 2^-32.  A sample of a walker of weight w adds
// llrint((double)w * 2^32), exactly 1 << 32 without weights; `total` sums the walker weights in the
// same units.  A walker whose weight is negative, not finite or >= 2^31 adds nothing and is counted
// in the plain integer `skipped`.  Capacity: 2^31 units of weight per word before the int64 wraps.
// All updates are integer adds, so the words are the same bits for any launch shape, any chunking
// of the batch, any walker order, either path below and any number of ranks.
//
// One launch of 256-thread workgroups, each over a contiguous range of walkers; per walker N
// electron items (one grid update and A radial updates) and N (N - 1) / 2 pair items.  The grid goes
// straight to 64-bit global atomics (its updates spread over many addresses).  The small families
// (radial, radial_out, pair, pair_out: contiguous in the layout) are privatised per workgroup in LDS
// with 64-bit LDS atomic adds and flushed with one global atomic per non-zero word, when they hold
// at most DENS_LDS_WORDS words (32 KiB of LDS); above that they too take global atomics.  total,
// skipped and grid_out (4 words) are always privatised.  No workspace: the context gets no buffer.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <string>

#include "aiqmc.h"
#include "api_util.h"

namespace {

constexpr int DENS_LDS_WORDS = AIQMC_DENSITY_LDS_WORDS;   // privatisation limit of the small families
constexpr int DENS_MAX_A = 8;                             // atoms passed by value in the launch arguments
constexpr int DENS_MAX_N = 16;
constexpr int DENS_WPB = 32;                              // walkers per workgroup, at least
constexpr int DENS_HDR = 4;                               // LDS header: total, skipped, grid_out[2]
constexpr double DENS_ONE = 4294967296.0;                 // 2^32

struct DensArgs {
  double atoms[3 * DENS_MAX_A];
  double lo[3], inv_h[3], rad_inv, pair_inv;
  int n[3], rad_n, pair_n;
  int N, A, nup, B, wpb;
  int64_t off_grid, off_grid_out, off_rad, off_rad_out, off_pair, off_pair_out, n_small;
};

typedef unsigned long long u64;

// sm: [DENS_HDR] header, then (PRIV) the n_small words of the small families
template <typename T, bool PRIV>
__global__ __launch_bounds__(256) void k_density(const T* __restrict__ pos, const T* __restrict__ wts,
                                                 const int* __restrict__ rowsrc, DensArgs a, u64* __restrict__ acc) {
  extern __shared__ u64 sm[];
  __shared__ int chan[DENS_MAX_N];
  const int tid = threadIdx.x;
  const int nsm = DENS_HDR + (PRIV ? (int)a.n_small : 0);
  for (int k = tid; k < nsm; k += 256) sm[k] = 0;
  if (tid < DENS_MAX_N) chan[tid] = 1;
  __syncthreads();
  if (tid < a.nup) {
    const int e = rowsrc[tid];
    if (e >= 0 && e < a.N) chan[e] = 0;
  }
  __syncthreads();
  u64* small = PRIV ? sm + DENS_HDR : acc + a.off_rad;   // word k of the small families
  const int rel_rad_out = (int)(a.off_rad_out - a.off_rad);
  const int rel_pair = (int)(a.off_pair - a.off_rad), rel_pair_out = (int)(a.off_pair_out - a.off_rad);
  const bool has_grid = a.n[0] > 0;
  const int N = a.N, items = N + N * (N - 1) / 2;
  const int b0 = blockIdx.x * a.wpb;
  const int nb = a.B - b0 < a.wpb ? a.B - b0 : a.wpb;
  const int64_t nt = (int64_t)nb * items;
  for (int64_t t = tid; t < nt; t += 256) {
    const int wl = (int)(t / items), it = (int)(t - (int64_t)wl * items);
    const int b = b0 + wl;
    u64 q = (u64)1 << 32;
    if (wts) {
      const double w = (double)wts[b];
      if (!(w >= 0.0 && w < 2147483648.0)) {
        if (it == 0) atomicAdd(&sm[1], (u64)1);
        continue;
      }
      q = (u64)llrint(w * DENS_ONE);
    }
    if (it == 0) atomicAdd(&sm[0], q);
    const T* x = pos + (size_t)b * 3 * N;
    if (it < N) {
      const int ch = chan[it];
      const T r0 = x[3 * it], r1 = x[3 * it + 1], r2 = x[3 * it + 2];
      if (has_grid) {
        const T f0 = (r0 - (T)a.lo[0]) * (T)a.inv_h[0], f1 = (r1 - (T)a.lo[1]) * (T)a.inv_h[1],
                f2 = (r2 - (T)a.lo[2]) * (T)a.inv_h[2];
        if (f0 >= T(0) && f0 < (T)a.n[0] && f1 >= T(0) && f1 < (T)a.n[1] && f2 >= T(0) && f2 < (T)a.n[2]) {
          const int64_t g = (((int64_t)ch * a.n[0] + (int)floor(f0)) * a.n[1] + (int)floor(f1)) * a.n[2] + (int)floor(f2);
          atomicAdd(&acc[a.off_grid + g], q);
        } else {
          atomicAdd(&sm[2 + ch], q);
        }
      }
      if (a.rad_n > 0) {
        for (int at = 0; at < a.A; ++at) {
          const T d0 = r0 - (T)a.atoms[3 * at], d1 = r1 - (T)a.atoms[3 * at + 1], d2 = r2 - (T)a.atoms[3 * at + 2];
          const T f = sqrt(d0 * d0 + d1 * d1 + d2 * d2) * (T)a.rad_inv;
          const int c = ch * a.A + at;
          if (f >= T(0) && f < (T)a.rad_n) atomicAdd(&small[c * a.rad_n + (int)floor(f)], q);
          else atomicAdd(&small[rel_rad_out + c], q);
        }
      }
    } else if (a.pair_n > 0) {
      int i = 0, rem = it - N;   // pair (i, j), i < j, rows in ascending i
      while (rem >= N - 1 - i) {
        rem -= N - 1 - i;
        ++i;
      }
      const int j = i + 1 + rem;
      const int ch = chan[i] == chan[j] ? chan[i] : 2;
      const T d0 = x[3 * i] - x[3 * j], d1 = x[3 * i + 1] - x[3 * j + 1], d2 = x[3 * i + 2] - x[3 * j + 2];
      const T f = sqrt(d0 * d0 + d1 * d1 + d2 * d2) * (T)a.pair_inv;
      if (f >= T(0) && f < (T)a.pair_n) atomicAdd(&small[rel_pair + ch * a.pair_n + (int)floor(f)], q);
      else atomicAdd(&small[rel_pair_out + ch], q);
    }
  }
  __syncthreads();
  if (tid < DENS_HDR) {
    const u64 v = sm[tid];
    if (v && (tid < 2 || has_grid)) atomicAdd(&acc[tid < 2 ? tid : a.off_grid_out + (tid - 2)], v);
  }
  if (PRIV) {
    for (int k = tid; k < (int)a.n_small; k += 256) {
      const u64 v = sm[DENS_HDR + k];
      if (v) atomicAdd(&acc[a.off_rad + k], v);
    }
  }
}

// the checks both entry points share, then the layout
int dens_layout(const aiqmc_ctx* c, const aiqmc_density_cfg* g, int64_t off[8], int64_t* n_words, int* priv) {
  if (!c) return fail(AIQMC_EINVAL, "null context");
  if (!g) return fail(AIQMC_EINVAL, "null density configuration");
  static const char* ax = "xyz";
  bool grid = true;
  for (int d = 0; d < 3; ++d) {
    if (g->grid_n[d] < 0) return fail(AIQMC_EINVAL, std::string("negative grid_n[") + std::to_string(d) + "]");
    if (g->grid_n[d] > AIQMC_DENSITY_MAX_BINS)
      return fail(AIQMC_EINVAL, std::string("grid_n[") + std::to_string(d) + "] above AIQMC_DENSITY_MAX_BINS");
    grid = grid && g->grid_n[d] > 0;
  }
  if (g->rad_n < 0) return fail(AIQMC_EINVAL, "negative rad_n");
  if (g->pair_n < 0) return fail(AIQMC_EINVAL, "negative pair_n");
  if (g->rad_n > AIQMC_DENSITY_MAX_BINS) return fail(AIQMC_EINVAL, "rad_n above AIQMC_DENSITY_MAX_BINS");
  if (g->pair_n > AIQMC_DENSITY_MAX_BINS) return fail(AIQMC_EINVAL, "pair_n above AIQMC_DENSITY_MAX_BINS");
  if (grid)
    for (int d = 0; d < 3; ++d)
      if (!(g->grid_hi[d] > g->grid_lo[d]) || !std::isfinite(g->grid_hi[d] - g->grid_lo[d]))
        return fail(AIQMC_EINVAL, std::string("grid_hi[") + std::to_string(d) + "] <= grid_lo[" + std::to_string(d) +
                                      "] (" + ax[d] + " axis; finite bounds with hi > lo are required)");
  if (g->rad_n > 0 && (!(g->rad_max > 0.0) || !std::isfinite(g->rad_max)))
    return fail(AIQMC_EINVAL, "rad_max must be positive and finite when rad_n > 0");
  if (g->pair_n > 0 && (!(g->pair_max > 0.0) || !std::isfinite(g->pair_max)))
    return fail(AIQMC_EINVAL, "pair_max must be positive and finite when pair_n > 0");
  const int64_t ng = grid ? 2 * (int64_t)g->grid_n[0] * g->grid_n[1] * g->grid_n[2] : 0;
  const int64_t nr = 2 * (int64_t)c->A * g->rad_n, np = 3 * (int64_t)g->pair_n;
  const int64_t sizes[8] = {1, 1, ng, grid ? 2 : 0, nr, nr ? 2 * (int64_t)c->A : 0, np, np ? 3 : 0};
  int64_t o = 0;
  for (int k = 0; k < 8; ++k) {
    off[k] = o;
    o += sizes[k];
  }
  if (o > AIQMC_DENSITY_MAX_WORDS)
    return fail(AIQMC_EINVAL, "density accumulator of " + std::to_string(o) + " words is above AIQMC_DENSITY_MAX_WORDS");
  *n_words = o;
  *priv = o - off[4] <= DENS_LDS_WORDS ? 1 : 0;
  return 0;
}

}  // namespace

extern "C" {

int aiqmc_density_layout(const aiqmc_ctx* c, const aiqmc_density_cfg* cfg, int64_t* offsets8, int64_t* n_words,
                         int32_t* privatised) {
  int64_t off[8], nw = 0;
  int priv = 0;
  if (int rc = dens_layout(c, cfg, off, &nw, &priv)) return rc;
  if (!offsets8 || !n_words) return fail(AIQMC_EINVAL, "null offsets8 / n_words");
  for (int k = 0; k < 8; ++k) offsets8[k] = off[k];
  *n_words = nw;
  if (privatised) *privatised = priv;
  return AIQMC_OK;
}

int aiqmc_density_accumulate(aiqmc_ctx* c, const aiqmc_density_cfg* cfg, const void* pos, int32_t B,
                             const void* weights, int64_t* acc, void* stream) {
  int64_t off[8], nw = 0;
  int priv = 0;
  if (int rc = dens_layout(c, cfg, off, &nw, &priv)) return rc;
  if (B < 0) return fail(AIQMC_EINVAL, "negative batch");
  if (c->A > DENS_MAX_A || c->N > DENS_MAX_N)
    return fail(AIQMC_EUNSUPPORTED, "density histograms take at most 8 atoms and 16 electrons");
  if (B == 0) return AIQMC_OK;
  if (!pos) return fail(AIQMC_EINVAL, "null positions");
  if (!acc) return fail(AIQMC_EINVAL, "null accumulator");
  HIPCHK(hipSetDevice(c->device));
  DensArgs a = {};
  for (int k = 0; k < 3 * c->A; ++k) a.atoms[k] = c->atoms[k];
  const bool grid = off[3] > off[2];
  for (int d = 0; d < 3; ++d) {
    a.n[d] = grid ? cfg->grid_n[d] : 0;
    a.lo[d] = cfg->grid_lo[d];
    a.inv_h[d] = grid ? cfg->grid_n[d] / (cfg->grid_hi[d] - cfg->grid_lo[d]) : 0.0;
  }
  a.rad_n = cfg->rad_n;
  a.rad_inv = cfg->rad_n > 0 ? cfg->rad_n / cfg->rad_max : 0.0;
  a.pair_n = cfg->pair_n;
  a.pair_inv = cfg->pair_n > 0 ? cfg->pair_n / cfg->pair_max : 0.0;
  a.N = c->N;
  a.A = c->A;
  a.nup = c->nup;
  a.B = B;
  a.off_grid = off[2];
  a.off_grid_out = off[3];
  a.off_rad = off[4];
  a.off_rad_out = off[5];
  a.off_pair = off[6];
  a.off_pair_out = off[7];
  a.n_small = nw - off[4];
  // at least DENS_WPB walkers per workgroup (what a flush is shared by), at most one workgroup per CU
  int64_t nblk = ((int64_t)B + DENS_WPB - 1) / DENS_WPB;
  if (nblk > c->ncu) nblk = c->ncu > 0 ? c->ncu : 1;
  a.wpb = (int)(((int64_t)B + nblk - 1) / nblk);
  const dim3 grd = blocks(B, a.wpb);
  const size_t lds = (size_t)(DENS_HDR + (priv ? a.n_small : 0)) * sizeof(u64);
  hipStream_t s = (hipStream_t)stream;
  by_dtype(c->dtype, [&](auto t) {
    using T = decltype(t);
    if (priv)
      k_density<T, true><<<grd, dim3(256), lds, s>>>((const T*)pos, (const T*)weights, c->d_rowsrc.as<int>(), a, (u64*)acc);
    else
      k_density<T, false><<<grd, dim3(256), lds, s>>>((const T*)pos, (const T*)weights, c->d_rowsrc.as<int>(), a, (u64*)acc);
  });
  HIPCHK(hipGetLastError());
  return AIQMC_OK;
}

}  // extern "C"
