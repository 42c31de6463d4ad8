// shape.hip -- kernels and host helpers for ONE (N, A) shape.  Compiled once
// per entry of AIQMC_SHAPE_LIST with -DAQ_N=<N> -DAQ_A=<A> (parallel build).
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstring>

#include "api_util.h"
// the wavefront kernels; walker_fwd.h first keeps the order their definitions have had in the code object
#include "walker_fwd.h"
#include "limdrift.h"
#include "walker_lap.h"
#include "quad_small.h"
#include "walker_pgrad.h"

using namespace aq;

#ifndef AQ_N
#error "compile with -DAQ_N=<electrons> -DAQ_A=<atoms>"
#endif

// One thread per (walker b, electron i): the acceptance of walkers_update (VMCmcstep.py:80-106)
// for the last sweep of aiqmc_mc_step (earlier sweeps fuse it into the next walker launch) and
// for the DMC drift-diffusion step.
template <typename T, int N>
__global__ __launch_bounds__(256) void k_accept(T* __restrict__ pos, AccArgs a, int B) {
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  // limdrift factors: every lane of the (full, 256-thread) block's waves before any returns
  const T te1 = taueff_wave<T>(a.taueff, a.tacc, 0, a.tstep, a.tpart), te2 = taueff_wave<T>(a.taueff, a.tacc, 1, a.tstep, a.tpart);
  // the next mc_step call's accumulator bank (not read by this call)
  for (int k = t; k < a.nzero; k += gridDim.x * blockDim.x) a.zero[k] = 0ull;
  if (t >= B * N) return;
  const int b = t / N, i = t - b * N;
  T xn[3];
  if (accept_one<T, N>(a, pos, b, i, xn, te1, te2)) {
#pragma unroll
    for (int c = 0; c < 3; ++c) pos[(size_t)b * 3 * N + 3 * i + c] = xn[c];
    if (a.count) atomicAdd(&a.count[b], 1);
  }
}

// the canonical <-> kernel-layout parameter map of this shape (param_map.h) from the context's tables
template <int N, int A>
static void param_map_impl(const aiqmc_ctx* c, ParamMap& m) {
  build_param_map<N, A>(c->npar, c->nanti, c->par.data(), c->anti.data(), c->atoms.data(), c->charges.data(), m);
}

// hipFuncSetAttribute for a launch that takes more dynamic LDS than the default 64 KB limit
static int raise_lds(const void* fn, int bytes) {
  if (bytes <= 65536) return 0;
  hipError_t e = hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, bytes);
  if (e != hipSuccess) return fail(AIQMC_EHIP, std::string("hipFuncSetAttribute: ") + hipGetErrorString(e));
  return 0;
}

template <typename T, int N, int A>
static int set_lds_t() {
  if (int rc = raise_lds((const void*)&k_walker<T, N, A, MODE_GRAD>, Smem<T, N, false>::bytes)) return rc;
  if (int rc = raise_lds((const void*)&k_walker<T, N, A, MODE_LAP>, Smem<T, N, true>::bytes)) return rc;
  if (int rc = raise_lds((const void*)&k_walker_rev<T, N, A>, SmemRev<T, N, A>::bytes)) return rc;
  // proposal launches: RevWpb configurations per workgroup.  fp32 only: an fp64 proposal workgroup
  // holds one configuration, within the default limit for every shape
  constexpr int pb = RevWpb<T, true>::value * SmemRev<T, N, A, true>::bytes;
  if constexpr (sizeof(T) == 4) return raise_lds((const void*)&k_walker_rev<T, N, A, false, true>, pb);
  else static_assert(pb <= 65536, "fp64 proposal launches need the raised LDS limit too");
  return 0;
}
template <int N, int A>
static int set_lds_impl() {   // both dtypes: the attribute belongs to the kernel, not to a context
  if (int rc = set_lds_t<float, N, A>()) return rc;
  return set_lds_t<double, N, A>();
}

// proposal-launch grid: ceil(nconf / wpb) workgroups, padded to a multiple of the 8 XCDs so that
// xcd_major keeps each walker's proposals on one XCD (the padding workgroups exit at once)
static inline unsigned prop_blocks(int nconf, int wpb) {
  const unsigned nb = (unsigned)((nconf + wpb - 1) / wpb);
  return wpb > 1 ? (nb + 7u) & ~7u : nb;
}

// The kernel of a walker launch (ops.walker): one case per row of route(kind, options)
// (launch_route.h has the table of which kind and options reach which row).  T = the dtype;
// n = nconf; Wp = RevWpb<T, true>, Ww = RevWpb<T, false> configurations per workgroup (both 1 for
// fp64); NSL = QSlot<N>::NSL configurations per wave (4 for N <= 4, 2 for N <= 8: quad_small.h, from
// the walker cache); LDS = dynamic LDS bytes.
//
//  #  row         kernel                      grid                block  LDS
//  1  QuadValue   k_quad_value<T>             prop_blocks(n,NSL)  64     0
//  2  QuadGrad    k_quad_grad<T>              ceil(n / NSL)       64     0
//  3  QuadWalker  k_quad_grad<T, walker>      ceil(n / NSL)       64     0
//  4  LapFwd      k_walker<T, MODE_LAP>       n                   64     Smem<T, N, true>
//  5  RevProp     k_walker_rev<T, PROP>       prop_blocks(n, Wp)  64 Wp  Wp SmemRev<T, true>
//  6  RevSplit    k_walker_rev<float, SPL>    n                   128    SmemRev<float>
//  7  Rev         k_walker_rev<T>             ceil(n / Ww)        64 Ww  Ww SmemRev<T>
//  8  GradFwd     k_walker<T, MODE_GRAD>      n                   64     Smem<T, N, false>
//
// Rows 1-3 are instantiated for N <= 8 alone and row 6 for float alone (route returns them for
// nothing else); every other row for every shape and both dtypes.
template <typename T, int N, int A>
static void walker_launch(const WalkerCall& w, int nconf, hipStream_t s) {
  const KArgs& ka = w.ka;
  switch (route(w.kind, sizeof(T) == 4, N, w.opts)) {
    case Row::QuadValue:
      if constexpr (N <= 8) k_quad_value<T, N, A><<<dim3(prop_blocks(nconf, QSlot<N>::NSL)), dim3(64), 0, s>>>(ka);
      break;
    case Row::QuadGrad:
      if constexpr (N <= 8) k_quad_grad<T, N, A><<<dim3((nconf + QSlot<N>::NSL - 1) / QSlot<N>::NSL), dim3(64), 0, s>>>(ka);
      break;
    case Row::QuadWalker:
      if constexpr (N <= 8)
        k_quad_grad<T, N, A, true><<<dim3((nconf + QSlot<N>::NSL - 1) / QSlot<N>::NSL), dim3(64), 0, s>>>(ka);
      break;
    case Row::LapFwd:
      k_walker<T, N, A, MODE_LAP><<<dim3(nconf), dim3(64), Smem<T, N, true>::bytes, s>>>(ka);
      break;
    case Row::RevProp: {   // proposals from the walker cache
      constexpr int W = RevWpb<T, true>::value;
      k_walker_rev<T, N, A, false, true><<<dim3(prop_blocks(nconf, W)), dim3(64 * W),
                                          W * SmemRev<T, N, A, true>::bytes, s>>>(ka);
      break;
    }
    case Row::RevSplit:   // two waves per walker: an fp32 instantiation only
      if constexpr (sizeof(T) == 4)
        k_walker_rev<T, N, A, false, false, false, true><<<dim3(nconf), dim3(128), SmemRev<T, N, A>::bytes, s>>>(ka);
      break;
    case Row::Rev: {
      constexpr int W = RevWpb<T, false>::value;
      static_assert(sizeof(T) == 4 || W == 1, "fp64 walker launches: one walker per workgroup, grid = nconf");
      k_walker_rev<T, N, A><<<dim3((nconf + W - 1) / W), dim3(64 * W), W * SmemRev<T, N, A>::bytes, s>>>(ka);
      break;
    }
    case Row::GradFwd:
      k_walker<T, N, A, MODE_GRAD><<<dim3(nconf), dim3(64), Smem<T, N, false>::bytes, s>>>(ka);
      break;
  }
}
template <int N, int A>
static void walker_impl(int dtype, const WalkerCall& w, int nconf, hipStream_t s) {
  by_dtype(dtype, [&](auto t) { walker_launch<decltype(t), N, A>(w, nconf, s); });
}

// Local energy: adjoint pass (k_walker_rev<PREP>) then first-derivative pass (k_walker_lap).
// phase: the same pair for theta = arg psi (the PH instantiations, complex_output=True)
template <typename T, int N, int A, bool PH>
static void lap_launch(const KArgs& k1, const KArgs& k2, int nconf, int waves, hipStream_t s) {
  const dim3 wg(64 * waves);   // waves per walker in the first-derivative pass: 1, 2 or 4
  k_walker_rev<T, N, A, true, false, PH><<<dim3(nconf), dim3(64), SmemRev<T, N, A>::bytes, s>>>(k1);
  if (waves == 1)
    k_walker_lap<T, N, A, 1, PH><<<dim3(nconf), wg, SmemLap<T, N, A>::bytes, s>>>(k2);
  else
    k_walker_lap<T, N, A, 4, PH><<<dim3(nconf), wg, SmemLap<T, N, A>::bytes, s>>>(k2);
}
template <int N, int A>
static void lap_impl(int dtype, const KArgs& k1, const KArgs& k2, int nconf, int waves, int phase, hipStream_t s) {
  by_dtype(dtype, [&](auto t) {
    using T = decltype(t);
    if (phase) lap_launch<T, N, A, true>(k1, k2, nconf, waves, s);
    else lap_launch<T, N, A, false>(k1, k2, nconf, waves, s);
  });
}

template <int N, int A>
static void moved_impl(int dtype, const KArgs& ka, hipStream_t s) {
  by_dtype(dtype, [&](auto t) {
    using T = decltype(t);
    if (ka.value_only && ka.xnew) {   // pp quadrature: values only, one configuration per lane
      const int nv = (ka.nconf + 63) / 64;
      k_moved_value<T, N, A><<<dim3(prop_blocks(nv, MOVED_WPB)), dim3(64 * MOVED_WPB), 0, s>>>(ka);
    } else {
      const int nb = (ka.nconf + 15) / 16;
      k_moved_electron<T, N, A><<<dim3(prop_blocks(nb, MOVED_WPB)), dim3(64 * MOVED_WPB), 0, s>>>(ka);
    }
  });
}

template <int N, int A>
static void accept_impl(int dtype, void* pos, const AccArgs& a, int B, hipStream_t s) {
  by_dtype(dtype, [&](auto t) {
    using T = decltype(t);
    k_accept<T, N><<<blocks(B * N, 256), dim3(256), 0, s>>>((T*)pos, a, B);
  });
}

// per-walker parameter gradients in the kernel layout: out [nconf][Lay::total]
template <int N, int A>
static int pgrad_impl(int dtype, const KArgs& ka, int nconf, hipStream_t s) {
  return by_dtype(dtype, [&](auto t) {
    using T = decltype(t);
    constexpr int K = PgK<N>::value;   // walkers per wave (walker_pgrad.h)
    constexpr int bytes = K * SmemPG<T, N, A>::bytes;
    if (int rc = raise_lds((const void*)&k_param_grad<T, N, A, K>, bytes)) return rc;
    k_param_grad<T, N, A, K><<<dim3((nconf + K - 1) / K), dim3(64), bytes, s>>>(ka);
    return 0;
  });
}

// dynamic LDS bytes and waves per workgroup of the launches that take dynamic LDS, by AIQMC_LDS_* kind
template <typename T, int N, int A>
static void launch_table(int* lds, int* waves) {
  constexpr int WP = RevWpb<T, true>::value, WW = RevWpb<T, false>::value;
  const int b[6] = {WP * SmemRev<T, N, A, true>::bytes, WW * SmemRev<T, N, A>::bytes, SmemRev<T, N, A>::bytes,
                    SmemLap<T, N, A>::bytes, PgK<N>::value * SmemPG<T, N, A>::bytes, Smem<T, N, true>::bytes};
  const int w[6] = {WP, WW, 1, 0, 1, 1};   // 0: the launch chooses (k_walker_lap: 1, 2 or 4 waves)
  for (int k = 0; k < 6; ++k) {
    lds[k] = b[k];
    waves[k] = w[k];
  }
}

static void phase_read_impl(unsigned long long* out) {
#ifdef AQ_PHASE_PROF
  (void)hipMemcpyFromSymbol(out, HIP_SYMBOL(aq_phase_cycles), 32 * sizeof(unsigned long long));
  unsigned long long z[32] = {};
  (void)hipMemcpyToSymbol(HIP_SYMBOL(aq_phase_cycles), z, sizeof(z));
#else
  for (int k = 0; k < 32; ++k) out[k] = 0;
#endif
}

#define AQ_CAT2(a, b, c) aiqmc_shape_ops_##a##_##b##c
#define AQ_CAT(a, b) AQ_CAT2(a, b, )
bool AQ_CAT(AQ_N, AQ_A)(ShapeOps* ops) {
  ops->set_lds = &set_lds_impl<AQ_N, AQ_A>;
  ops->walker = &walker_impl<AQ_N, AQ_A>;
  ops->accept = &accept_impl<AQ_N, AQ_A>;
  ops->moved = &moved_impl<AQ_N, AQ_A>;
  ops->lap = &lap_impl<AQ_N, AQ_A>;
  ops->lcache_n = LapCache<AQ_N, AQ_A>::size;
  ops->phase_read = &phase_read_impl;
  ops->wcache_n = WCache<AQ_N, AQ_A>::size;
  ops->ecache_n = ECache<AQ_N, AQ_A>::size;
  ops->param_map = &param_map_impl<AQ_N, AQ_A>;
  ops->pgrad = &pgrad_impl<AQ_N, AQ_A>;
  launch_table<float, AQ_N, AQ_A>(ops->dyn_lds[0], ops->wg_waves[0]);
  launch_table<double, AQ_N, AQ_A>(ops->dyn_lds[1], ops->wg_waves[1]);
  return true;
}
