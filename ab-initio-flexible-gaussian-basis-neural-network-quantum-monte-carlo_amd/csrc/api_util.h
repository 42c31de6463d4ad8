// api_util.h -- what every translation unit of the library shares (ctx.h lists them): the error
// return, the HIP error check and the prologue of the entry points that take a context and a batch
// of positions, and the typed launch layer (by_dtype, the grid helper and the KArgs builders).
// What only the context units call of one another is declared in host_shared.h.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstring>
#include <string>

#include "aiqmc.h"
#include "ctx.h"

// aiqmc.hip: records the message for aiqmc_last_error and returns the code
int aiqmc_fail(int code, const std::string& msg);
inline int fail(int code, const std::string& m) { return aiqmc_fail(code, m); }

#define HIPCHK(x)                                                                          \
  do {                                                                                     \
    hipError_t e_ = (x);                                                                   \
    if (e_ != hipSuccess) return fail(AIQMC_EHIP, std::string(#x) + ": " + hipGetErrorString(e_)); \
  } while (0)

inline int check_call(const aiqmc_ctx* c, const void* pos, int B) {
  if (!c) return fail(AIQMC_EINVAL, "null context");
  if (!c->params_set) return fail(AIQMC_ESTATE, "aiqmc_set_params has not been called");
  if (B < 0) return fail(AIQMC_EINVAL, "negative batch");
  if (!pos && B > 0) return fail(AIQMC_EINVAL, "null positions");
  return 0;
}

// The prologue of a context entry point, in this order everywhere: (1) check_call, (2) an empty
// batch returns AIQMC_OK, (3) the context's device becomes current (before anything allocates),
// (4) `ops` is declared and looked up.  AIQMC_ENTER is all four; an entry whose own argument
// checks also hold for an empty batch puts them between AIQMC_CHECK (1) and AIQMC_BEGIN (2-4).
#define AIQMC_CHECK(c, pos, B)                          \
  do {                                                  \
    if (int rc_ = check_call(c, pos, B)) return rc_;    \
  } while (0)
#define AIQMC_BEGIN(c, B, ops)         \
  if ((B) == 0) return AIQMC_OK;       \
  HIPCHK(hipSetDevice((c)->device));   \
  ShapeOps ops;                        \
  aiqmc_shape_ops((c)->N, (c)->A, &ops)
#define AIQMC_ENTER(c, pos, B, ops) \
  AIQMC_CHECK(c, pos, B);           \
  AIQMC_BEGIN(c, B, ops)

// The one dtype dispatch of the host code: f(float{}) or f(double{}), whatever f returns.  Used as
//   by_dtype(dtype, [&](auto t) { using T = decltype(t); k<T><<<g, b, 0, s>>>((const T*)x, ...); });
// so that a launch is written once.  dtype is AIQMC_F32 or AIQMC_F64: a context's always is
// (aiqmc_create), an entry point that takes it from the caller checks first.  Where fp32 and fp64
// do something different, the code says so explicitly at that place instead.
inline bool is_dtype(int dtype) { return dtype == AIQMC_F32 || dtype == AIQMC_F64; }
template <typename F>
inline auto by_dtype(int dtype, F&& f) {
  if (dtype == AIQMC_F32) return f(float{});
  return f(double{});
}

// grid of n threads in workgroups of `per`
inline dim3 blocks(int64_t n, int per) { return dim3((unsigned)((n + per - 1) / per)); }

// ---- KArgs builders: what every launch of a kind shares; the call site adds its outputs
// the context's part of every launch (the memset relies on an all-zero-bytes KArgs being the
// value-initialised one, which tests/host/launch_abi_check.cpp checks)
inline KArgs base_args(const aiqmc_ctx* c) {
  KArgs ka;
  std::memset(&ka, 0, sizeof(ka));
  ka.nup = c->nup;
  ka.rowsrc = c->d_rowsrc.as<int>();
  ka.prm = c->d_prm.as();
  ka.quad_pivoted = c->quad_pivoted;
  return ka;
}
// n configurations at pos, one launch slot each (forward-mode, local-energy and parameter-gradient
// launches: no cache)
inline KArgs conf_args(const aiqmc_ctx* c, const void* pos, int n, void* logabs) {
  KArgs ka = base_args(c);
  ka.nconf = n;
  ka.pos = pos;
  ka.logabs = logabs;
  return ka;
}
// The context's part of the routing options (launch_route.h); mc_sweep adds `split`.
inline aq::LaunchOpts launch_opts(const aiqmc_ctx* c) {
  aq::LaunchOpts o;
  o.packed = c->packed_walkers != 0;
  o.reuse = c->reuse;
  o.ablate = c->ablate != 0;
  o.env_split = c->env_walk_split;
  o.env_quad_grad = c->env_quad_grad;
  return o;
}
// A walker launch (ops.walker) of `kind` over n configurations, with the KArgs fields the kind
// implies.  The walker kinds run the n configurations at pos; the kernel keeps its electron-local
// Jacobians (and what the proposals re-use) in the walker cache `cache`.  Proposal and Quadrature
// run n single-electron-moved configurations of the walkers at pos: with proposal reuse from the
// walker cache and the moved electrons' stage in `cache` (the caller runs ops.moved first);
// without, each takes a scratch cache of the walker layout (d_wcp) and no ecache.  The forward
// kinds take no cache.
inline WalkerCall launch_args(const aiqmc_ctx* c, aq::Launch kind, const void* pos, int n, void* logabs,
                              const DevBuf* cache = nullptr) {
  WalkerCall w{kind, launch_opts(c), conf_args(c, pos, n, logabs)};
  KArgs& ka = w.ka;
  switch (kind) {
    case aq::Launch::WalkerOrbitals: ka.value_only = 1; [[fallthrough]];
    case aq::Launch::WalkerValue:
    case aq::Launch::WalkerGrad:
    case aq::Launch::SweepWalker: ka.wcache = cache->as(); break;
    case aq::Launch::Quadrature: ka.value_only = 1; [[fallthrough]];
    case aq::Launch::Proposal:
      ka.proposal = 1;
      ka.wcache = c->reuse ? c->d_wc.as() : c->d_wcp.as();
      ka.ecache = c->reuse ? cache->as() : nullptr;
      break;
    case aq::Launch::LapForward:
    case aq::Launch::GradForward: break;
  }
  return w;
}
