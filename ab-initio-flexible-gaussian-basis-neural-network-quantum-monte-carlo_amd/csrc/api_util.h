// api_util.h -- what every translation unit of the library shares (the context units aiqmc.hip,
// dmc.hip, debug.hip, observables.hip, components.hip, density.hip and corrsamples.hip, the
// context-free loss.hip, sr_gram.hip and blocking.hip, and shape.hip): the error return, the HIP
// error check and the prologue of the entry points that take a context and a batch of positions,
// and the typed launch layer (by_dtype, the grid helper and the KArgs builders).  What only the
// context units call of one another is declared in host_shared.h.
#pragma once
#include <hip/hip_runtime.h>

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

// ---- KArgs builders: what every launch of a kind shares; the call site adds its outputs and flags
// the context's part of every launch
inline KArgs base_args(const aiqmc_ctx* c) {
  KArgs ka;
  std::memset(&ka, 0, sizeof(ka));
  ka.nup = c->nup;
  ka.rowsrc = c->d_rowsrc.as<int>();
  ka.prm = c->d_prm.as();
  ka.one_wave = c->packed_walkers ? 0 : 1;
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
// walker launch over B configurations at pos; the kernel keeps its electron-local Jacobians (and
// what the proposals re-use) in the walker cache wc
inline KArgs walker_args(const aiqmc_ctx* c, const void* pos, int B, void* logabs, const DevBuf& wc) {
  KArgs ka = conf_args(c, pos, B, logabs);
  ka.wcache = wc.as();
  return ka;
}
// proposal launch: n single-electron-moved configurations of the walkers at pos.  With proposal
// reuse they come from the walker cache and the moved electrons' stage in ec (the caller runs
// ops.moved first); without, each takes a scratch cache of the walker layout (d_wcp) and no ecache.
inline KArgs proposal_args(const aiqmc_ctx* c, const void* pos, int n, void* logabs, const DevBuf& ec) {
  KArgs kp = conf_args(c, pos, n, logabs);
  kp.proposal = 1;
  kp.wcache = c->reuse ? c->d_wc.as() : c->d_wcp.as();
  kp.ecache = c->reuse ? ec.as() : nullptr;
  return kp;
}
