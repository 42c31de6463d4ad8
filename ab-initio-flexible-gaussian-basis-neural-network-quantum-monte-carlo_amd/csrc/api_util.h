// api_util.h -- what the C-ABI translation units (aiqmc.hip, observables.hip, loss.hip,
// sr_gram.hip, shape.hip) share: the error return, the HIP error check and the prologue of the
// entry points that take a context and a batch of positions.
#pragma once
#include <hip/hip_runtime.h>

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
