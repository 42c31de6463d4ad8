// launch_abi_check.cpp -- stand-alone host check of the launch ABI: csrc/kargs.h (KArgs, AccArgs,
// the accumulator word layout), csrc/ecp_args.h (EcpArgs) and csrc/launch_route.h, the three
// headers the host and the kernels share (built and run by
// tests/test_capi_cpu.py::test_launch_abi_host_check under -fsanitize=address,undefined).
//  1. That this file compiles as plain C++ with -Werror shows the headers need nothing of HIP.
//  2. The frozen layout: sizeof and every field offset of the three structs against the table
//     below.  Its numbers were read off the structs as they stood when the kernels' headers still
//     held them, and are the ones the headers' own static_asserts carry: a layout change has to
//     edit both places.
//  3. What the host relies on: base_args (api_util.h) builds a KArgs by memset, so the
//     value-initialised structs must be all-zero bytes; and the relations between the accumulator
//     constants that the kernels' indexing assumes.
#include <cstddef>
#include <cstdio>
#include <cstring>

#include "ecp_args.h"
#include "kargs.h"
#include "launch_route.h"

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

struct Field {
  const char* name;
  size_t got, want;
};
#define F(S, f, want) {#S "." #f, offsetof(S, f), want}

static const Field fields[] = {
    {"sizeof(AccArgs)", sizeof(AccArgs), 112},
    F(AccArgs, grad, 0), F(AccArgs, lp, 8), F(AccArgs, lpn, 16), F(AccArgs, gown, 24), F(AccArgs, gauss1, 32),
    F(AccArgs, gauss2, 40), F(AccArgs, u, 48), F(AccArgs, taueff, 56), F(AccArgs, tacc, 64), F(AccArgs, tpart, 72),
    F(AccArgs, tstep, 80), F(AccArgs, count, 88), F(AccArgs, zero, 96), F(AccArgs, nzero, 104),
    {"sizeof(KArgs)", sizeof(KArgs), 368},
    F(KArgs, nconf, 0), F(KArgs, nup, 4), F(KArgs, rowsrc, 8), F(KArgs, prm, 16), F(KArgs, pos, 24),
    F(KArgs, proposal, 32), F(KArgs, pgrad, 40), F(KArgs, gauss1, 48), F(KArgs, taueff, 56), F(KArgs, tacc, 64),
    F(KArgs, tpart, 72), F(KArgs, tstep, 80), F(KArgs, seed, 88), F(KArgs, step, 96), F(KArgs, mper, 104),
    F(KArgs, mdiv, 108), F(KArgs, xnew, 112), F(KArgs, value_only, 120), F(KArgs, orb, 128), F(KArgs, ablate, 136),
    F(KArgs, phase_grad, 140), F(KArgs, dg1, 144), F(KArgs, dg2, 152), F(KArgs, du, 160), F(KArgs, acc, 168),
    F(KArgs, pvok, 280), F(KArgs, reserved0, 284), F(KArgs, reserved1, 288), F(KArgs, quad_pivoted, 292),
    F(KArgs, wcache, 296), F(KArgs, ecache, 304), F(KArgs, lapcache, 312), F(KArgs, logabs, 320), F(KArgs, phase, 328),
    F(KArgs, grad, 336), F(KArgs, el, 344), F(KArgs, sumsq, 352), F(KArgs, gown, 360),
    {"sizeof(EcpArgs)", sizeof(EcpArgs), 184},
    F(EcpArgs, B, 0), F(EcpArgs, N, 4), F(EcpArgs, A, 8), F(EcpArgs, KL, 12), F(EcpArgs, KN, 16), F(EcpArgs, L, 20),
    F(EcpArgs, tab, 24), F(EcpArgs, pos, 32), F(EcpArgs, rot, 40), F(EcpArgs, lp0, 48), F(EcpArgs, ph0, 56),
    F(EcpArgs, lpq, 64), F(EcpArgs, phq, 72), F(EcpArgs, eall, 80), F(EcpArgs, e_re, 88), F(EcpArgs, e_im, 96),
    F(EcpArgs, xnew, 104), F(EcpArgs, seed, 112), F(EcpArgs, step, 120), F(EcpArgs, skip_nl, 128),
    F(EcpArgs, cdf_lds, 132), F(EcpArgs, tstep, 136), F(EcpArgs, usel, 144), F(EcpArgs, uacc, 152), F(EcpArgs, acc, 160),
    F(EcpArgs, pos_out, 168), F(EcpArgs, scr, 176),
};

template <typename S>
static bool all_zero_bytes(const S& s) {
  unsigned char z[sizeof(S)];
  std::memset(z, 0, sizeof(S));
  return std::memcmp(&s, z, sizeof(S)) == 0;
}

int main() {
  for (const Field& f : fields) {
    std::printf("%-22s %4zu\n", f.name, f.got);
    REQ(f.got == f.want, "%s is %zu, the frozen layout has %zu", f.name, f.got, f.want);
  }
  // the table is in declaration order: within a struct (a sizeof row starts one) the offsets ascend
  for (size_t i = 1; i < sizeof(fields) / sizeof(fields[0]); ++i) {
    const bool starts = std::strncmp(fields[i].name, "sizeof", 6) == 0 || std::strncmp(fields[i - 1].name, "sizeof", 6) == 0;
    REQ(starts || fields[i].got > fields[i - 1].got, "%s does not follow %s", fields[i].name, fields[i - 1].name);
  }
  // the last field of the table ends its struct and AccArgs sits in KArgs whole.  (A field added
  // between two others is not found by this program: it shifts the later offsets or, in padding,
  // nothing, and is a change to the table's struct that review sees.)
  REQ(offsetof(AccArgs, nzero) + sizeof(int32_t) + 4 == sizeof(AccArgs), "AccArgs ends after nzero (and its padding)");
  REQ(offsetof(KArgs, gown) + sizeof(void*) == sizeof(KArgs), "KArgs ends after gown");
  REQ(offsetof(EcpArgs, scr) + sizeof(double*) == sizeof(EcpArgs), "EcpArgs ends after scr");
  REQ(offsetof(KArgs, pvok) == offsetof(KArgs, acc) + sizeof(AccArgs), "AccArgs is embedded in KArgs whole");

  const KArgs ka{};
  const AccArgs aa{};
  REQ(all_zero_bytes(ka), "a value-initialised KArgs is not all-zero bytes (base_args memsets it)");
  REQ(all_zero_bytes(aa), "a value-initialised AccArgs is not all-zero bytes");
  REQ(aa.zero == nullptr && aa.nzero == 0, "AccArgs' defaulted members");

  REQ(TACC_STRIDE == TACC_SLOTS + 64, "TACC_STRIDE %d, TACC_SLOTS %d", TACC_STRIDE, TACC_SLOTS);
  REQ(TPART_KIND == 4 * TPART, "TPART_KIND %d, TPART %d", TPART_KIND, TPART);
  REQ(TACC_BAD < TACC_STRIDE, "TACC_BAD %d, TACC_STRIDE %d", TACC_BAD, TACC_STRIDE);
  REQ(TACC_MID == TACC_SLOTS && TACC_HI == TACC_SLOTS + 1 && TACC_BAD == TACC_SLOTS + 2, "mid, hi, bad follow the lo slots");

  std::printf("launch_abi_check: %d failures\n", g_bad);
  return g_bad ? 1 : 0;
}
