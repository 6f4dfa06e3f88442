// TEST INFRASTRUCTURE: the backward-pass kernel (mujoco_jaco_amd/csrc/lqr.h) on the lockstep wavefront emulator.  lqr.h reads no model,
// so this build sees the public header, lqr.h and the library's own argument check (jaco_lqr_bind of entry_args.h) and nothing of the
// layouts: one library serves every build.
#include <functional>
#include <string>

#include "../../include/jaco_env.h"
#include "../../mujoco_jaco_amd/csrc/lqr.h"
#define JACO_ENTRY_ARGS_LQR_ONLY
#include "../../mujoco_jaco_amd/csrc/entry_args.h"

void emu_run_wave(int block, std::function<void()> body);
long emu_counter[16];

static_assert(sizeof(JacoLqrOptions) == sizeof(JacoLqrOpts) && sizeof(JacoLqrProblem) == sizeof(JacoLqrProb) && sizeof(JacoLqrOut) == sizeof(JacoLqrOutp),
              "the public records and lqr.h's (field by field: abi_agreement.h in the library's build)");

static std::string g_error;
extern "C" const char* emu_last_error() { return g_error.c_str(); }
extern "C" int emu_lqr_lds_bytes() { return (int)sizeof(JacoLqrLDS); }

// jaco_lqr without the handle and the stream: host pointers in the records
extern "C" int emu_lqr(const JacoLqrOptions* opt, int n, const JacoLqrProblem* prob, const JacoLqrOut* out) {
  JacoLqrArgs Q;
  g_error = jaco_lqr_bind(opt, n, prob, out, &Q);
  if (!g_error.empty()) return JACO_EINVAL;
  for (int i = 0; i < n; i++) emu_run_wave(i, [&]() { jaco_lqr_kernel(Q); });
  return JACO_OK;
}
