// TEST INFRASTRUCTURE: the emulator driver of tests/emu plus the inverse-kinematics entry -- the host half of jaco_ik (argument checks,
// active dof set: jaco_ik_resolve of ik.h, the very function jaco_env.hip calls) and the grid of jaco_ik_kernel, one wavefront per env.
#include "../emu/emu_driver.cpp"

static_assert(sizeof(JacoIkOptions) == sizeof(JacoIkOpts) && offsetof(JacoIkOptions, dof_mask) == offsetof(JacoIkOpts, dof_mask) &&
                  offsetof(JacoIkOptions, max_iters) == offsetof(JacoIkOpts, max_iters) && JACO_IK_MAX_ITERS == JIK_MAX_ITERS,
              "JacoIkOptions (include/jaco_env.h) and JacoIkOpts (ik.h) disagree");

static std::string g_ik_error;
extern "C" const char* emu_ik_last_error() { return g_ik_error.c_str(); }
extern "C" int emu_ik_lds_bytes() { return (int)sizeof(JacoLDS<JacoArm>); }
extern "C" int emu_ik(const void* blob, long blob_size, int nenv, const JacoFrame* frame, const JacoIkOptions* opt, const float* qpos_seed,
                      const float* target_pos, const float* target_quat, float* qpos_out, float* resid, int* status) {
  if (load_model(blob, blob_size)) return -1;
  if (!frame || !qpos_seed || !target_pos || !qpos_out) { g_ik_error = "jaco_ik: the frame, the target positions and the output qpos are required"; return JACO_EINVAL; }
  const JacoIkOptions defaults = JACO_IK_DEFAULTS;
  JacoIkArgs Q{};
  memcpy(&Q.fr, frame, sizeof(JacoFrame));
  memcpy(&Q.opt, opt ? opt : &defaults, sizeof(JacoIkOptions));
  if (const char* why = jaco_ik_resolve(g_model, Q.fr, Q.opt, &Q.active)) { g_ik_error = std::string("jaco_ik: ") + why; return JACO_EINVAL; }
  Q.model = &g_model; Q.qpos = qpos_seed; Q.target_pos = target_pos; Q.target_quat = target_quat;
  Q.qpos_out = qpos_out; Q.resid = resid; Q.status = status; Q.nenv = nenv;
  emu_grid = nenv;
  for (int e = 0; e < nenv; e++) emu_run_wave(e, [&]() { jaco_ik_kernel(Q); });
  return 0;
}
