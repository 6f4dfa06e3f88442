// TEST INFRASTRUCTURE: the emulator driver of tests/emu plus the entry of the rollout kernel -- the host half of jaco_rollout (every
// argument check, the options and the frame by value: jaco_rollout_resolve of rollout.h, the very function jaco_env.hip calls) and the
// grid of jaco_rollout_kernel, one wavefront per rollout.  The handle's fp32 state, which the library falls back to when no state
// override is given, is handed in as handle_qpos / handle_qvel [num_envs][..].  The entries of ../emu/emu_driver.cpp (steps, queries ...)
// are in this library too, and emu_step_lo: the contact-free step with the low words a handle keeps.
#include "../emu/emu_driver.cpp"

extern "C" int emu_rollout(const void* blob, long blob_size, const JacoRolloutOptions* opt, const JacoFrame* frame, int n, const int32_t* state_idx, int nstates,
                           const float* qpos0, const float* qvel0, const float* ctrl, const JacoRolloutOut* out, int num_envs, const float* handle_qpos,
                           const float* handle_qvel) {
  if (load_model(blob, blob_size)) return -1;
  JacoRolloutArgs Q{};
  Q.state_idx = state_idx; Q.qpos0 = qpos0; Q.qvel0 = qvel0; Q.ctrl = ctrl;
  if (out) { Q.qpos = out->qpos; Q.qvel = out->qvel; Q.xpos = out->xpos; Q.xmat = out->xmat; Q.status = out->status; }
  const std::string why = jaco_rollout_resolve(g_model, reinterpret_cast<const JacoRolloutOpts*>(opt), reinterpret_cast<const JacoQueryFrame*>(frame), n, nstates,
                                               num_envs, out != nullptr, &Q);
  if (!why.empty()) return refuse("jaco_rollout", why);
  if (n == 0) return 0;
  Q.model = &g_model;
  if (!Q.qpos0) { Q.qpos0 = handle_qpos; Q.qvel0 = handle_qvel; }
  emu_grid = n;
  for (int e = 0; e < n; e++) emu_run_wave(e, [&]() { jaco_rollout_kernel(Q); });
  return 0;
}

// A contact-free ctrl-level step as a handle runs it (jaco_physics_step under option "disable_contact"): like emu_physics_step of
// ../emu/emu_driver.cpp, with the compensated low words the library keeps between calls (qpos_lo / qvel_lo, zeroed by jaco_set_state).
extern "C" int emu_step_lo(const void* blob, long blob_size, int nenv, int nsub, float* qpos, float* qvel, float* qacc_ws, float* qpos_lo, float* qvel_lo,
                           const float* ctrl, unsigned* flags) {
  if (load_model(blob, blob_size)) return -1;
  JacoStepArgs A{};
  A.model = &g_model; A.hull = g_hull.data(); A.qpos = qpos; A.qvel = qvel; A.qacc_ws = qacc_ws; A.qpos_lo = qpos_lo; A.qvel_lo = qvel_lo; A.ctrl = ctrl;
  A.flags = flags; A.nenv = nenv; A.nsub = nsub; A.disable_contact = 1; A.dbg_env = -1;
  return emu_launch(A, nullptr);
}
