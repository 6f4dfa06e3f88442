// TEST INFRASTRUCTURE: the emulator driver of tests/emu_rollout (steps, queries, emu_rollout, emu_step_lo ...) plus the entry of the
// closed-loop rollout kernel -- the host half of jaco_rollout_fb (every argument check, the options, the dof list, the plan and the frame
// by value: jaco_rollout_fb_resolve of rollout_fb.h, the very function jaco_env.hip calls) and the grid of jaco_rollout_fb_kernel, one
// wavefront per rollout.  The handle's fp32 state, which the library falls back to when no state override is given, is handed in as
// handle_qpos / handle_qvel [num_envs][..].
#include "../emu_rollout/emu_rollout_driver.cpp"

extern "C" int emu_rollout_fb(const void* blob, long blob_size, const JacoRolloutFbOptions* opt, const JacoFrame* frame, int n, const int32_t* state_idx, int nstates,
                              const float* qpos0, const float* qvel0, const JacoRolloutPlan* plan, const JacoRolloutFbOut* out, int num_envs,
                              const float* handle_qpos, const float* handle_qvel) {
  if (load_model(blob, blob_size)) return -1;
  JacoRolloutFbArgs Q{};
  Q.R.state_idx = state_idx; Q.R.qpos0 = qpos0; Q.R.qvel0 = qvel0;
  if (out) { Q.R.qpos = out->qpos; Q.R.qvel = out->qvel; Q.R.xpos = out->xpos; Q.R.xmat = out->xmat; Q.R.status = out->status; Q.ctrl_out = out->ctrl; }
  const std::string why = jaco_rollout_fb_resolve(g_model, reinterpret_cast<const JacoRolloutFbOpts*>(opt), reinterpret_cast<const JacoQueryFrame*>(frame), n, nstates,
                                                  num_envs, reinterpret_cast<const JacoRolloutFbPlan*>(plan), out != nullptr, &Q);
  if (!why.empty()) return refuse("jaco_rollout_fb", why);
  if (n == 0) return 0;
  Q.R.model = &g_model;
  if (!Q.R.qpos0) { Q.R.qpos0 = handle_qpos; Q.R.qvel0 = handle_qvel; }
  emu_grid = n;
  for (int e = 0; e < n; e++) emu_run_wave(e, [&]() { jaco_rollout_fb_kernel(Q); });
  return 0;
}
