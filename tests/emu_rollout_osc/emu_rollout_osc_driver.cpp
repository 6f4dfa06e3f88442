// TEST INFRASTRUCTURE: the operational-space rollout kernel (csrc/rollout_osc.h, jaco_rollout_osc) under the lockstep wavefront emulator.
// Built by tests/emu_rollout_osc/Makefile into libjaco_emu_rollout_osc{,_d12,_d30}.so; used by tests/rollout_osc_binding.py.
// The one entry below is jaco_rollout_osc with the handle taken away, as emu_rollout_fb is jaco_rollout_fb: jaco_rollout_osc_bind of
// entry_args.h, the very function jaco_env.hip calls, then the kernel over the grid the library launches.  The model loader, the refusal
// text and the grid loop are the emulator driver's own (load_model, refuse, run_grid), included as they are -- and with them every entry
// that driver has (emu_osc, emu_rollout, the step), on the same build.
#include "../emu/emu_driver.cpp"

extern "C" int emu_rollout_osc(const void* blob, long blob_size, const JacoRolloutOscOptions* opt, const JacoFrame* frames, int nframes, const JacoFrame* out_frame, int n,
                               const int32_t* state_idx, int nstates, const float* qpos0, const float* qvel0, const JacoRolloutOscPlan* plan,
                               const JacoRolloutFbOut* out, int num_envs, const float* handle_qpos, const float* handle_qvel) {
  if (load_model(blob, blob_size)) return -1;
  JacoRolloutOscArgs Q;
  const std::string why = jaco_rollout_osc_bind(g_model, opt, frames, nframes, out_frame, n, state_idx, nstates, qpos0, qvel0, plan, out, num_envs, handle_qpos,
                                                handle_qvel, &Q);
  if (!why.empty()) return refuse(why);
  Q.R.model = &g_model;
  return run_grid(n, [&]() { jaco_rollout_osc_kernel(Q); });
}
