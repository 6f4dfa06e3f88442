// TEST INFRASTRUCTURE: the costed rollout kernel (csrc/rollout_cost.h, jaco_rollout_cost) under the lockstep wavefront emulator.
// Built by tests/emu_rollout_cost/Makefile into libjaco_emu_rollout_cost{,_d12,_d30}.so; used by tests/rollout_cost_binding.py.
// The one entry below is jaco_rollout_cost with the handle taken away, as emu_rollout_fb is jaco_rollout_fb: jaco_rollout_cost_bind of
// entry_args.h, the very function jaco_env.hip calls, then the kernel over the grid the library launches.  The model loader, the refusal
// text and the grid loop are the emulator driver's own (load_model, refuse, run_grid), included as they are.
#include "../emu/emu_driver.cpp"

extern "C" int emu_rollout_cost(const void* blob, long blob_size, const JacoRolloutCostOptions* opt, const JacoFrame* frame, int n, const int32_t* state_idx,
                                int nstates, const float* qpos0, const float* qvel0, const JacoRolloutPlan* plan, const JacoRolloutGoal* goal,
                                const JacoRolloutCostOut* out, int num_envs, const float* handle_qpos, const float* handle_qvel) {
  if (load_model(blob, blob_size)) return -1;
  JacoRolloutCostArgs Q;
  const std::string why = jaco_rollout_cost_bind(g_model, opt, frame, n, state_idx, nstates, qpos0, qvel0, plan, goal, out, num_envs, handle_qpos, handle_qvel, &Q);
  if (!why.empty()) return refuse(why);
  Q.F.R.model = &g_model;
  return run_grid(n, [&]() { jaco_rollout_cost_kernel(Q); });
}
