// TEST INFRASTRUCTURE: the transition-Jacobian kernel (csrc/transition.h, jaco_transition_fd) under the lockstep wavefront emulator.
// Built by tests/emu_transition/Makefile into libjaco_emu_transition{,_d12,_d30}.so; used by tests/transition_binding.py.
// The one entry below is jaco_transition_fd with the handle taken away, as emu_rollout is jaco_rollout: jaco_transition_bind of
// entry_args.h, the very function jaco_env.hip calls, then the kernel over the grid the library launches (n * groups work items).  The
// model loader, the refusal text and the grid loop are the emulator driver's own (load_model, refuse, run_grid), included as they are --
// and with them every entry that driver has (emu_rollout, emu_fd, the step), on the same build.
#include "../emu/emu_driver.cpp"

extern "C" int emu_transition_fd(const void* blob, long blob_size, const JacoTransitionOptions* opt, int n, const float* qpos, const float* qvel, const float* ctrl,
                                 const JacoTransitionOut* out, int num_envs, const float* handle_qpos, const float* handle_qvel) {
  if (load_model(blob, blob_size)) return -1;
  JacoTransitionArgs Q;
  const std::string why = jaco_transition_bind(g_model, opt, n, qpos, qvel, ctrl, out, num_envs, handle_qpos, handle_qvel, &Q);
  if (!why.empty()) return refuse(why);
  Q.model = &g_model;
  return run_grid(n * Q.groups, [&]() { jaco_transition_fd_kernel(Q); });
}
