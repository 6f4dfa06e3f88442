// TEST INFRASTRUCTURE: the cost-expansion kernel (csrc/cost_quad.h, jaco_cost_quad) under the lockstep wavefront emulator.
// Built by tests/emu_cost_quad/Makefile into libjaco_emu_cost_quad{,_d12,_d30}.so; used by tests/cost_quad_binding.py.
// The one entry below is jaco_cost_quad with the handle taken away, as emu_transition_fd is jaco_transition_fd: jaco_cost_quad_bind of
// entry_args.h, the very function jaco_env.hip calls, then the kernel over the grid the library launches (R * T work items).  The
// transition driver is included as it is -- and with it the emulator driver and every entry the two have (emu_transition_fd, emu_rollout_fb,
// emu_rollout_cost, emu_query, ...): one library per layout holds every entry an iLQR iteration needs but jaco_lqr, which reads no model.
#include "../emu_transition/emu_transition_driver.cpp"

extern "C" int emu_cost_quad(const void* blob, long blob_size, const JacoCostQuadOptions* opt, const JacoFrame* frame, int R, const float* qpos, const float* qvel,
                             const float* ctrl, const JacoCostQuadGoal* goal, const JacoCostQuadOut* out) {
  if (load_model(blob, blob_size)) return -1;
  JacoCostQuadArgs Q;
  const std::string why = jaco_cost_quad_bind(g_model, opt, frame, R, qpos, qvel, ctrl, goal, out, &Q);
  if (!why.empty()) return refuse(why);
  Q.model = &g_model;
  return run_grid(R * Q.T, [&]() { jaco_cost_quad_kernel(Q); });
}
