// TEST INFRASTRUCTURE: the emulator driver of tests/emu plus the entry of the forward-dynamics kernel -- the host half of jaco_fd (every
// argument check, the resolved dof mask, the steps: jaco_fd_resolve of fd.h, the very function jaco_env.hip calls) and the grid of
// jaco_fd_kernel, one wavefront per env.  The entries of ../emu/emu_driver.cpp (steps, queries, inverse kinematics ...) are in this
// library too.
#include "../emu/emu_driver.cpp"

extern "C" int emu_fd(const void* blob, long blob_size, int nenv, const JacoFdOptions* opt_in, const float* qpos, const float* qvel, const float* ctrl,
                      const JacoFdOut* out) {
  if (load_model(blob, blob_size)) return -1;
  const JacoFdOptions defaults = JACO_FD_DEFAULTS;
  JacoFdOpts opt;
  memcpy(&opt, opt_in ? opt_in : &defaults, sizeof(JacoFdOptions));
  JacoFdArgs Q{};
  if (out) { Q.qacc = out->qacc; Q.qfrc_smooth = out->qfrc_smooth; Q.dqacc_dqpos = out->dqacc_dqpos; Q.dqacc_dqvel = out->dqacc_dqvel; Q.dqacc_dctrl = out->dqacc_dctrl; }
  const std::string why = jaco_fd_resolve(g_model, opt, out != nullptr, &Q);
  if (!why.empty()) return refuse("jaco_fd", why);
  Q.model = &g_model; Q.qpos = qpos; Q.qvel = qvel; Q.ctrl = ctrl; Q.nenv = nenv;
  emu_grid = nenv;
  for (int e = 0; e < nenv; e++) emu_run_wave(e, [&]() { jaco_fd_kernel(Q); });
  return 0;
}
