// TEST INFRASTRUCTURE: the emulator driver of tests/emu plus the entry of the joint-space controller -- the host half of jaco_joint
// (every argument check, the active dof set, the dofs to wrap, the saturation level: jaco_joint_resolve of joint.h, the very function
// jaco_env.hip calls) and the grid of jaco_joint_kernel, one wavefront per env.  The entries of ../emu/emu_driver.cpp (steps, queries,
// inverse kinematics ...) are in this library too.
#include "../emu/emu_driver.cpp"

extern "C" int emu_joint(const void* blob, long blob_size, int nenv, const JacoJointOptions* opt_in, const float* qpos, const float* qvel,
                         const float* target_qpos, const float* target_qvel, const float* qacc_ff, const float* ctrl_in, float* ctrl_out) {
  if (load_model(blob, blob_size)) return -1;
  const JacoJointOptions defaults = JACO_JOINT_DEFAULTS;
  JacoJointOpts opt;
  memcpy(&opt, opt_in ? opt_in : &defaults, sizeof(JacoJointOptions));
  JacoJointArgs Q{};
  Q.target_qpos = target_qpos; Q.target_qvel = target_qvel; Q.qacc_ff = qacc_ff; Q.ctrl_in = ctrl_in; Q.ctrl_out = ctrl_out;
  const std::string why = jaco_joint_resolve(g_model, opt, &Q);
  if (!why.empty()) return refuse("jaco_joint", why);
  Q.model = &g_model; Q.qpos = qpos; Q.qvel = qvel; Q.nenv = nenv;
  emu_grid = nenv;
  for (int e = 0; e < nenv; e++) emu_run_wave(e, [&]() { jaco_joint_kernel(Q); });
  return 0;
}
