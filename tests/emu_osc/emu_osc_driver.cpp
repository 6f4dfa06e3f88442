// TEST INFRASTRUCTURE: the emulator driver of tests/emu plus the entry of the operational-space controller -- the host half of jaco_osc
// (every argument check, active dof sets, saturation levels: jaco_osc_resolve of osc.h, the very function jaco_env.hip calls) and the
// grid of jaco_osc_kernel, one wavefront per env.  The entries of ../emu/emu_driver.cpp (steps, queries, ...) are in this library too.
#include "../emu/emu_driver.cpp"

extern "C" int emu_osc(const void* blob, long blob_size, int nenv, const JacoFrame* frames, int nframes, const JacoOscOptions* opt_in,
                       const float* qpos, const float* qvel, const float* target_pos, const float* target_quat, const float* ctrl_in,
                       float* ctrl_out, int* status) {
  if (load_model(blob, blob_size)) return -1;
  const JacoOscOptions defaults = JACO_OSC_DEFAULTS;
  JacoOscOpts opt;
  memcpy(&opt, opt_in ? opt_in : &defaults, sizeof(JacoOscOptions));
  JacoOscArgs Q{};
  Q.target_pos = target_pos; Q.target_quat = target_quat; Q.ctrl_in = ctrl_in; Q.ctrl_out = ctrl_out; Q.status = status;
  const std::string why = jaco_osc_resolve(g_model, reinterpret_cast<const JacoQueryFrame*>(frames), nframes, opt, &Q);
  if (!why.empty()) return refuse("jaco_osc", why);
  Q.model = &g_model; Q.qpos = qpos; Q.qvel = qvel; Q.nenv = nenv;
  emu_grid = nenv;
  for (int e = 0; e < nenv; e++) emu_run_wave(e, [&]() { jaco_osc_kernel(Q); });
  return 0;
}
