// TEST INFRASTRUCTURE: the emulator driver of tests/emu_osc plus the entry of the task-axis / null-space controller -- the host half of
// jaco_osc_task (jaco_osc_task_resolve of osc_task.h, the very function jaco_env.hip calls) and the grid of jaco_osc_task_kernel, one
// wavefront per env.  A NULL task record forwards to emu_osc, as jaco_osc_task forwards to jaco_osc.
#include "../emu_osc/emu_osc_driver.cpp"

extern "C" int emu_osc_task(const void* blob, long blob_size, int nenv, const JacoFrame* frames, int nframes, const JacoOscOptions* opt_in,
                            const JacoOscTask* task_in, const float* qpos, const float* qvel, const float* target_pos, const float* target_quat,
                            const float* rest_qpos, const float* ctrl_in, float* ctrl_out, int* status) {
  if (!task_in) return emu_osc(blob, blob_size, nenv, frames, nframes, opt_in, qpos, qvel, target_pos, target_quat, ctrl_in, ctrl_out, status);
  if (load_model(blob, blob_size)) return -1;
  const JacoOscOptions defaults = JACO_OSC_DEFAULTS;
  JacoOscOpts opt;
  memcpy(&opt, opt_in ? opt_in : &defaults, sizeof(JacoOscOptions));
  JacoOscTaskOpts task;
  memcpy(&task, task_in, sizeof(JacoOscTask));
  JacoOscTaskArgs T{};
  T.o.target_pos = target_pos; T.o.target_quat = target_quat; T.o.ctrl_in = ctrl_in; T.o.ctrl_out = ctrl_out; T.o.status = status;
  T.rest_qpos = rest_qpos;
  const std::string why = jaco_osc_task_resolve(g_model, reinterpret_cast<const JacoQueryFrame*>(frames), nframes, opt, task, &T);
  if (!why.empty()) return refuse("jaco_osc_task", why);
  T.o.model = &g_model; T.o.qpos = qpos; T.o.qvel = qvel; T.o.nenv = nenv;
  emu_grid = nenv;
  for (int e = 0; e < nenv; e++) emu_run_wave(e, [&]() { jaco_osc_task_kernel(T); });
  return 0;
}
