// TEST INFRASTRUCTURE: the robot-configuration query kernel (mujoco_jaco_amd/csrc/query.h) under the lockstep wavefront emulator --
// what jaco_query / jaco_launch_query do on the GPU, one emulated wavefront per env.  Built by tests/emu/query.mk into
// libjaco_emu_query{,_d12,_d30}.so together with emu_driver.cpp, so one library both steps envs and queries them.
#include <cstdio>
#include <functional>
#include <string>
#include <vector>

// (the kernels themselves, jaco_query_kernel among them, are defined once, by emu_driver.cpp's unit: this one defines none)
#define JACO_TU (-1)
#include "../../include/jaco_env.h"
#include "../../mujoco_jaco_amd/csrc/model_blob.h"
#include "../../mujoco_jaco_amd/csrc/physics_kernel.h"

void emu_run_wave(int block, std::function<void()> body);
void jaco_query_kernel(JacoQueryArgs Q);   // (query.h, defined in emu_driver.cpp's unit)

extern "C" int emu_query_lds_bytes() { return (int)sizeof(JacoLDS<JacoArm>); }

// the host half of jaco_query (argument checks, frame table by value) and the grid of the kernel
extern "C" int emu_query(const void* blob, long blob_size, int nenv, const float* qpos, const float* qvel, const JacoFrame* frames, int nframes,
                         float* xpos, float* xmat, float* jac, float* qM, float* qfrc_bias) {
  static JacoModelDev model;
  static std::vector<float> hull;
  std::string err;
  if (jaco_model_from_blob(blob, (size_t)blob_size, &model, &hull, &err)) { fprintf(stderr, "emu: %s\n", err.c_str()); return -1; }
  if (nframes < 0 || nframes > JACO_QUERY_MAX_FRAMES) return JACO_EINVAL;
  JacoQueryArgs Q{};
  for (int f = 0; f < nframes; f++) {
    if (frames[f].body < -1 || frames[f].body >= model.nbody) return JACO_EINVAL;
    memcpy(&Q.fr[f], &frames[f], sizeof(JacoFrame));
  }
  Q.model = &model; Q.qpos = qpos; Q.qvel = qvel; Q.xpos = xpos; Q.xmat = xmat; Q.jac = jac; Q.qM = qM; Q.bias = qfrc_bias;
  Q.nenv = nenv; Q.nframes = nframes;
  for (int e = 0; e < nenv; e++) emu_run_wave(e, [&]() { jaco_query_kernel(Q); });
  return 0;
}
