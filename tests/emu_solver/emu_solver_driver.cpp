// TEST INFRASTRUCTURE: the dense solver blocks of the kernel sources, each called on one wave of the lockstep wavefront emulator with the
// registers the caller hands in: lane l holds row l of the matrix, its right-hand side and its damping word; what every lane holds
// afterwards comes back.  Nothing here knows a model: the routines are called as the Newton stage and the controller call them.
#include <functional>

#include <jaco/model_dev.h>
#include <jaco/wave_ops.h>
#include "../../mujoco_jaco_amd/csrc/solver_blocks.h"   // (nothing else of the kernel sources: the header stands alone)

void emu_run_wave(int block, std::function<void()> body);
long emu_counter[16];

// JNV, JB0, JB1, the dual block's shared pivots, and which forms this library holds
extern "C" void emu_solver_dims(int* d) { d[0] = JNV; d[1] = JB0; d[2] = JB1; d[3] = JLDL_NSH; d[4] = JACO_SOLVER_MASKS; }

// which: 0 ldl_block<0, JB0>, 1 ldl_block<JB0, JB1>, 2 ldl_block<JB1, JNV>, 3 ldl_block<JB0, JNV>, 4 ldl_block0_dual, 5 ldl_solve<true>,
// 6 ldl_solve<false>.  H [64][JNV], b [64], hd [64] in; x [64], xd [64] (the dual's damped solution, else 0) and the rows [64][JNV] out.
extern "C" int emu_ldl(int which, const float* H, const float* b, const float* hd, float* x, float* xd, float* Hout) {
  if (which < 0 || which > 6) return -1;
  emu_run_wave(0, [&]() {
    const int lane = lane_id();
    float h[JNV], r = 0.f, rd = 0.f;
    for (int j = 0; j < JNV; j++) h[j] = H[lane * JNV + j];
    switch (which) {
      case 0: r = ldl_block<0, JB0>(h, b[lane], lane); break;
      case 1: r = ldl_block<JB0, JB1>(h, b[lane], lane); break;
      case 2: r = ldl_block<JB1, JNV>(h, b[lane], lane); break;
      case 3: r = ldl_block<JB0, JNV>(h, b[lane], lane); break;
      case 4: r = ldl_block0_dual(h, b[lane], hd[lane], lane, &rd); break;
      case 5: r = ldl_solve<true>(h, b[lane], lane); break;
      default: r = ldl_solve<false>(h, b[lane], lane); break;
    }
    x[lane] = r;
    xd[lane] = rd;
    for (int j = 0; j < JNV; j++) Hout[lane * JNV + j] = h[j];
  });
  return 0;
}

// which: 0 gj_inverse6 (A [64][6], B [64][6] in and out), 1 gj_solve6 (A, and B[lane][0] as the right-hand side, in and out).  det [64].
extern "C" int emu_gj(int which, float* A, float* B, float* det) {
  if (which < 0 || which > 1) return -1;
  emu_run_wave(0, [&]() {
    const int lane = lane_id();
    float a[6], bb[6];
    for (int j = 0; j < 6; j++) { a[j] = A[lane * 6 + j]; bb[j] = B[lane * 6 + j]; }
    det[lane] = which == 0 ? gj_inverse6(a, bb, lane) : gj_solve6(a, bb[0], lane);
    for (int j = 0; j < 6; j++) { A[lane * 6 + j] = a[j]; B[lane * 6 + j] = bb[j]; }
  });
  return 0;
}
