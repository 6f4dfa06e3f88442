// What the query-style entries (query.h .. rollout_fb.h) share: the frame record and its pose, the state load, the forward pass made of
// the step kernel's own stages, row `lane` of the mass matrix, a wave OR, and the kernel / launcher definition.
// WHO CALLS THE FUNCTIONS BELOW: run_osc_task, run_joint, run_fd (fd_pass), run_rollout (both rollout kernels), run_transition
// (entry_walk, wave_or and the entry macro; its restore of a pair is written out in transition.h) and run_cost_quad (entry_state, entry_walk,
// frame_pose, wave_or).  Among those, "the same
// prologue", "the same forward pass", "run_rollout's loop" hold by construction.
// WHO DOES NOT: run_query, run_ik and run_osc keep prologue, forward pass and pose written out in their own headers, because built on
// these functions their kernels measured slower on the MI355X.  For them entry_state, entry_forward and body_frame_pose are
// hand-kept twins: identity with those three entries rests on the bit-for-bit tests, as before, and a change to one side has to be
// made on the other.
// The promise of identity with the step kernel holds because everything here calls run_env's stages as they are.
// Included from the tail of physics_kernel.h, in front of the entry headers.
#pragma once

struct JacoQueryFrame {   // = JacoFrame of include/jaco_env.h (static_assert in abi_agreement.h)
  int body;               // fused body index, -1: world-fixed
  float pos[3], mat[9];   // frame pose in that body's frame (row-major rotation)
  float point[3];         // Jacobian reference point, in the frame's coordinates
};

// The pose of frame F on a body (F.body >= 0) at the body poses in s.xpos / s.xmat, composed as ee_frame composes the EE (xpos_b + R_b p,
// R_b R_f), so that the EE frame reproduces obs[1:4].
template <class L>
JDEV void body_frame_pose(const L& s, const JacoQueryFrame& F, v3* p, m3* R) {
  const int b = F.body;
  const m3 Rb = ldm(s.xmat[b]);
  *p = ld3(s.xpos[b]) + mul(Rb, ld3(F.pos));
  *R = mul(Rb, ldm(F.mat));
}
// The same for any frame: a world-fixed one (F.body < 0) is its own pose.  For the entries whose host half lets such a frame through.
template <class L>
JDEV void frame_pose(const L& s, const JacoQueryFrame& F, v3* p, m3* R) {
  *p = ld3(F.pos);
  *R = ldm(F.mat);
  if (F.body >= 0) body_frame_pose(s, F, p, R);
}
// The frame's Jacobian reference point in the world, from its pose (p, R).
JDEV v3 frame_point(const v3 p, const m3& R, const JacoQueryFrame& F) { return p + mul(R, ld3(F.point)); }

// The prologue of every entry: state row `row` into LDS exactly as the floats handed in (low-order words zero), then the model tables.
// ENTRY_CTRL: the ctrl row too (ctrl nullptr: zeros).  ENTRY_SUBSTEPS, for the entries that go on to run substeps: a zero warm start and
// zero row counters, as a fresh env has them.
enum { ENTRY_CTRL = 1, ENTRY_SUBSTEPS = 2 };
template <int WITH = 0, class L>
JDEV void entry_state(const JacoModelDev* m, L& s, const float* qpos, const float* qvel, const float* ctrl, int row, int lane) {
  const int nq = m->nq, nv = m->nv, nu = m->nu;
  if (lane < nq) { s.qpos[lane] = qpos[(size_t)row * nq + lane]; s.qpos_lo[lane] = 0.f; }
  if (lane < nv) {
    s.qvel[lane] = qvel[(size_t)row * nv + lane]; s.qvel_lo[lane] = 0.f;
    if (WITH & ENTRY_SUBSTEPS) s.qacc_ws[lane] = 0.f;
  }
  if ((WITH & ENTRY_CTRL) && lane < nu) s.ctrl[lane] = ctrl ? ctrl[(size_t)row * nu + lane] : 0.f;
  stage_model(m, s, lane);
  if ((WITH & ENTRY_SUBSTEPS) && lane == 0) { s.ncon = 0; s.nefc = 0; s.ncand = 0; s.nlimit = 0; s.nsphere = 0; s.nside = 0; s.nside_cand = 0; }   // (LDS is not zeroed between workgroups)
  wave_sync();
}

// The forward pass on the state in LDS, in two halves.  entry_walk: the step kernel's tree walk (no markers) and the zeroing of s.M;
// leaves the body poses of the current state in s.xpos / s.xmat.
template <class L>
JDEV void entry_walk(const JacoModelDev* m, L& s, int lane) {
  stage_walk(m, s, lane, false);
  for (int i = lane; i < JMBLK; i += 64) s.M[i] = 0.f;
  wave_sync();
}
// entry_mass_bias: subtree sums, then mass matrix + bias (s.M, s.bias, s.smooth = passive - bias).  The per-dof constants are fetched
// here, per call, and handed back for the stages that follow.
template <class L>
JDEV StagePrefetch entry_mass_bias(const JacoModelDev* m, L& s, int lane) {
  const StagePrefetch pf = stage_prefetch(m, lane);
  stage_accumulate(m, s, lane);
  wave_sync();
  stage_mass_bias(m, s, lane, pf);
  wave_sync();
  return pf;
}
// Both: the values of a sim.forward() on the state in LDS (mass: false stops after the walk).
template <class L>
JDEV void entry_forward(const JacoModelDev* m, L& s, int lane, bool mass = true) {
  entry_walk(m, s, lane);
  if (mass) entry_mass_bias(m, s, lane);
}
// Prologue and forward pass in one call: the values of a sim.forward() on state row `row`.  (One function on purpose.  The two calls
// written out in a kernel's body compile to another instruction schedule than this call does -- the compiler inlines by nesting level --
// and jaco_joint measured 0.35 % slower that way; called like this, its code is what it was when this was osc_task.h's osc_forward.)
template <class L>
JDEV void entry_state_forward(const JacoModelDev* m, L& s, const float* qpos, const float* qvel, int row, int lane) {
  entry_state(m, s, qpos, qvel, nullptr, row, lane);
  entry_forward(m, s, lane);
}

// Row `lane` of the block-diagonal mass matrix from s.M into registers, zero rows for lanes >= nv (run_env loads its mrow with the same
// loop: its twin, kept there as it is).
template <class L>
JDEV void mass_row(float (&mrow)[JNV], const L& s, int lane, int nv) {
  const int blo = lane < JB0 ? 0 : (lane < JB1 ? JB0 : JB1), bn = lane < JB0 ? JB0 : (lane < JB1 ? JB1 - JB0 : JNV - JB1);
  const int rbase = lane < nv ? m_index(lane, blo) : 0;
#pragma unroll
  for (int j = 0; j < JNV; j++) { const bool in = lane < nv && j >= blo && j < blo + bn; mrow[j] = in ? s.M[in ? rbase + j - blo : 0] : 0.f; }
}

// OR over the wavefront, in every lane: an xor butterfly of gathers (run_env reduces its flags with the same loop: its twin, kept there).
// Written on wave_shfl_i and lane_id, which the device's and the emulator's jaco/wave_ops.h both have: one text serves both builds.
JDEV unsigned wave_or(unsigned v) {
  for (int o = 1; o < 64; o <<= 1) v |= (unsigned)wave_shfl_i((int)v, lane_id() ^ o);
  return v;
}

// The kernel of an entry -- one 64-lane wavefront per item on the contact-free LDS type, items past `count` (an expression in the
// argument block Q) leave at once, run(Q, s, item, lane) does the work -- and its launcher, called by the host side (jaco_env.hip).
// Each entry header declares the launcher everywhere and defines kernel and launcher in its own translation unit:
//   #if JACO_TU_HAS(n)  JACO_DEFINE_ENTRY(...)  #else  JACO_DECLARE_ENTRY(...)  #endif
#if defined(JACO_EMULATED)
#define JACO_ENTRY_LAUNCHER(name, Args, body)
#elif defined(JACO_TU)
#define JACO_ENTRY_LAUNCHER(name, Args, body) void jaco_launch_##name(unsigned grid, hipStream_t st, const Args& Q) body
#else   // (a device build of every kernel at once: declarations only, as for the step kernels' launchers)
#define JACO_ENTRY_LAUNCHER(name, Args, body) void jaco_launch_##name(unsigned grid, hipStream_t st, const Args& Q);
#endif
#define JACO_DECLARE_ENTRY(name, Args) JACO_ENTRY_LAUNCHER(name, Args, ;)
#define JACO_DEFINE_ENTRY(name, Args, count, run)                                        \
  __global__ __launch_bounds__(64, 4) void jaco_##name##_kernel(Args Q) {                \
    __shared__ JacoLDS<JacoArm> s;                                                       \
    const int item = (int)blockIdx.x;                                                    \
    if (item >= (count)) return;                                                         \
    run(Q, s, item, (int)threadIdx.x);                                                   \
  }                                                                                      \
  JACO_ENTRY_LAUNCHER(name, Args, { hipLaunchKernelGGL(jaco_##name##_kernel, dim3(grid), dim3(64), 0, st, Q); })
