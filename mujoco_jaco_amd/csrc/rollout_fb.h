// Batched closed-loop rollouts (jaco_rollout_fb, include/jaco_env.h): jaco_rollout with the ctrl of knot k computed inside the kernel from
// the state at knot k -- the forward pass of iLQR and its line search, a plan tracked with TVLQR gains, PD tracking of a joint trajectory.
//
// One 64-lane wavefront per rollout on JacoLDS<JacoArm>, the whole knot x hold loop in the one launch: run_rollout of rollout.h with its
// prologue, rollout_walk, rollout_substep, rollout_pose and status reduction called as they are.  The one thing that differs is where
// run_rollout loads the knot's ctrl row into s.ctrl: here the feedback law is evaluated from the state in LDS.
//
// THE LAW (the order of operations is part of the interface: tests recompute it).  Rollout i follows plan p = plan_idx[i] (NULL: i); at
// an evaluation in knot k, with nd = ndofs and nx = 2 nd:
//   x_j = qpos[d_qadr[dofs[j]]] for j < nd, qvel[dofs[j - nd]] for nd <= j < nx     (the fp32 high words of the state)
//   d_j = x_j - xref[p][k][j]                                                        (one fp32 subtraction, not wrapped)
//   u_a = kff ? fmaf(alpha_i, kff[p][k][a], ctrl[p][k][a]) : ctrl[p][k][a]           (alpha NULL: 1.0f)
//   u_a = fmaf(gain[p][k][a][j], d_j, u_a)   for j = 0 .. nx-1, ascending            (gain NULL: skipped)
//   s.ctrl[a] = u_a   for every actuator a = 0 .. nu-1
// u is the commanded value; the actuator stage clamps it to ctrlrange afterwards, as it clamps any ctrl.  per_substep = 0 evaluates the
// law before the first substep of a knot and holds it (zero-order hold); per_substep = 1 evaluates it before every substep, against the
// same knot's rows.  Every evaluation's u goes to the ctrl output ([n][E][nu], E = nknots or nknots * hold, lane = word) whether or not
// final_only is set.
// Mapping: lane j < nx forms d_j in a register; lane a < nu accumulates u_a, fetching d_j with wave_bcast (j is wave-uniform) and reading
// its gain row gain[p][k][a][0 .. nx) -- contiguous -- at the point of use, all of it in flight before the first fma.  Nothing of the law lives across a substep; no LDS beyond the
// step's, no scratch memory.  The options (the dof list included) and the frame travel by value in the kernel arguments, re-read through
// rollout_fb_args_view per substep as run_rollout does and for the reason written there.
// A state_idx or plan_idx entry out of range writes the status word JROLLOUT_BAD_INDEX and nothing else.
// Included at the end of rollout.h; the kernel is translation unit 16 (kernels.hip -DJACO_TU=16).
#pragma once

#define JROLLOUT_FB_MAX_DOFS 18   // = JACO_ROLLOUT_FB_MAX_DOFS
struct JacoRolloutFbOpts {   // = JacoRolloutFbOptions of include/jaco_env.h (static_assert in abi_agreement.h)
  int nknots, hold, final_only, per_substep;
  int ndofs;
  int dofs[JROLLOUT_FB_MAX_DOFS];
  int reserved;
};
struct JacoRolloutFbPlan {   // = JacoRolloutPlan of include/jaco_env.h
  const float* ctrl;       // [nplans][nknots][nu]
  const float* kff;        // [nplans][nknots][nu] or nullptr
  const float* gain;       // [nplans][nknots][nu][nx] or nullptr
  const float* xref;       // [nplans][nknots][nx], with gain
  const float* alpha;      // [n] or nullptr
  const int* plan_idx;     // [n] or nullptr: rollout i follows plan i
  int nplans;
};
struct JacoRolloutFbArgs {
  JacoRolloutArgs R;         // the open-loop kernel's block, first (rollout_pose and the shared halves read it); R.ctrl is the plans' ctrl
  JacoRolloutFbPlan plan;
  float* ctrl_out;           // [n][E][nu] or nullptr; E = per_substep ? nknots * hold : nknots
  int per_substep, ndofs;
  int dofs[JROLLOUT_FB_MAX_DOFS];
};

// The host half shared by jaco_rollout_fb (jaco_env.hip) and the emulator's entry: jaco_rollout_resolve's checks, then the plan's and
// the law's.  The caller has filled in Q->R's state and output pointers and Q->ctrl_out as they were handed over.  Returns an empty
// string, or what is wrong.
static inline std::string jaco_rollout_fb_resolve(const JacoModelDev& m, const JacoRolloutFbOpts* o, const JacoQueryFrame* frame, int n, int nstates, int num_envs,
                                                  const JacoRolloutFbPlan* plan, bool have_out, JacoRolloutFbArgs* Q) {
  if (!plan) return "the plan is required";
  Q->R.ctrl = plan->ctrl;
  {
    JacoRolloutOpts ro{};
    if (o) { ro.nknots = o->nknots; ro.hold = o->hold; ro.final_only = o->final_only; }
    const bool any = Q->R.qpos || Q->R.qvel || Q->R.xpos || Q->R.xmat || Q->R.status || Q->ctrl_out;   // (here status or ctrl alone will do)
    const std::string why = jaco_rollout_resolve_outputs(m, o ? &ro : nullptr, frame, n, nstates, num_envs, have_out, any,
                                                         "at least one of the outputs qpos, qvel, xpos, xmat, status and ctrl is required", &Q->R);
    if (!why.empty()) return why;
  }
  if (o->per_substep != 0 && o->per_substep != 1) return "per_substep must be 0 or 1";
  if (plan->nplans < 1) return "nplans " + std::to_string(plan->nplans) + ": at least one plan is required";
  if (!plan->plan_idx && n > plan->nplans) return "n " + std::to_string(n) + " rollouts from " + std::to_string(plan->nplans) + " plans without a plan index";
  if (plan->gain && !plan->xref) return "a gain needs xref";
  if (plan->alpha && !plan->kff) return "alpha needs kff";
  Q->plan = *plan;
  Q->per_substep = o->per_substep;
  Q->ndofs = 0;
  if (plan->gain) {
    if (o->ndofs < 1 || o->ndofs > JROLLOUT_FB_MAX_DOFS) return "ndofs " + std::to_string(o->ndofs) + " outside [1, " + std::to_string(JROLLOUT_FB_MAX_DOFS) + "]";
    for (int j = 0; j < o->ndofs; j++) {
      const int d = o->dofs[j];
      if (d < 0 || d >= m.nv) return "dof " + std::to_string(d) + " outside [0, " + std::to_string(m.nv) + ")";
      if (m.d_qadr[d] < 0) return "dof " + std::to_string(d) + " belongs to a free joint";
      for (int k = 0; k < j; k++) if (o->dofs[k] == d) return "dof " + std::to_string(d) + " is listed twice";
      Q->dofs[j] = d;
    }
    Q->ndofs = o->ndofs;
  }
  return std::string();
}

// (as rollout_args_view)
#ifdef JACO_EMULATED
JDEV const JacoRolloutFbArgs* rollout_fb_args_view(const JacoRolloutFbArgs& Q) { return &Q; }
#else
JDEV const JacoRolloutFbArgs* rollout_fb_args_view(const JacoRolloutFbArgs&) {
  typedef const JacoRolloutFbArgs __attribute__((address_space(4))) * KP;
  KP p = (KP)__builtin_amdgcn_kernarg_segment_ptr();
  return (const JacoRolloutFbArgs*)p;
}
#endif

// One evaluation of the law (the header's order of operations) for rollout i on plan p at knot k, into s.ctrl and row `erow` of the ctrl
// output.  Every lane runs the j loop: wave_bcast is a wavefront operation.
template <class L>
JDEV void rollout_fb_law(const JacoRolloutFbArgs* Q, const JacoModelDev* m, L& s, int i, int p, int k, size_t erow, int lane) {
  const int nu = m->nu, nd = Q->ndofs, nx = 2 * nd;
  const size_t pk = (size_t)p * Q->R.nknots + k;
  const float* gain = Q->plan.gain;
  float d = 0.f;
  if (gain && lane < nx) {
    const int dof = Q->dofs[lane < nd ? lane : lane - nd];
    const float x = lane < nd ? s.qpos[m->d_qadr[dof]] : s.qvel[dof];
    d = x - Q->plan.xref[pk * nx + lane];
  }
  const int a = lane < nu ? lane : 0;
  float u = Q->R.ctrl[pk * nu + a];
  if (Q->plan.kff) u = fmaf(Q->plan.alpha ? Q->plan.alpha[i] : 1.0f, Q->plan.kff[pk * nu + a], u);
  if (gain) {
    // the whole row first (nx is even: pair by pair under wave-uniform guards, every load in flight before the first use), then the
    // fmas in ascending j with d_j from lane j -- a gain row fetched word by word inside the j loop pays one memory latency per word
    const float* row = gain + (pk * nu + a) * nx;
    float g[2 * JROLLOUT_FB_MAX_DOFS];
#pragma unroll
    for (int c = 0; c < JROLLOUT_FB_MAX_DOFS; c++)
      if (c < nd) { g[2 * c] = row[2 * c]; g[2 * c + 1] = row[2 * c + 1]; }
#pragma unroll
    for (int c = 0; c < JROLLOUT_FB_MAX_DOFS; c++)
      if (c < nd) {
        u = fmaf(g[2 * c], wave_bcast(d, 2 * c), u);
        u = fmaf(g[2 * c + 1], wave_bcast(d, 2 * c + 1), u);
      }
  }
  if (lane < nu) {
    s.ctrl[lane] = u;
    if (Q->ctrl_out) Q->ctrl_out[erow * nu + lane] = u;
  }
  wave_sync();
}

template <class L>
JDEV void run_rollout_fb(const JacoRolloutFbArgs& Q_, L& s, int i, int lane) {
  const JacoRolloutFbArgs* Qp = rollout_fb_args_view(Q_);
  const JacoModelDev* m = opaque_ptr(Qp->R.model);
  const int nq = m->nq, nv = m->nv;
  const int src = wave_uniform_i(Qp->R.state_idx ? Qp->R.state_idx[i] : i);
  const int p = wave_uniform_i(Qp->plan.plan_idx ? Qp->plan.plan_idx[i] : i);
  if (src < 0 || src >= Qp->R.nstates || p < 0 || p >= Qp->plan.nplans) {   // (as run_rollout: neither a fault nor silence)
    if (lane == 0 && Qp->R.status) Qp->R.status[i] = JROLLOUT_BAD_INDEX;
    return;
  }
  rollout_prologue(&Qp->R, m, s, src, lane);
  unsigned flags = 0u;
  const int nknots = Qp->R.nknots, hold = Qp->R.hold;
  const bool every = Qp->R.final_only == 0, pose = Qp->R.xpos != nullptr || Qp->R.xmat != nullptr, each = Qp->per_substep != 0;
#pragma nounroll
  for (int k = 0; k < nknots; k++) {
#pragma nounroll
    for (int sub = 0; sub < hold; sub++) {
      // (as run_rollout's substep loop: the argument block is read afresh, the pointer's provenance and the lane id hidden)
      Qp = rollout_fb_args_view(Q_);
      m = opaque_ptr(Qp->R.model);
      lane = wave_opaque_i(lane);
      if (each || sub == 0) rollout_fb_law(Qp, m, s, i, p, k, each ? ((size_t)i * nknots + k) * hold + sub : (size_t)i * nknots + k, lane);
      rollout_walk(m, s, lane);
      if (pose && every && sub == 0 && k > 0) rollout_pose(Qp->R, s, (size_t)i * nknots + (k - 1), lane);   // the previous knot's pose: this walk's
      rollout_substep(m, s, lane, flags);
    }
    if (every || k == nknots - 1) {
      const size_t row = every ? (size_t)i * nknots + k : (size_t)i;
      if (Qp->R.qpos && lane < nq) Qp->R.qpos[row * nq + lane] = s.qpos[lane];
      if (Qp->R.qvel && lane < nv) Qp->R.qvel[row * nv + lane] = s.qvel[lane];
    }
  }
  Qp = rollout_fb_args_view(Q_);
  if (pose) {   // the last knot's pose needs a walk of its own
    stage_walk(opaque_ptr(Qp->R.model), s, lane, false);
    wave_sync();
    rollout_pose(Qp->R, s, every ? (size_t)i * nknots + (nknots - 1) : (size_t)i, lane);
  }
  rollout_status(&Qp->R, flags, i, lane);
}

#if JACO_TU_HAS(16)
__global__ __launch_bounds__(64, 4) void jaco_rollout_fb_kernel(JacoRolloutFbArgs Q) {
  __shared__ JacoLDS<JacoArm> s;
  const int i = (int)blockIdx.x;
  if (i >= Q.R.n) return;
  run_rollout_fb(Q, s, i, (int)threadIdx.x);
}
#endif

#ifndef JACO_EMULATED
void jaco_launch_rollout_fb(unsigned grid, hipStream_t st, const JacoRolloutFbArgs& Q);
#if defined(JACO_TU) && JACO_TU == 16
void jaco_launch_rollout_fb(unsigned grid, hipStream_t st, const JacoRolloutFbArgs& Q) { hipLaunchKernelGGL(jaco_rollout_fb_kernel, dim3(grid), dim3(64), 0, st, Q); }
#endif
#endif

// the iLQR / TVLQR backward pass kernel (jaco_lqr): translation unit 17
#include "lqr.h"
