// Batched closed-loop rollouts (jaco_rollout_fb, include/jaco_env.h): jaco_rollout with the ctrl of knot k computed inside the kernel from
// the state at knot k -- the forward pass of iLQR and its line search, a plan tracked with TVLQR gains, PD tracking of a joint trajectory.
//
// One 64-lane wavefront per rollout on JacoLDS<JacoArm>, the whole knot x hold loop in the one launch: run_rollout of rollout.h itself,
// instantiated on this kernel's argument block -- the same prologue, substep, pose and status reduction.  The one thing that differs is
// where run_rollout loads the knot's ctrl row into s.ctrl: here the feedback law is evaluated from the state in LDS.
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
// kernarg_view per substep by run_rollout, for the reason written there.
// A state_idx or plan_idx entry out of range writes the status word JROLLOUT_BAD_INDEX and nothing else.
// Listed at the tail of physics_kernel.h; the kernel is translation unit 16 (kernels.hip -DJACO_TU=16).
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

// The dof list of the law -- and of jaco_rollout_cost's state term -- checked and put into the block.
static inline std::string jaco_rollout_fb_dofs(const JacoModelDev& m, int ndofs, const int* dofs, JacoRolloutFbArgs* Q) {
  if (ndofs < 1 || ndofs > JROLLOUT_FB_MAX_DOFS) return "ndofs " + std::to_string(ndofs) + " outside [1, " + std::to_string(JROLLOUT_FB_MAX_DOFS) + "]";
  for (int j = 0; j < ndofs; j++) {
    const int d = dofs[j];
    if (d < 0 || d >= m.nv) return "dof " + std::to_string(d) + " outside [0, " + std::to_string(m.nv) + ")";
    if (m.d_qadr[d] < 0) return "dof " + std::to_string(d) + " belongs to a free joint";
    for (int k = 0; k < j; k++) if (dofs[k] == d) return "dof " + std::to_string(d) + " is listed twice";
    Q->dofs[j] = d;
  }
  Q->ndofs = ndofs;
  return std::string();
}

// The host half shared by jaco_rollout_fb (jaco_env.hip), the emulator's entry and, with its own rule for which outputs count
// (any_output, and the message when none is there), jaco_rollout_cost_resolve: jaco_rollout_resolve's checks, then the plan's and the
// law's.  The caller has filled in Q->R's state and output pointers and Q->ctrl_out as they were handed over.  Returns an empty
// string, or what is wrong.
static inline std::string jaco_rollout_fb_resolve_outputs(const JacoModelDev& m, const JacoRolloutFbOpts* o, const JacoQueryFrame* frame, int n, int nstates, int num_envs,
                                                          const JacoRolloutFbPlan* plan, bool have_out, bool any_output, const char* no_output, JacoRolloutFbArgs* Q) {
  if (!plan) return "the plan is required";
  Q->R.ctrl = plan->ctrl;
  {
    JacoRolloutOpts ro{};
    if (o) { ro.nknots = o->nknots; ro.hold = o->hold; ro.final_only = o->final_only; }
    const std::string why = jaco_rollout_resolve_outputs(m, o ? &ro : nullptr, frame, n, nstates, num_envs, have_out, any_output, no_output, &Q->R);
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
  if (plan->gain) return jaco_rollout_fb_dofs(m, o->ndofs, o->dofs, Q);
  return std::string();
}

// jaco_rollout_fb's own: status or ctrl alone will do as an output.
static inline std::string jaco_rollout_fb_resolve(const JacoModelDev& m, const JacoRolloutFbOpts* o, const JacoQueryFrame* frame, int n, int nstates, int num_envs,
                                                  const JacoRolloutFbPlan* plan, bool have_out, JacoRolloutFbArgs* Q) {
  return jaco_rollout_fb_resolve_outputs(m, o, frame, n, nstates, num_envs, plan, have_out,
                                         Q->R.qpos || Q->R.qvel || Q->R.xpos || Q->R.xmat || Q->R.status || Q->ctrl_out,
                                         "at least one of the outputs qpos, qvel, xpos, xmat, status and ctrl is required", Q);
}

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

// (the kernel: run_rollout of rollout.h on this block)
#if JACO_TU_HAS(16)
JACO_DEFINE_ENTRY(rollout_fb, JacoRolloutFbArgs, Q.R.n, run_rollout)
#else
JACO_DECLARE_ENTRY(rollout_fb, JacoRolloutFbArgs)
#endif
