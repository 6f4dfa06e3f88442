// Batched rollouts under the operational-space controller (jaco_rollout_osc, include/jaco_env.h): jaco_rollout with the motor words of the
// ctrl computed inside the kernel by jaco_osc's law towards a plan of end-effector targets -- what a planner that samples EE targets
// (MPPI, CEM, shooting over waypoints) wants of a rollout, and the env's own substep loop ("OSC towards a target, then step") in one launch.
//
// One 64-lane wavefront per rollout on JacoLDS<JacoArm>, the whole knot x hold loop in the one launch: run_rollout of rollout.h itself,
// instantiated on this kernel's argument block -- the same prologue, substep, pose and status reduction.  What differs is where the ctrl
// comes from: rollout_substep opens between entry_mass_bias and stage_actuation and runs rollout_osc_law there.
//
// THE LAW, per evaluation.  Rollout i follows plan p = plan_idx[i] (NULL: i), at knot k:
//   1. s.ctrl[a] = ctrl[p][k][a] for every actuator a (a NULL ctrl: zeros) -- gripper commands and the other arm's words go through as
//      they come, as jaco_osc's ctrl_in does;
//   2. for each frame f < nframes: the frame's pose and point from s.xpos / s.xmat (body_frame_pose, frame_point), the target quaternion
//      normalised again (osc_unit_quat), stage_osc_frame of osc.h as it is on the frame's active dofs, target_pos[p][k][f], the gains;
//      s.ctrl[a] = Uo[dof(a)] for the motor actuator of every active dof (osc_write_ctrl's selection), every other word left alone;
//   3. the commanded row to the ctrl output ([n][E][nu], E = per_substep ? nknots * hold : nknots, lane = word), whether or not final_only
//      is set.  The actuator stage clamps u afterwards, as it clamps any ctrl.
// WHERE IT SITS AND WHY.  stage_osc_frame needs s.cdof, s.M, s.bias, s.qvel and the body poses: the substep has exactly those after
// entry_mass_bias, so the law costs no forward pass of its own.  They are THIS substep's own values -- fresh, as jaco_osc's are on the
// state it is handed, not one substep stale as the reference's controller reads them.  The law's scratch, s.J[0, 224 + JNV), is the row
// area: stage_mass_bias is done with it and stage_limit_rows writes it only after stage_actuation.  per_substep = 1 evaluates before every
// substep (the shape of the env's own loop); per_substep = 0 evaluates in the first substep of a knot and holds u over the knot.
// Nothing of the law lives across the rest of the substep: the actuator and per-dof constants are fetched after it (rollout_substep).
// Status: JFLAG_NAN and JFLAG_SOLVER_MAXITER as jaco_rollout, plus JROLLOUT_OSC_SINGULAR0 << f when any evaluation of frame f took the
// pseudo-inverse branch.  A state_idx or plan_idx entry out of range writes the status word JROLLOUT_BAD_INDEX and nothing else.
// OUT OF SCOPE: task axes and null-space terms (jaco_osc_task), an in-kernel cost, contacts -- validity is jaco_rollout's: the arm's
// free-space prediction with joint limits.
// No LDS beyond the step's.  Listed at the tail of physics_kernel.h; the kernel is translation unit 19 (kernels.hip -DJACO_TU=19).
#pragma once

#define JROLLOUT_OSC_SINGULAR0 0x200000u   // = JACO_ROLLOUT_OSC_SINGULAR0; frame 1: << 1 = JACO_ROLLOUT_OSC_SINGULAR1
struct JacoRolloutOscOpts {   // = JacoRolloutOscOptions of include/jaco_env.h (static_assert in abi_agreement.h)
  int nknots, hold, final_only, per_substep, nframes, reserved;
  float kp, ko, kv, vmax_xyz, vmax_abg;
  unsigned long long dof_mask;
};
struct JacoRolloutOscTargets {   // = JacoRolloutOscPlan of include/jaco_env.h
  const float* ctrl;          // [nplans][nknots][nu] or nullptr: zeros
  const float* target_pos;    // [nplans][nknots][nframes][3]
  const float* target_quat;   // [nplans][nknots][nframes][4]
  const int* plan_idx;        // [n] or nullptr: rollout i follows plan i
  int nplans;
};
struct JacoRolloutOscArgs {
  JacoRolloutArgs R;         // the open-loop kernel's block, first (rollout_pose and the shared halves read it); R.ctrl is the plans' base ctrl or nullptr
  JacoOscArgs O;             // the controller's block: target_pos / target_quat (the plans'), ctrl_out ([n][E][nu] or nullptr), nframes, active,
                             // sat_xyz, sat_abg, fr, opt; its state, ctrl_in, status and nenv are not used
  const int* plan_idx;
  int nplans, per_substep;
};

// The host half shared by jaco_rollout_osc (jaco_env.hip) and the emulator's entry: jaco_rollout_resolve_outputs' checks (status or ctrl
// alone will do as an output), then the plan's, then the controller's (jaco_osc_resolve_law).  The caller has filled in Q->R's state and
// output pointers and Q->O.ctrl_out as they were handed over.  Returns an empty string, or what is wrong.
static inline std::string jaco_rollout_osc_resolve(const JacoModelDev& m, const JacoRolloutOscOpts* o, const JacoQueryFrame* frames, int nframes,
                                                   const JacoQueryFrame* out_frame, int n, int nstates, int num_envs, const JacoRolloutOscTargets* plan,
                                                   bool have_out, JacoRolloutOscArgs* Q) {
  if (!plan) return "the plan is required";
  static const float no_ctrl = 0.f;
  Q->R.ctrl = plan->ctrl ? plan->ctrl : &no_ctrl;   // (jaco_rollout_resolve_outputs requires one; here NULL means zeros)
  {
    JacoRolloutOpts ro{};
    if (o) { ro.nknots = o->nknots; ro.hold = o->hold; ro.final_only = o->final_only; }
    const std::string why = jaco_rollout_resolve_outputs(m, o ? &ro : nullptr, out_frame, n, nstates, num_envs, have_out,
                                                         Q->R.qpos || Q->R.qvel || Q->R.xpos || Q->R.xmat || Q->R.status || Q->O.ctrl_out,
                                                         "at least one of the outputs qpos, qvel, xpos, xmat, status and ctrl is required", &Q->R);
    if (!why.empty()) return why;
  }
  Q->R.ctrl = plan->ctrl;
  if (o->per_substep != 0 && o->per_substep != 1) return "per_substep must be 0 or 1";
  if (plan->nplans < 1) return "nplans " + std::to_string(plan->nplans) + ": at least one plan is required";
  if (!plan->plan_idx && n > plan->nplans) return "n " + std::to_string(n) + " rollouts from " + std::to_string(plan->nplans) + " plans without a plan index";
  if (o->nframes != nframes) return "nframes " + std::to_string(nframes) + " but the options' nframes " + std::to_string(o->nframes);
  Q->O.target_pos = plan->target_pos; Q->O.target_quat = plan->target_quat;
  JacoOscOpts g;
  g.kp = o->kp; g.ko = o->ko; g.kv = o->kv; g.vmax_xyz = o->vmax_xyz; g.vmax_abg = o->vmax_abg; g.reserved = 0; g.dof_mask = o->dof_mask;
  const std::string why = jaco_osc_resolve_law(m, frames, nframes, g, plan->target_pos && plan->target_quat,
                                               "the target positions and the target quaternions are required", &Q->O);
  if (!why.empty()) return why;
  Q->plan_idx = plan->plan_idx; Q->nplans = plan->nplans;
  Q->per_substep = o->per_substep;
  return std::string();
}

// One evaluation of the law (the header's steps) for a rollout on plan p at knot k, into s.ctrl and row `erow` of the ctrl output; sets
// the frame's singular bit in `flags` (wave-uniform).  Runs inside the substep, after entry_mass_bias.
template <class L>
JDEV void rollout_osc_law(const JacoRolloutOscArgs* Q, const JacoModelDev* m, L& s, int p, int k, size_t erow, int lane, unsigned& flags) {
  const int nv = m->nv, nu = m->nu, nf = Q->O.nframes;
  const size_t pk = (size_t)p * Q->R.nknots + k;
  static_assert(224 + JNV <= sizeof(s.J) / sizeof(float), "Uo must lie inside the row area");
  if (lane < nu) s.ctrl[lane] = Q->R.ctrl ? Q->R.ctrl[pk * nu + lane] : 0.f;
  float* Uo = s.J + 224;   // [JNV] u_d by dof (where run_osc keeps it)
  const OscGains g = osc_gains(Q->O);
  unsigned all = 0u;
  for (int f = 0; f < nf; f++) {   // wave-uniform; s.M, s.bias and s.cdof serve every frame
    v3 pe;
    m3 Re;
    body_frame_pose(s, Q->O.fr[f], &pe, &Re);   // (the host half lets no world-fixed frame through)
    pe = frame_point(pe, Re, Q->O.fr[f]);
    const v3 pt = ld3(Q->O.target_pos + (pk * nf + f) * 3);
    float qd[4];
    osc_unit_quat(Q->O.target_quat + (pk * nf + f) * 4, qd);
    const unsigned act = Q->O.active[f];
    if (stage_osc_frame(s, lane, act, pe, Re, pt, qd, g, Uo)) flags |= JROLLOUT_OSC_SINGULAR0 << f;
    all |= act;
  }
  if (lane < nu) {   // the base row with the motor of every active dof replaced: every other word stays as it came
    const int d = m->a_dof[lane];
    const bool mine = m->a_position[lane] == 0 && d >= 0 && d < nv && ((all >> (d >= 0 ? d : 0)) & 1u) != 0u;
    if (mine) s.ctrl[lane] = Uo[d];
    if (Q->O.ctrl_out) Q->O.ctrl_out[erow * nu + lane] = s.ctrl[lane];
  }
  wave_sync();
}

// (the kernel: run_rollout of rollout.h on this block)
#if JACO_TU_HAS(19)
JACO_DEFINE_ENTRY(rollout_osc, JacoRolloutOscArgs, Q.R.n, run_rollout)
#else
JACO_DECLARE_ENTRY(rollout_osc, JacoRolloutOscArgs)
#endif
