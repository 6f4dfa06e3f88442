// Batched open-loop rollouts (jaco_rollout, include/jaco_env.h): what happens over the next nknots * hold substeps if this ctrl sequence
// is applied from this state?  mujoco.rollout.rollout(model, data, initial_state, control), contact-free.
//
// One 64-lane wavefront per rollout on the contact-free LDS type (JacoLDS<JacoArm>); the whole knot x hold loop runs inside the one
// launch with the state in LDS and registers.  The initial state is exactly the floats handed in (low words zero, as run_query), the
// warm start is zero and stage_model runs once.  Every substep (rollout_substep) is the contact-free substep of jaco_physics_step --
// what run_env<JacoArm> does for a real step under option disable_contact -- made of the step kernel's own stages, called as they are
// and in the same order:
//   stage_walk (no markers) and the zeroing of s.M, act_fetch / stage_prefetch, stage_accumulate, stage_mass_bias, stage_actuation,
//   stage_limit_rows, row `lane` of M into registers, stage_newton_limits (warm-started from the previous substep's qacc), the Euler
//   stage with implicit joint damping on the compensated pair (honouring m->compensated), stage_integrate_pos.
// Joint-limit rows are in, contacts are not; free bodies are integrated like everything else.  The status word collects JFLAG_NAN and
// JFLAG_SOLVER_MAXITER with the step kernel's rules and the rollout goes on, as the step does.
// Mapping: lane d owns dof d, position coordinate d and row d of M.  After the last substep of a knot the lanes store the fp32 (hi)
// state into that knot's contiguous output row, lane = word.  The frame pose of knot k is composed (as run_query composes frames) from
// the tree walk that the next substep runs anyway; only the last knot costs a walk of its own.  Lanes 0 .. 8 store the pose row's words.
// Fan-out: rollout i starts from state row state_idx[i] (NULL: row i); an index outside [0, nstates) writes the status word
// JROLLOUT_BAD_INDEX and nothing else.
// No LDS beyond the step's, no scratch memory.  Nothing of a handle is read but the model (and its fp32 state when no override is given).
// Listed at the tail of physics_kernel.h; the kernel is translation unit 15 (kernels.hip -DJACO_TU=15).
#pragma once
#include <string>
#include <type_traits>

#define JROLLOUT_MAX_SUBSTEPS 16384   // = JACO_ROLLOUT_MAX_SUBSTEPS
#define JROLLOUT_BAD_INDEX 0x80000u   // = JACO_ROLLOUT_BAD_INDEX
struct JacoRolloutOpts {   // = JacoRolloutOptions of include/jaco_env.h (static_assert in abi_agreement.h)
  int nknots, hold, final_only, reserved;
};
struct JacoRolloutArgs {
  const JacoModelDev* model;
  const int* state_idx;       // [n] or nullptr: rollout i starts from state row i
  const float* qpos0;         // [nstates][nq]  (the handle's hi words, or the caller's override)
  const float* qvel0;         // [nstates][nv]
  const float* ctrl;          // [n][nknots][nu]
  float* qpos;                // [n][rows][nq] or nullptr; rows = final_only ? 1 : nknots
  float* qvel;                // [n][rows][nv] or nullptr
  float* xpos;                // [n][rows][3] or nullptr
  float* xmat;                // [n][rows][9] or nullptr
  unsigned* status;           // [n] or nullptr
  int n, nstates, nknots, hold, final_only;
  JacoQueryFrame fr;          // by value: no device buffer, no upload (read only when xpos or xmat is wanted)
};

// The host half shared by jaco_rollout (jaco_env.hip), the emulator's entry and, with its own rule for which outputs count
// (any_output, and the message when none is there), jaco_rollout_fb_resolve: every argument check, then the options and the frame
// into the argument block, whose pointers the caller has filled in as they were handed over (qpos0 / qvel0 nullptr: the handle's state
// of num_envs rows, which the caller puts in afterwards; have_out: the output record was not NULL).  Returns an empty string, or what
// is wrong.
static inline std::string jaco_rollout_resolve_outputs(const JacoModelDev& m, const JacoRolloutOpts* o, const JacoQueryFrame* frame, int n, int nstates, int num_envs,
                                                       bool have_out, bool any_output, const char* no_output, JacoRolloutArgs* Q) {
  if (!o) return "the options are required";
  if (o->nknots < 1 || o->hold < 1 || (long long)o->nknots * o->hold > JROLLOUT_MAX_SUBSTEPS)
    return "nknots " + std::to_string(o->nknots) + " x hold " + std::to_string(o->hold) + ": both must be at least 1 and their product at most " + std::to_string(JROLLOUT_MAX_SUBSTEPS);
  if (o->final_only != 0 && o->final_only != 1) return "final_only must be 0 or 1";
  if (n < 0) return "n " + std::to_string(n) + " is negative";
  if (!Q->ctrl) return "the ctrl sequences are required";
  if (!have_out) return "the output record is required";
  if (!any_output) return no_output;
  if ((Q->xpos || Q->xmat) && !frame) return "xpos and xmat need a frame";
  if (frame && (frame->body < -1 || frame->body >= m.nbody)) return "frame body " + std::to_string(frame->body) + " outside [-1, " + std::to_string(m.nbody) + ")";
  if ((Q->qpos0 != nullptr) != (Q->qvel0 != nullptr)) return "qpos0 and qvel0 are given together or not at all";
  if (!Q->qpos0 && nstates != num_envs) return "nstates " + std::to_string(nstates) + " with the handle's state of " + std::to_string(num_envs) + " envs";
  if (Q->qpos0 && nstates < 1) return "nstates " + std::to_string(nstates) + " with a state override";
  if (!Q->state_idx && n > nstates) return "n " + std::to_string(n) + " rollouts from " + std::to_string(nstates) + " states without a state index";
  Q->n = n; Q->nstates = nstates;
  Q->nknots = o->nknots; Q->hold = o->hold; Q->final_only = o->final_only;
  if (frame) Q->fr = *frame;
  return std::string();
}

// jaco_rollout's own: one of the four state / pose outputs is required.
static inline std::string jaco_rollout_resolve(const JacoModelDev& m, const JacoRolloutOpts* o, const JacoQueryFrame* frame, int n, int nstates, int num_envs,
                                               bool have_out, JacoRolloutArgs* Q) {
  return jaco_rollout_resolve_outputs(m, o, frame, n, nstates, num_envs, have_out, Q->qpos || Q->qvel || Q->xpos || Q->xmat,
                                      "at least one of the outputs qpos, qvel, xpos and xmat is required", Q);
}

// A substep after its first half (entry_walk: the tree walk and the zeroing of s.M), from the subtree sums to the position update:
// run_env's contact-free substep body, stage by stage.
// law: what runs between entry_mass_bias and stage_actuation -- s.M, s.bias, s.cdof and the body poses are this substep's own there and the
// row area s.J is free (stage_mass_bias is done with it, stage_limit_rows writes it only afterwards) -- and leaves the ctrl in s.ctrl.
// rollout_no_law: nothing (the ctrl was put there before the walk).  With a law the actuator and per-dof constants are fetched after it,
// not held in registers across it.
struct JacoRolloutOscArgs;
template <class L>
JDEV void rollout_osc_law(const JacoRolloutOscArgs* Q, const JacoModelDev* m, L& s, int p, int k, size_t erow, int lane, unsigned& flags);
struct rollout_no_law { static constexpr bool present = false; };
struct rollout_osc_hook {   // rollout_osc_law (rollout_osc.h) on plan p at knot k into row erow of the ctrl output, when `on`
  static constexpr bool present = true;
  const JacoRolloutOscArgs* Q; int p, k; size_t erow; bool on;
};
template <class L, class Law = rollout_no_law>
JDEV void rollout_substep(const JacoModelDev* m, L& s, int lane, unsigned& flags, const Law law = Law()) {   // (by value: by reference the costed kernel's schedule moves)
  const int nv = m->nv;
  ActParams actp;
  StagePrefetch pf;
  if constexpr (!Law::present) {
    actp = act_fetch(m, lane);
    pf = entry_mass_bias(m, s, lane);
  } else {
    entry_mass_bias(m, s, lane);
    if (law.on) rollout_osc_law(law.Q, m, s, law.p, law.k, law.erow, lane, flags);
    actp = act_fetch(m, lane);
    pf = stage_prefetch(m, lane);
  }
  stage_actuation(m, s, lane, actp);
  stage_limit_rows(m, s, lane, pf);
  wave_sync();
  float mrow[JNV], h[JNV];
  mass_row(mrow, s, lane, nv);
  const float smooth = lane < nv ? s.smooth[lane] : 0.f;
  wave_sync();
  const float hdamp = (m->has_damping && lane < nv) ? m->timestep * pf.damping : 0.f;
  const NewtonOut nw = stage_newton_limits(m, s, mrow, smooth, hdamp, lane);
  if ((nw.iters & 255) >= m->iterations) flags |= JFLAG_SOLVER_MAXITER;
  wave_sync();
  // Euler with implicit joint damping: (M + h D) qacc = total on the damped block, the solver's qacc elsewhere
  const float total = smooth + nw.qfrc_con;
  float qacc_e = nw.qacc;
  if (m->has_damping) {
    float qd;
    if (nw.have_qdamped) qd = nw.qdamped;
    else {
#pragma unroll
      for (int j = 0; j < JNV; j++) h[j] = (lane < nv ? mrow[j] : 0.f) + (lane == j ? (lane < nv ? hdamp : 1.f) : 0.f);
      qd = ldl_solve_blocks(h, total, lane, JDAMPED_BLOCKS);
    }
    qacc_e = lane < JB0 ? qd : nw.qacc;
  }
  wave_sync();
  if (lane < nv) {
    float v;
    if (m->compensated) {
      const f2 nvl = comp_advance(s.qvel[lane], s.qvel_lo[lane], m->timestep, m->timestep_lo, qacc_e, 0.f);
      v = nvl.hi; s.qvel_lo[lane] = nvl.lo;
    } else v = s.qvel[lane] + m->timestep * qacc_e;
    s.qvel[lane] = v;
    s.qacc_ws[lane] = nw.qacc;
    if (!(v == v) || fabsf(v) > 1e10f) flags |= JFLAG_NAN;
  }
  wave_sync();
  stage_integrate_pos(m, s, lane);
  wave_sync();
}

// The frame's pose at the body poses in s.xpos / s.xmat (run_query's: frame_pose) into row `row` of the pose outputs: every lane
// composes it (the world-fixed case is wave-uniform), lane k stores word k.
// store = false: the pose is composed and nothing is stored (the costed kernel, for a knot whose row is not asked for).  Returns the position.
template <class L>
JDEV v3 rollout_pose(const JacoRolloutArgs& Q, const L& s, size_t row, int lane, bool store = true) {
  v3 p;
  m3 R;
  frame_pose(s, Q.fr, &p, &R);
  float w = lane == 0 ? p.x : (lane == 1 ? p.y : p.z), r = 0.f;
#pragma unroll
  for (int k = 0; k < 9; k++) if (lane == k) r = R.m[k];
  if (store && Q.xpos && lane < 3) Q.xpos[row * 3 + lane] = w;
  if (store && Q.xmat && lane < 9) Q.xmat[row * 9 + lane] = r;
  return p;
}

// The closed-loop kernel's block and law (rollout_fb.h) and the costed kernel's block and terms (rollout_cost.h), which the one loop
// below serves too.  rollout_kind<A>: what block A adds to the open loop -- closed: the ctrl of a knot comes from rollout_fb_law and the
// rollout follows a plan; costed: closed, plus the noise and the running cost.  The operational-space block and law (rollout_osc.h) too --
// osc: the rollout follows a plan of targets and the motor words of the ctrl come from rollout_osc_law, evaluated INSIDE the substep.
struct JacoRolloutFbArgs;
struct JacoRolloutCostArgs;
template <class L>
JDEV void rollout_fb_law(const JacoRolloutFbArgs* Q, const JacoModelDev* m, L& s, int i, int p, int k, size_t erow, int lane);
template <class L>
JDEV void rollout_cost_ctrl(const JacoRolloutCostArgs* Q, const JacoModelDev* m, L& s, int i, int k, int lane, float& acc);
template <class L>
JDEV void rollout_cost_state(const JacoRolloutCostArgs* Q, const JacoModelDev* m, const L& s, int p, int k, int lane, float& acc);
JDEV void rollout_cost_pose(const JacoRolloutCostArgs* Q, int p, int k, int lane, const v3 pos, float& acc);
JDEV void rollout_cost_finish(const JacoRolloutCostArgs* Q, int i, int lane, float acc, unsigned flags);
template <class A> struct rollout_kind {
  static constexpr bool costed = std::is_same<A, JacoRolloutCostArgs>::value;
  static constexpr bool closed = costed || std::is_same<A, JacoRolloutFbArgs>::value;
  static constexpr bool osc = std::is_same<A, JacoRolloutOscArgs>::value;
};
// the JacoRolloutFbArgs of a closed block: the block itself, or the costed block's F
template <class A>
JDEV const JacoRolloutFbArgs* rollout_law_block(const A* Q) {
  if constexpr (rollout_kind<A>::costed) return &Q->F; else return Q;
}
// the JacoRolloutArgs of any block: the block itself, or the closed-loop / operational-space block's R
template <class A>
JDEV const JacoRolloutArgs* rollout_block(const A* Q) {
  if constexpr (rollout_kind<A>::closed) return &rollout_law_block(Q)->R;
  else if constexpr (rollout_kind<A>::osc) return &Q->R;
  else return Q;
}

// The knot x hold loop of rollout i, for jaco_rollout (A = JacoRolloutArgs), jaco_rollout_fb (A = JacoRolloutFbArgs),
// jaco_rollout_cost (A = JacoRolloutCostArgs) and jaco_rollout_osc (A = JacoRolloutOscArgs).  They differ in where a knot's ctrl comes from
// -- its row of the ctrl sequences, loaded once per knot, rollout_fb_law evaluated on the state in LDS, per knot or per substep, or
// rollout_osc_law evaluated inside the substep on its mass matrix, bias and poses -- in the plan index of all but the first, and in
// the costed kernel's terms (rollout_cost.h says where they are formed and why there).
template <class A, class L>
JDEV void run_rollout(const A& Q_, L& s, int i, int lane) {
  constexpr bool closed = rollout_kind<A>::closed, costed = rollout_kind<A>::costed, osc = rollout_kind<A>::osc;
  const A* Qp = kernarg_view(Q_);
  const JacoRolloutArgs* R = rollout_block(Qp);
  const JacoModelDev* m = opaque_ptr(R->model);
  const int nq = m->nq, nv = m->nv, nu = m->nu;
  const int src = wave_uniform_i(R->state_idx ? R->state_idx[i] : i);
  int p = 0;
  bool bad = src < 0 || src >= R->nstates;
  if constexpr (closed) {
    const auto* F = rollout_law_block(Qp);   // (JacoRolloutFbArgs, complete by the time this is instantiated)
    p = wave_uniform_i(F->plan.plan_idx ? F->plan.plan_idx[i] : i);
    bad = bad || p < 0 || p >= F->plan.nplans;
  }
  if constexpr (osc) {
    p = wave_uniform_i(Qp->plan_idx ? Qp->plan_idx[i] : i);
    bad = bad || p < 0 || p >= Qp->nplans;
  }
  if (bad) {   // (as jaco_load_envs: neither a fault nor silence)
    if (lane == 0 && R->status) R->status[i] = JROLLOUT_BAD_INDEX;
    return;
  }
  // the state row exactly as the floats handed in, a zero warm start, the model staged once
  entry_state<ENTRY_SUBSTEPS>(m, s, R->qpos0, R->qvel0, nullptr, src, lane);
  unsigned flags = 0u;
  const int nknots = R->nknots, hold = R->hold;
  const bool every = R->final_only == 0, pose = R->xpos != nullptr || R->xmat != nullptr;
  bool each = false;
  if constexpr ((closed && !costed) || osc) each = Qp->per_substep != 0;
  float acc = 0.f;   // (the costed kernel's one accumulator per lane)
#pragma nounroll
  for (int k = 0; k < nknots; k++) {
    if constexpr (!closed && !osc) {
      if (lane < nu) s.ctrl[lane] = R->ctrl[((size_t)i * nknots + k) * nu + lane];
      wave_sync();
    }
#pragma nounroll
    for (int sub = 0; sub < hold; sub++) {
      // (as run_env's substep loop and fd_pass: the argument block is read afresh, and with the pointer's provenance and the lane id
      // hidden the optimiser cannot hoist the substep's model loads and lane-derived addresses out of the loop and keep them alive,
      // spilled, across all of it)
      Qp = kernarg_view(Q_);
      R = rollout_block(Qp);
      m = opaque_ptr(R->model);
      lane = wave_opaque_i(lane);
      if constexpr (closed) {
        if (each || sub == 0) {
          rollout_fb_law(rollout_law_block(Qp), m, s, i, p, k, each ? ((size_t)i * nknots + k) * hold + sub : (size_t)i * nknots + k, lane);
          if constexpr (costed) rollout_cost_ctrl(Qp, m, s, i, k, lane, acc);
        }
      }
      entry_walk(m, s, lane);
      bool knot_pose = pose && every;
      if constexpr (costed) knot_pose = knot_pose || Qp->wp != 0.f;
      if (knot_pose && sub == 0 && k > 0) {   // the previous knot's pose: this walk's
        const v3 pos = rollout_pose(*R, s, (size_t)i * nknots + (k - 1), lane, pose && every);
        if constexpr (costed) rollout_cost_pose(Qp, p, k - 1, lane, pos, acc);
      }
      if constexpr (osc) {
        const rollout_osc_hook law{Qp, p, k, each ? ((size_t)i * nknots + k) * hold + sub : (size_t)i * nknots + k, each || sub == 0};
        rollout_substep(m, s, lane, flags, law);
      } else rollout_substep(m, s, lane, flags);
    }
    if (every || k == nknots - 1) {
      const size_t row = every ? (size_t)i * nknots + k : (size_t)i;
      if (R->qpos && lane < nq) R->qpos[row * nq + lane] = s.qpos[lane];
      if (R->qvel && lane < nv) R->qvel[row * nv + lane] = s.qvel[lane];
    }
    if constexpr (costed) rollout_cost_state(Qp, m, s, p, k, lane, acc);
  }
  Qp = kernarg_view(Q_);
  R = rollout_block(Qp);
  bool last_pose = pose;
  if constexpr (costed) last_pose = last_pose || Qp->wp != 0.f || Qp->wpT != 0.f;
  if (last_pose) {   // the last knot's pose needs a walk of its own
    stage_walk(opaque_ptr(R->model), s, lane, false);
    wave_sync();
    const v3 pos = rollout_pose(*R, s, every ? (size_t)i * nknots + (nknots - 1) : (size_t)i, lane);
    if constexpr (costed) rollout_cost_pose(Qp, p, nknots - 1, lane, pos, acc);
  }
  if (R->status || costed) {   // the lanes' sticky flags, or-reduced over the wavefront
    const unsigned f = wave_or(flags);
    if (lane == 0 && R->status) R->status[i] = f;
    if constexpr (costed) rollout_cost_finish(Qp, i, lane, acc, f);
  }
}

#if JACO_TU_HAS(15)
JACO_DEFINE_ENTRY(rollout, JacoRolloutArgs, Q.n, run_rollout)
#else
JACO_DECLARE_ENTRY(rollout, JacoRolloutArgs)
#endif
