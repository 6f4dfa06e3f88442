// Batched costed rollouts (jaco_rollout_cost, include/jaco_env.h): jaco_rollout_fb with a per-rollout additive perturbation of the commanded
// ctrl and a running quadratic cost accumulated inside the kernel -- what MPPI, CEM, random shooting and iLQR's line search want of a
// rollout: one number, not the trajectory.
//
// One 64-lane wavefront per rollout on JacoLDS<JacoArm>, the whole knot x hold loop in the one launch: run_rollout of rollout.h itself,
// instantiated on this kernel's argument block -- the same prologue, law (rollout_fb_law, once per knot), substep, pose and status
// reduction.  What this header adds is called from run_rollout at three places, under rollout_kind<A>::costed:
//   rollout_cost_ctrl   after the law: u_a = u_a + noise[i][k][a] (ONE fp32 add, part of the interface) into s.ctrl and the ctrl output,
//                       and the ctrl term of knot k;
//   rollout_cost_state  after the last substep of knot k, where the qpos / qvel rows are stored: the state term on the same words;
//   rollout_cost_pose   where rollout_pose runs (the walk of the next knot's first substep; the final walk for the last knot), on the
//                       very frame_pose result rollout_pose stores: the pose term.  With wp == 0 only the final walk's pose is formed.
//
// THE COST.  x: the fp32 state on the option's dofs (the law's x_j), nx = 2 ndofs; pos: the frame's position; g = goal_per_knot ? k : 0:
//   J_i = sum_k [ 1/2 sum_a wu[a] u_ka^2 + 1/2 sum_j WX_k[j] (x_(k+1)j - xgoal[p][g][j])^2 + 1/2 WP_k |pos_(k+1) - pgoal[p][g]|^2 ]
// with (WX_k, WP_k) = (wx, wp) for k < T - 1 and (wxT, wpT) for the last knot; x_(k+1), pos_(k+1) are the words row k of the qpos / qvel
// / xpos outputs holds.  Differences are not wrapped.  The order of the sum is not part of the interface; it is fixed, so two runs agree
// bit for bit, and it does not depend on final_only or on which outputs are asked for.
// Mapping: ONE accumulator register per lane, the lanes partitioned by term: lane j in [0, 36) accumulates state word j, lane 36 + a in
// [36, 54) ctrl word a (read back from s.ctrl), lane 54 + c in [54, 57) pose component c.  Each term of a knot is one subtraction, one
// square and one fmaf onto the lane's accumulator; the weights and goals are read at the point of use (the weights through kernarg_view:
// a by-value array under a lane index would otherwise go to scratch), nothing else of the cost lives across a substep.  After the loop
// three masked wave_sums give terms = (ctrl, state, pose) and cost = (ctrl + state) + pose.  A rollout whose status has JFLAG_NAN writes
// +inf to all four, so a softmin ignores it.
// No LDS beyond the step's, no scratch memory.  A state_idx or plan_idx entry out of range writes the status word JROLLOUT_BAD_INDEX and
// nothing else.
// Listed at the tail of physics_kernel.h; the kernel is translation unit 18 (kernels.hip -DJACO_TU=18).
#pragma once
#include <cmath>

#define JROLLOUT_COST_MAX_NU 18   // = JACO_ROLLOUT_COST_MAX_NU
#define JRC_NX (2 * JROLLOUT_FB_MAX_DOFS)
#define JRC_LANE_U JRC_NX                              // first lane of the ctrl term
#define JRC_LANE_P (JRC_NX + JROLLOUT_COST_MAX_NU)     // first lane of the pose term
static_assert(JRC_LANE_P + 3 <= 64, "the three terms' lanes must fit one wavefront");

struct JacoRolloutCostOpts {   // = JacoRolloutCostOptions of include/jaco_env.h (static_assert in abi_agreement.h)
  int nknots, hold, final_only, goal_per_knot;
  int ndofs;
  int dofs[JROLLOUT_FB_MAX_DOFS];
  float wx[JRC_NX], wxT[JRC_NX], wu[JROLLOUT_COST_MAX_NU], wp, wpT;
  int reserved;
};
struct JacoRolloutCostGoal {   // = JacoRolloutGoal of include/jaco_env.h
  const float* noise;      // [n][nknots][nu] or nullptr
  const float* xgoal;      // [nplans][G][nx] or nullptr; G = goal_per_knot ? nknots : 1
  const float* pgoal;      // [nplans][G][3] or nullptr
};
struct JacoRolloutCostArgs {
  JacoRolloutFbArgs F;       // the closed-loop kernel's block, first (the law and the shared halves read it); F.ctrl_out is nullptr: the
                             // ctrl output is written here, after the noise
  JacoRolloutCostGoal goal;
  float* ctrl_out;           // [n][nknots][nu] or nullptr
  float* cost;               // [n] or nullptr
  float* terms;              // [n][3] or nullptr
  int goal_per_knot;
  float wp, wpT;
  float wx[JRC_NX], wxT[JRC_NX], wu[JROLLOUT_COST_MAX_NU];
};

// The host half shared by jaco_rollout_cost (jaco_env.hip) and the emulator's entry: jaco_rollout_fb_resolve's checks with no per_substep
// and eight outputs, then the cost's own.  The caller has filled in Q->F.R's state and output pointers, Q->F.ctrl_out (the ctrl output, moved
// to Q->ctrl_out here), Q->cost and Q->terms as they were handed over.  Returns an empty string, or what is wrong.
static inline std::string jaco_rollout_cost_resolve(const JacoModelDev& m, const JacoRolloutCostOpts* o, const JacoQueryFrame* frame, int n, int nstates, int num_envs,
                                                    const JacoRolloutFbPlan* plan, const JacoRolloutCostGoal* goal, bool have_out, JacoRolloutCostArgs* Q) {
  {
    JacoRolloutFbOpts fo{};
    if (o) {
      fo.nknots = o->nknots; fo.hold = o->hold; fo.final_only = o->final_only; fo.ndofs = o->ndofs;
      for (int j = 0; j < JROLLOUT_FB_MAX_DOFS; j++) fo.dofs[j] = o->dofs[j];
    }
    const bool any = Q->F.R.qpos || Q->F.R.qvel || Q->F.R.xpos || Q->F.R.xmat || Q->F.R.status || Q->F.ctrl_out || Q->cost || Q->terms;
    const std::string why = jaco_rollout_fb_resolve_outputs(m, o ? &fo : nullptr, frame, n, nstates, num_envs, plan, have_out, any,
                                                            "at least one of the outputs qpos, qvel, xpos, xmat, status, ctrl, cost and terms is required", &Q->F);
    if (!why.empty()) return why;
  }
  if (o->goal_per_knot != 0 && o->goal_per_knot != 1) return "goal_per_knot must be 0 or 1";
  if (m.nu > JROLLOUT_COST_MAX_NU) return "the model's nu " + std::to_string(m.nu) + " is above " + std::to_string(JROLLOUT_COST_MAX_NU);
  bool state = false;
  const auto bad = [](float w) { return !(w >= 0.f) || !std::isfinite(w); };
  for (int j = 0; j < JRC_NX; j++) {
    if (bad(o->wx[j])) return "weight wx[" + std::to_string(j) + "] is negative or not finite";
    if (bad(o->wxT[j])) return "weight wxT[" + std::to_string(j) + "] is negative or not finite";
    state = state || o->wx[j] != 0.f || o->wxT[j] != 0.f;
  }
  for (int a = 0; a < JROLLOUT_COST_MAX_NU; a++)
    if (bad(o->wu[a])) return "weight wu[" + std::to_string(a) + "] is negative or not finite";
  if (bad(o->wp)) return "weight wp is negative or not finite";
  if (bad(o->wpT)) return "weight wpT is negative or not finite";
  const bool pose = o->wp != 0.f || o->wpT != 0.f;
  if (state && !(goal && goal->xgoal)) return "a non-zero state weight needs xgoal";
  if (state && !plan->gain) {   // (with a gain the dofs are checked already)
    if (o->ndofs == 0) return "a non-zero state weight needs dofs";
    const std::string why = jaco_rollout_fb_dofs(m, o->ndofs, o->dofs, &Q->F);
    if (!why.empty()) return why;
  }
  if (pose && !(goal && goal->pgoal)) return "a non-zero pose weight needs pgoal";
  if (pose && !frame) return "a non-zero pose weight needs a frame";
  if (goal) Q->goal = *goal;
  if (!state) Q->goal.xgoal = nullptr;   // (the kernel forms the state term where xgoal is there)
  if (!pose) Q->goal.pgoal = nullptr;
  Q->ctrl_out = Q->F.ctrl_out; Q->F.ctrl_out = nullptr;
  Q->goal_per_knot = o->goal_per_knot;
  Q->wp = o->wp; Q->wpT = o->wpT;
  for (int j = 0; j < JRC_NX; j++) { Q->wx[j] = o->wx[j]; Q->wxT[j] = o->wxT[j]; }
  for (int a = 0; a < JROLLOUT_COST_MAX_NU; a++) Q->wu[a] = o->wu[a];
  return std::string();
}

// One term onto the lane's accumulator: 1/2 w d^2.
JDEV void rollout_cost_add(float& acc, float w, float d) { acc = fmaf(0.5f * w, d * d, acc); }

// After the law of knot k: the noise (one fp32 add onto the law's u, read back from s.ctrl) into s.ctrl, the ctrl output row, and the
// ctrl term in lanes JRC_LANE_U + a.
template <class L>
JDEV void rollout_cost_ctrl(const JacoRolloutCostArgs* Q, const JacoModelDev* m, L& s, int i, int k, int lane, float& acc) {
  const int nu = m->nu;
  const size_t row = ((size_t)i * Q->F.R.nknots + k) * nu;
  if (lane < nu) {
    float u = s.ctrl[lane];
    if (Q->goal.noise) {
      u = u + Q->goal.noise[row + lane];
      s.ctrl[lane] = u;
    }
    if (Q->ctrl_out) Q->ctrl_out[row + lane] = u;
  }
  wave_sync();
  const int a = lane - JRC_LANE_U;
  if (a >= 0 && a < nu) {
    const float w = Q->wu[a];
    if (w != 0.f) rollout_cost_add(acc, w, s.ctrl[a]);
  }
}

// After the last substep of knot k: the state term on the words the qpos / qvel rows hold, in lanes j < nx.
template <class L>
JDEV void rollout_cost_state(const JacoRolloutCostArgs* Q, const JacoModelDev* m, const L& s, int p, int k, int lane, float& acc) {
  const float* xgoal = Q->goal.xgoal;
  if (!xgoal) return;
  const int nd = Q->F.ndofs, nx = 2 * nd, T = Q->F.R.nknots;
  if (lane < nx) {
    const float w = k == T - 1 ? Q->wxT[lane] : Q->wx[lane];
    if (w != 0.f) {
      const int dof = Q->F.dofs[lane < nd ? lane : lane - nd];
      const float x = lane < nd ? s.qpos[m->d_qadr[dof]] : s.qvel[dof];
      const size_t g = Q->goal_per_knot ? (size_t)p * T + k : (size_t)p;
      rollout_cost_add(acc, w, x - xgoal[g * nx + lane]);
    }
  }
}

// Where the pose of knot k has been composed (pos: rollout_pose's result): the pose term, in lanes JRC_LANE_P + c.
JDEV void rollout_cost_pose(const JacoRolloutCostArgs* Q, int p, int k, int lane, const v3 pos, float& acc) {
  const int T = Q->F.R.nknots, c = lane - JRC_LANE_P;
  const float w = k == T - 1 ? Q->wpT : Q->wp;
  if (w != 0.f && c >= 0 && c < 3) {
    const size_t g = Q->goal_per_knot ? (size_t)p * T + k : (size_t)p;
    const float x = c == 0 ? pos.x : (c == 1 ? pos.y : pos.z);
    rollout_cost_add(acc, w, x - Q->goal.pgoal[g * 3 + c]);
  }
}

// After the loop: the lanes' accumulators reduced per term; flags: the rollout's status word (or-reduced).
JDEV void rollout_cost_finish(const JacoRolloutCostArgs* Q, int i, int lane, float acc, unsigned flags) {
  float tx = wave_sum(lane < JRC_LANE_U ? acc : 0.f);
  float tu = wave_sum(lane >= JRC_LANE_U && lane < JRC_LANE_P ? acc : 0.f);
  float tp = wave_sum(lane >= JRC_LANE_P ? acc : 0.f);
  float J = (tu + tx) + tp;
  if (flags & JFLAG_NAN) tu = tx = tp = J = INFINITY;
  if (Q->cost && lane == 0) Q->cost[i] = J;
  if (Q->terms && lane < 3) Q->terms[(size_t)i * 3 + lane] = lane == 0 ? tu : (lane == 1 ? tx : tp);
}

// (the kernel: run_rollout of rollout.h on this block)
#if JACO_TU_HAS(18)
JACO_DEFINE_ENTRY(rollout_cost, JacoRolloutCostArgs, Q.F.R.n, run_rollout)
#else
JACO_DECLARE_ENTRY(rollout_cost, JacoRolloutCostArgs)
#endif
