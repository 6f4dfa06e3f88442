// The agreement between the public header (include/jaco_env.h) and the kernel-side records and constants that restate it, field by
// field.  Include it after both sides: jaco_env.h, physics_kernel.h (with query.h, ik.h, osc.h, osc_task.h, joint.h, fd.h, rollout.h, rollout_fb.h, lqr.h, rollout_cost.h, rollout_osc.h, transition.h and cost_quad.h) and snapshot.h.  The library's host unit
// (jaco_env.hip) and the CPU tests' host build (tests/emu/emu_driver.cpp) both do.
#pragma once
#include <cstddef>

static_assert(JFLAG_CON_OVERFLOW == JACO_FLAG_CON_OVERFLOW && JFLAG_EFC_OVERFLOW == JACO_FLAG_EFC_OVERFLOW &&
                  JFLAG_CAND_OVERFLOW == JACO_FLAG_CAND_OVERFLOW && JFLAG_NAN == JACO_FLAG_NAN &&
                  JFLAG_SOLVER_MAXITER == JACO_FLAG_SOLVER_MAXITER && JFLAG_HEAVY_TIER == JACO_FLAG_HEAVY_TIER,
              "flag bits of the kernel and the public header must agree");
static_assert(JSNAP_FLAG_BAD == JACO_FLAG_BAD_SNAPSHOT, "flag bit of snapshot.h and the public header must agree");
static_assert(sizeof(JacoContact) == sizeof(JacoContactRec) && offsetof(JacoContact, force) == offsetof(JacoContactRec, force) &&
                  offsetof(JacoContact, geom) == offsetof(JacoContactRec, geom) && offsetof(JacoContact, dim) == offsetof(JacoContactRec, dim) &&
                  JACO_CONTACT_MAX_CAPACITY == JCONREC_MAX_CAPACITY,
              "JacoContact (include/jaco_env.h) and JacoContactRec (physics_kernel.h) disagree");
static_assert(sizeof(JacoFrame) == sizeof(JacoQueryFrame) && offsetof(JacoFrame, pos) == offsetof(JacoQueryFrame, pos) &&
                  offsetof(JacoFrame, mat) == offsetof(JacoQueryFrame, mat) && offsetof(JacoFrame, point) == offsetof(JacoQueryFrame, point) &&
                  JACO_QUERY_MAX_FRAMES == JQ_MAXFRAMES, "JacoFrame of the public header and the kernel's frame record must agree");
static_assert(sizeof(JacoIkOptions) == sizeof(JacoIkOpts) && offsetof(JacoIkOptions, tol_pos) == offsetof(JacoIkOpts, tol_pos) &&
                  offsetof(JacoIkOptions, tol_rot) == offsetof(JacoIkOpts, tol_rot) && offsetof(JacoIkOptions, damping) == offsetof(JacoIkOpts, damping) &&
                  offsetof(JacoIkOptions, max_step) == offsetof(JacoIkOpts, max_step) && offsetof(JacoIkOptions, max_iters) == offsetof(JacoIkOpts, max_iters) &&
                  offsetof(JacoIkOptions, dof_mask) == offsetof(JacoIkOpts, dof_mask) && JACO_IK_MAX_ITERS == JIK_MAX_ITERS,
              "JacoIkOptions of the public header and the kernel's option record must agree");
static_assert(sizeof(JacoOscOptions) == sizeof(JacoOscOpts) && offsetof(JacoOscOptions, kp) == offsetof(JacoOscOpts, kp) &&
                  offsetof(JacoOscOptions, ko) == offsetof(JacoOscOpts, ko) && offsetof(JacoOscOptions, kv) == offsetof(JacoOscOpts, kv) &&
                  offsetof(JacoOscOptions, vmax_xyz) == offsetof(JacoOscOpts, vmax_xyz) && offsetof(JacoOscOptions, vmax_abg) == offsetof(JacoOscOpts, vmax_abg) &&
                  offsetof(JacoOscOptions, dof_mask) == offsetof(JacoOscOpts, dof_mask) && JACO_OSC_MAX_FRAMES == JOSC_MAXFRAMES,
              "JacoOscOptions of the public header and the kernel's option record must agree");
static_assert(sizeof(JacoOscTask) == sizeof(JacoOscTaskOpts) && offsetof(JacoOscTask, axes) == offsetof(JacoOscTaskOpts, axes) &&
                  offsetof(JacoOscTask, null_kv) == offsetof(JacoOscTaskOpts, null_kv) && offsetof(JacoOscTask, rest_kp) == offsetof(JacoOscTaskOpts, rest_kp) &&
                  offsetof(JacoOscTask, rest_kv) == offsetof(JacoOscTaskOpts, rest_kv) && offsetof(JacoOscTask, rest_mask) == offsetof(JacoOscTaskOpts, rest_mask),
              "JacoOscTask of the public header and the kernel's task record must agree");
static_assert(sizeof(JacoJointOptions) == sizeof(JacoJointOpts) && offsetof(JacoJointOptions, kp) == offsetof(JacoJointOpts, kp) &&
                  offsetof(JacoJointOptions, kv) == offsetof(JacoJointOpts, kv) && offsetof(JacoJointOptions, vmax) == offsetof(JacoJointOpts, vmax) &&
                  offsetof(JacoJointOptions, dof_mask) == offsetof(JacoJointOpts, dof_mask),
              "JacoJointOptions of the public header and the kernel's option record must agree");
static_assert(sizeof(JacoFdOptions) == sizeof(JacoFdOpts) && offsetof(JacoFdOptions, eps_qpos) == offsetof(JacoFdOpts, eps_qpos) &&
                  offsetof(JacoFdOptions, eps_qvel) == offsetof(JacoFdOpts, eps_qvel) && offsetof(JacoFdOptions, implicit_damping) == offsetof(JacoFdOpts, implicit_damping) &&
                  offsetof(JacoFdOptions, dof_mask) == offsetof(JacoFdOpts, dof_mask),
              "JacoFdOptions of the public header and the kernel's option record must agree");
static_assert(sizeof(JacoRolloutOptions) == sizeof(JacoRolloutOpts) && offsetof(JacoRolloutOptions, nknots) == offsetof(JacoRolloutOpts, nknots) &&
                  offsetof(JacoRolloutOptions, hold) == offsetof(JacoRolloutOpts, hold) && offsetof(JacoRolloutOptions, final_only) == offsetof(JacoRolloutOpts, final_only) &&
                  JACO_ROLLOUT_MAX_SUBSTEPS == JROLLOUT_MAX_SUBSTEPS && JACO_ROLLOUT_BAD_INDEX == JROLLOUT_BAD_INDEX,
              "JacoRolloutOptions of the public header and the kernel's option record must agree");
static_assert(sizeof(JacoRolloutFbOptions) == sizeof(JacoRolloutFbOpts) && offsetof(JacoRolloutFbOptions, nknots) == offsetof(JacoRolloutFbOpts, nknots) &&
                  offsetof(JacoRolloutFbOptions, hold) == offsetof(JacoRolloutFbOpts, hold) && offsetof(JacoRolloutFbOptions, final_only) == offsetof(JacoRolloutFbOpts, final_only) &&
                  offsetof(JacoRolloutFbOptions, per_substep) == offsetof(JacoRolloutFbOpts, per_substep) && offsetof(JacoRolloutFbOptions, ndofs) == offsetof(JacoRolloutFbOpts, ndofs) &&
                  offsetof(JacoRolloutFbOptions, dofs) == offsetof(JacoRolloutFbOpts, dofs) && JACO_ROLLOUT_FB_MAX_DOFS == JROLLOUT_FB_MAX_DOFS,
              "JacoRolloutFbOptions of the public header and the kernel's option record must agree");
static_assert(sizeof(JacoRolloutPlan) == sizeof(JacoRolloutFbPlan) && offsetof(JacoRolloutPlan, ctrl) == offsetof(JacoRolloutFbPlan, ctrl) &&
                  offsetof(JacoRolloutPlan, kff) == offsetof(JacoRolloutFbPlan, kff) && offsetof(JacoRolloutPlan, gain) == offsetof(JacoRolloutFbPlan, gain) &&
                  offsetof(JacoRolloutPlan, xref) == offsetof(JacoRolloutFbPlan, xref) && offsetof(JacoRolloutPlan, alpha) == offsetof(JacoRolloutFbPlan, alpha) &&
                  offsetof(JacoRolloutPlan, plan_idx) == offsetof(JacoRolloutFbPlan, plan_idx) && offsetof(JacoRolloutPlan, nplans) == offsetof(JacoRolloutFbPlan, nplans),
              "JacoRolloutPlan of the public header and the kernel's plan record must agree");
static_assert(sizeof(JacoLqrOptions) == sizeof(JacoLqrOpts) && offsetof(JacoLqrOptions, nknots) == offsetof(JacoLqrOpts, nknots) &&
                  offsetof(JacoLqrOptions, nx) == offsetof(JacoLqrOpts, nx) && offsetof(JacoLqrOptions, nu) == offsetof(JacoLqrOpts, nu) &&
                  offsetof(JacoLqrOptions, rows_out) == offsetof(JacoLqrOpts, rows_out) && offsetof(JacoLqrOptions, row) == offsetof(JacoLqrOpts, row) &&
                  offsetof(JacoLqrOptions, shared_knots) == offsetof(JacoLqrOpts, shared_knots) &&
                  offsetof(JacoLqrOptions, shared_probs) == offsetof(JacoLqrOpts, shared_probs) && JACO_LQR_MAX_NX == JLQR_MAX_NX &&
                  JACO_LQR_MAX_NU == JLQR_MAX_NU && JACO_LQR_MAX_NX == 2 * JACO_ROLLOUT_FB_MAX_DOFS && JACO_ROLLOUT_MAX_SUBSTEPS == JLQR_MAX_KNOTS &&
                  JACO_LQR_BAD_INDEX == JLQR_BAD_INDEX && JACO_LQR_BAD_INDEX == JACO_ROLLOUT_BAD_INDEX && JACO_LQR_NOT_PD == JLQR_NOT_PD &&
                  JACO_LQR_LXX == JLQR_LXX && JACO_LQR_LUU == JLQR_LUU && JACO_LQR_LUX == JLQR_LUX && JACO_LQR_LX == JLQR_LX &&
                  JACO_LQR_LU == JLQR_LU && JACO_LQR_VXX == JLQR_VXX && JACO_LQR_VX == JLQR_VX,
              "JacoLqrOptions of the public header and the kernel's option record must agree");
static_assert(sizeof(JacoLqrProblem) == sizeof(JacoLqrProb) && offsetof(JacoLqrProblem, A) == offsetof(JacoLqrProb, A) &&
                  offsetof(JacoLqrProblem, B) == offsetof(JacoLqrProb, B) && offsetof(JacoLqrProblem, lxx) == offsetof(JacoLqrProb, lxx) &&
                  offsetof(JacoLqrProblem, luu) == offsetof(JacoLqrProb, luu) && offsetof(JacoLqrProblem, lux) == offsetof(JacoLqrProb, lux) &&
                  offsetof(JacoLqrProblem, lx) == offsetof(JacoLqrProb, lx) && offsetof(JacoLqrProblem, lu) == offsetof(JacoLqrProb, lu) &&
                  offsetof(JacoLqrProblem, Vxx) == offsetof(JacoLqrProb, Vxx) && offsetof(JacoLqrProblem, Vx) == offsetof(JacoLqrProb, Vx) &&
                  offsetof(JacoLqrProblem, mu) == offsetof(JacoLqrProb, mu) && offsetof(JacoLqrProblem, prob_idx) == offsetof(JacoLqrProb, prob_idx) &&
                  offsetof(JacoLqrProblem, nprob) == offsetof(JacoLqrProb, nprob),
              "JacoLqrProblem of the public header and the kernel's problem record must agree");
static_assert(sizeof(JacoLqrOut) == sizeof(JacoLqrOutp) && offsetof(JacoLqrOut, gain) == offsetof(JacoLqrOutp, gain) &&
                  offsetof(JacoLqrOut, kff) == offsetof(JacoLqrOutp, kff) && offsetof(JacoLqrOut, dV) == offsetof(JacoLqrOutp, dV) &&
                  offsetof(JacoLqrOut, Vxx0) == offsetof(JacoLqrOutp, Vxx0) && offsetof(JacoLqrOut, Vx0) == offsetof(JacoLqrOutp, Vx0) &&
                  offsetof(JacoLqrOut, status) == offsetof(JacoLqrOutp, status),
              "JacoLqrOut of the public header and the kernel's output record must agree");
static_assert(sizeof(JacoRolloutCostOptions) == sizeof(JacoRolloutCostOpts) && offsetof(JacoRolloutCostOptions, nknots) == offsetof(JacoRolloutCostOpts, nknots) &&
                  offsetof(JacoRolloutCostOptions, hold) == offsetof(JacoRolloutCostOpts, hold) && offsetof(JacoRolloutCostOptions, final_only) == offsetof(JacoRolloutCostOpts, final_only) &&
                  offsetof(JacoRolloutCostOptions, goal_per_knot) == offsetof(JacoRolloutCostOpts, goal_per_knot) && offsetof(JacoRolloutCostOptions, ndofs) == offsetof(JacoRolloutCostOpts, ndofs) &&
                  offsetof(JacoRolloutCostOptions, dofs) == offsetof(JacoRolloutCostOpts, dofs) && offsetof(JacoRolloutCostOptions, wx) == offsetof(JacoRolloutCostOpts, wx) &&
                  offsetof(JacoRolloutCostOptions, wxT) == offsetof(JacoRolloutCostOpts, wxT) && offsetof(JacoRolloutCostOptions, wu) == offsetof(JacoRolloutCostOpts, wu) &&
                  offsetof(JacoRolloutCostOptions, wp) == offsetof(JacoRolloutCostOpts, wp) && offsetof(JacoRolloutCostOptions, wpT) == offsetof(JacoRolloutCostOpts, wpT) &&
                  JACO_ROLLOUT_COST_MAX_NU == JROLLOUT_COST_MAX_NU && 2 * JACO_ROLLOUT_FB_MAX_DOFS == JRC_NX,
              "JacoRolloutCostOptions of the public header and the kernel's option record must agree");
static_assert(sizeof(JacoRolloutGoal) == sizeof(JacoRolloutCostGoal) && offsetof(JacoRolloutGoal, noise) == offsetof(JacoRolloutCostGoal, noise) &&
                  offsetof(JacoRolloutGoal, xgoal) == offsetof(JacoRolloutCostGoal, xgoal) && offsetof(JacoRolloutGoal, pgoal) == offsetof(JacoRolloutCostGoal, pgoal),
              "JacoRolloutGoal of the public header and the kernel's goal record must agree");
static_assert(offsetof(JacoRolloutCostOut, qpos) == offsetof(JacoRolloutFbOut, qpos) && offsetof(JacoRolloutCostOut, status) == offsetof(JacoRolloutFbOut, status) &&
                  offsetof(JacoRolloutCostOut, ctrl) == offsetof(JacoRolloutFbOut, ctrl) && offsetof(JacoRolloutCostOut, cost) == sizeof(JacoRolloutFbOut) &&
                  offsetof(JacoRolloutCostOut, terms) == sizeof(JacoRolloutFbOut) + sizeof(float*) && offsetof(JacoRolloutCostArgs, F) == 0,
              "JacoRolloutCostOut extends JacoRolloutFbOut; the costed kernel's block starts with the closed-loop kernel's");
static_assert(sizeof(JacoRolloutOscOptions) == sizeof(JacoRolloutOscOpts) && offsetof(JacoRolloutOscOptions, nknots) == offsetof(JacoRolloutOscOpts, nknots) &&
                  offsetof(JacoRolloutOscOptions, hold) == offsetof(JacoRolloutOscOpts, hold) && offsetof(JacoRolloutOscOptions, final_only) == offsetof(JacoRolloutOscOpts, final_only) &&
                  offsetof(JacoRolloutOscOptions, per_substep) == offsetof(JacoRolloutOscOpts, per_substep) && offsetof(JacoRolloutOscOptions, nframes) == offsetof(JacoRolloutOscOpts, nframes) &&
                  offsetof(JacoRolloutOscOptions, kp) == offsetof(JacoRolloutOscOpts, kp) && offsetof(JacoRolloutOscOptions, ko) == offsetof(JacoRolloutOscOpts, ko) &&
                  offsetof(JacoRolloutOscOptions, kv) == offsetof(JacoRolloutOscOpts, kv) && offsetof(JacoRolloutOscOptions, vmax_xyz) == offsetof(JacoRolloutOscOpts, vmax_xyz) &&
                  offsetof(JacoRolloutOscOptions, vmax_abg) == offsetof(JacoRolloutOscOpts, vmax_abg) && offsetof(JacoRolloutOscOptions, dof_mask) == offsetof(JacoRolloutOscOpts, dof_mask),
              "JacoRolloutOscOptions of the public header and the kernel's option record must agree");
static_assert(sizeof(JacoRolloutOscPlan) == sizeof(JacoRolloutOscTargets) && offsetof(JacoRolloutOscPlan, ctrl) == offsetof(JacoRolloutOscTargets, ctrl) &&
                  offsetof(JacoRolloutOscPlan, target_pos) == offsetof(JacoRolloutOscTargets, target_pos) &&
                  offsetof(JacoRolloutOscPlan, target_quat) == offsetof(JacoRolloutOscTargets, target_quat) &&
                  offsetof(JacoRolloutOscPlan, plan_idx) == offsetof(JacoRolloutOscTargets, plan_idx) && offsetof(JacoRolloutOscPlan, nplans) == offsetof(JacoRolloutOscTargets, nplans),
              "JacoRolloutOscPlan of the public header and the kernel's plan record must agree");
static_assert(JACO_ROLLOUT_OSC_SINGULAR0 == JROLLOUT_OSC_SINGULAR0 && JACO_ROLLOUT_OSC_SINGULAR1 == (JROLLOUT_OSC_SINGULAR0 << 1) && JACO_OSC_MAX_FRAMES == 2 &&
                  (JACO_ROLLOUT_OSC_SINGULAR0 & (JACO_ROLLOUT_BAD_INDEX | JACO_FLAG_NAN | JACO_FLAG_SOLVER_MAXITER)) == 0 && offsetof(JacoRolloutOscArgs, R) == 0,
              "the singular bits of the public header and rollout_osc.h must agree and lie clear of the rollout's other status bits");
static_assert(sizeof(JacoTransitionOptions) == sizeof(JacoTransitionOpts) && offsetof(JacoTransitionOptions, hold) == offsetof(JacoTransitionOpts, hold) &&
                  offsetof(JacoTransitionOptions, centered) == offsetof(JacoTransitionOpts, centered) && offsetof(JacoTransitionOptions, groups) == offsetof(JacoTransitionOpts, groups) &&
                  offsetof(JacoTransitionOptions, ndofs) == offsetof(JacoTransitionOpts, ndofs) && offsetof(JacoTransitionOptions, dofs) == offsetof(JacoTransitionOpts, dofs) &&
                  offsetof(JacoTransitionOptions, nacts) == offsetof(JacoTransitionOpts, nacts) && offsetof(JacoTransitionOptions, acts) == offsetof(JacoTransitionOpts, acts) &&
                  offsetof(JacoTransitionOptions, eps_qpos) == offsetof(JacoTransitionOpts, eps_qpos) && offsetof(JacoTransitionOptions, eps_qvel) == offsetof(JacoTransitionOpts, eps_qvel) &&
                  offsetof(JacoTransitionOptions, eps_ctrl) == offsetof(JacoTransitionOpts, eps_ctrl) && JACO_TRANSITION_MAX_HOLD == JTRANSITION_MAX_HOLD,
              "JacoTransitionOptions of the public header and the kernel's option record must agree");
static_assert(sizeof(JacoTransitionOut) == sizeof(JacoTransitionOutp) && offsetof(JacoTransitionOut, A) == offsetof(JacoTransitionOutp, A) &&
                  offsetof(JacoTransitionOut, B) == offsetof(JacoTransitionOutp, B) && offsetof(JacoTransitionOut, next_qpos) == offsetof(JacoTransitionOutp, next_qpos) &&
                  offsetof(JacoTransitionOut, next_qvel) == offsetof(JacoTransitionOutp, next_qvel) && offsetof(JacoTransitionOut, status) == offsetof(JacoTransitionOutp, status),
              "JacoTransitionOut of the public header and the kernel's output record must agree");
#define JACO_ABI_SAME(A, B, f) (offsetof(A, f) == offsetof(B, f))
static_assert(sizeof(JacoCostQuadOptions) == sizeof(JacoCostQuadOpts) && JACO_ABI_SAME(JacoCostQuadOptions, JacoCostQuadOpts, nknots) &&
                  JACO_ABI_SAME(JacoCostQuadOptions, JacoCostQuadOpts, goal_per_knot) && JACO_ABI_SAME(JacoCostQuadOptions, JacoCostQuadOpts, ndofs) &&
                  JACO_ABI_SAME(JacoCostQuadOptions, JacoCostQuadOpts, dofs) && JACO_ABI_SAME(JacoCostQuadOptions, JacoCostQuadOpts, nacts) &&
                  JACO_ABI_SAME(JacoCostQuadOptions, JacoCostQuadOpts, acts) && JACO_ABI_SAME(JacoCostQuadOptions, JacoCostQuadOpts, wx) &&
                  JACO_ABI_SAME(JacoCostQuadOptions, JacoCostQuadOpts, wxT) && JACO_ABI_SAME(JacoCostQuadOptions, JacoCostQuadOpts, wu) &&
                  JACO_ABI_SAME(JacoCostQuadOptions, JacoCostQuadOpts, wp) && JACO_ABI_SAME(JacoCostQuadOptions, JacoCostQuadOpts, wpT),
              "JacoCostQuadOptions of the public header and the kernel's option record must agree");
static_assert(sizeof(JacoCostQuadGoal) == sizeof(JacoCostQuadGoals) && JACO_ABI_SAME(JacoCostQuadGoal, JacoCostQuadGoals, xgoal) &&
                  JACO_ABI_SAME(JacoCostQuadGoal, JacoCostQuadGoals, pgoal) && JACO_ABI_SAME(JacoCostQuadGoal, JacoCostQuadGoals, goal_idx) &&
                  JACO_ABI_SAME(JacoCostQuadGoal, JacoCostQuadGoals, ngoals),
              "JacoCostQuadGoal of the public header and the kernel's goal record must agree");
static_assert(sizeof(JacoCostQuadOut) == sizeof(JacoCostQuadOutp) && JACO_ABI_SAME(JacoCostQuadOut, JacoCostQuadOutp, lx) && JACO_ABI_SAME(JacoCostQuadOut, JacoCostQuadOutp, lxx) &&
                  JACO_ABI_SAME(JacoCostQuadOut, JacoCostQuadOutp, lu) && JACO_ABI_SAME(JacoCostQuadOut, JacoCostQuadOutp, Vx) && JACO_ABI_SAME(JacoCostQuadOut, JacoCostQuadOutp, Vxx) &&
                  JACO_ABI_SAME(JacoCostQuadOut, JacoCostQuadOutp, l) && JACO_ABI_SAME(JacoCostQuadOut, JacoCostQuadOutp, status),
              "JacoCostQuadOut of the public header and the kernel's output record must agree");
#undef JACO_ABI_SAME
