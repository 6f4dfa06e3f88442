// From the C ABI's arguments to the kernel's argument block, for the thirteen query-style entries (jaco_query, jaco_ik, jaco_osc,
// jaco_osc_task, jaco_joint, jaco_fd, jaco_rollout, jaco_rollout_fb, jaco_lqr, jaco_rollout_cost, jaco_rollout_osc, jaco_transition_fd, jaco_cost_quad).  Host only: included by the library's host unit (jaco_env.hip)
// and by the CPU tests' host build (tests/emu/emu_driver.cpp), after include/jaco_env.h, physics_kernel.h and abi_agreement.h -- the
// public records are copied into the kernel-side records that restate them, which the feature headers (query.h ... rollout_fb.h)
// cannot do: they do not see the public header.  kernels.hip does not include this file.
//
// One function per entry.  Each takes the host copy of the model, the entry's arguments as the caller handed them over (without the
// handle and the stream), the number of envs of the handle and the handle's fp32 state rows, which stand in where no state override is
// given.  Each fills the whole block but its model pointer (the library points it at the device copy, the emulator at the host copy)
// and returns the refusal as jaco_last_error gives it, the entry's name in front; an empty string accepts the call.  What is checked,
// and in which order, is here and in the feature header's jaco_<entry>_resolve, nowhere else.
#pragma once
#include <cstring>
#include <string>

// (jaco_lqr reads no model and no state: its host build for the CPU tests, tests/emu_lqr, sees lqr.h and the public header only and
// defines JACO_ENTRY_ARGS_LQR_ONLY to take this one function)
static inline std::string jaco_lqr_bind(const JacoLqrOptions* opt, int n, const JacoLqrProblem* prob, const JacoLqrOut* out, JacoLqrArgs* Q) {
  *Q = JacoLqrArgs{};
  const std::string why = jaco_lqr_resolve(reinterpret_cast<const JacoLqrOpts*>(opt), n, reinterpret_cast<const JacoLqrProb*>(prob),
                                           reinterpret_cast<const JacoLqrOutp*>(out), Q);
  return why.empty() ? why : "jaco_lqr: " + why;
}

#ifndef JACO_ENTRY_ARGS_LQR_ONLY

static inline std::string jaco_query_bind(const JacoModelDev& m, const JacoFrame* frames, int nframes, const float* qpos, const float* qvel, const JacoQueryOut* out,
                                          int num_envs, const float* state_qpos, const float* state_qvel, JacoQueryArgs* Q) {
  *Q = JacoQueryArgs{};
  const std::string why = jaco_query_resolve(m, reinterpret_cast<const JacoQueryFrame*>(frames), nframes, Q);
  if (!why.empty()) return "jaco_query: " + why;
  Q->qpos = qpos ? qpos : state_qpos;
  Q->qvel = qvel ? qvel : state_qvel;
  if (out) { Q->xpos = out->xpos; Q->xmat = out->xmat; Q->jac = out->jac; Q->qM = out->qM; Q->bias = out->qfrc_bias; }
  Q->nenv = num_envs;
  return why;
}

// (a seed there must be: the caller's, or the state rows)
static inline std::string jaco_ik_bind(const JacoModelDev& m, const JacoFrame* frame, const JacoIkOptions* opt, const float* qpos_seed, const float* target_pos,
                                       const float* target_quat, float* qpos_out, float* resid, int32_t* status, int num_envs, const float* state_qpos,
                                       JacoIkArgs* Q) {
  *Q = JacoIkArgs{};
  if (!frame || !target_pos || !qpos_out || !(qpos_seed || state_qpos)) return "jaco_ik: the frame, the target positions and the output qpos are required";
  const JacoIkOptions defaults = JACO_IK_DEFAULTS;
  memcpy(&Q->fr, frame, sizeof(JacoFrame));
  memcpy(&Q->opt, opt ? opt : &defaults, sizeof(JacoIkOptions));
  if (const char* why = jaco_ik_resolve(m, Q->fr, Q->opt, &Q->active)) return std::string("jaco_ik: ") + why;
  Q->qpos = qpos_seed ? qpos_seed : state_qpos;
  Q->target_pos = target_pos; Q->target_quat = target_quat;
  Q->qpos_out = qpos_out; Q->resid = resid; Q->status = status;
  Q->nenv = num_envs;
  return std::string();
}

static inline JacoOscOpts jaco_osc_options(const JacoOscOptions* opt) {   // NULL: the defaults
  const JacoOscOptions defaults = JACO_OSC_DEFAULTS;
  JacoOscOpts o;
  memcpy(&o, opt ? opt : &defaults, sizeof(JacoOscOptions));
  return o;
}

static inline std::string jaco_osc_bind(const JacoModelDev& m, const JacoFrame* frames, int nframes, const JacoOscOptions* opt, const float* qpos, const float* qvel,
                                        const float* target_pos, const float* target_quat, const float* ctrl_in, float* ctrl_out, int32_t* status, int num_envs,
                                        const float* state_qpos, const float* state_qvel, JacoOscArgs* Q) {
  *Q = JacoOscArgs{};
  Q->target_pos = target_pos; Q->target_quat = target_quat; Q->ctrl_in = ctrl_in; Q->ctrl_out = ctrl_out; Q->status = status;
  const std::string why = jaco_osc_resolve(m, reinterpret_cast<const JacoQueryFrame*>(frames), nframes, jaco_osc_options(opt), Q);
  if (!why.empty()) return "jaco_osc: " + why;
  Q->qpos = qpos ? qpos : state_qpos;
  Q->qvel = qvel ? qvel : state_qvel;
  Q->nenv = num_envs;
  return why;
}

// (the task record is there: an entry handed a NULL one calls jaco_osc's own path instead, block and kernel)
static inline std::string jaco_osc_task_bind(const JacoModelDev& m, const JacoFrame* frames, int nframes, const JacoOscOptions* opt, const JacoOscTask* task,
                                             const float* qpos, const float* qvel, const float* target_pos, const float* target_quat, const float* rest_qpos,
                                             const float* ctrl_in, float* ctrl_out, int32_t* status, int num_envs, const float* state_qpos, const float* state_qvel,
                                             JacoOscTaskArgs* T) {
  *T = JacoOscTaskArgs{};
  JacoOscTaskOpts t;
  memcpy(&t, task, sizeof(JacoOscTask));
  T->o.target_pos = target_pos; T->o.target_quat = target_quat; T->o.ctrl_in = ctrl_in; T->o.ctrl_out = ctrl_out; T->o.status = status;
  T->rest_qpos = rest_qpos;
  const std::string why = jaco_osc_task_resolve(m, reinterpret_cast<const JacoQueryFrame*>(frames), nframes, jaco_osc_options(opt), t, T);
  if (!why.empty()) return "jaco_osc_task: " + why;
  T->o.qpos = qpos ? qpos : state_qpos;
  T->o.qvel = qvel ? qvel : state_qvel;
  T->o.nenv = num_envs;
  return why;
}

static inline std::string jaco_joint_bind(const JacoModelDev& m, const JacoJointOptions* opt, const float* qpos, const float* qvel, const float* target_qpos,
                                          const float* target_qvel, const float* qacc_ff, const float* ctrl_in, float* ctrl_out, int num_envs,
                                          const float* state_qpos, const float* state_qvel, JacoJointArgs* Q) {
  *Q = JacoJointArgs{};
  const JacoJointOptions defaults = JACO_JOINT_DEFAULTS;
  JacoJointOpts o;
  memcpy(&o, opt ? opt : &defaults, sizeof(JacoJointOptions));
  Q->target_qpos = target_qpos; Q->target_qvel = target_qvel; Q->qacc_ff = qacc_ff; Q->ctrl_in = ctrl_in; Q->ctrl_out = ctrl_out;
  const std::string why = jaco_joint_resolve(m, o, Q);
  if (!why.empty()) return "jaco_joint: " + why;
  Q->qpos = qpos ? qpos : state_qpos;
  Q->qvel = qvel ? qvel : state_qvel;
  Q->nenv = num_envs;
  return why;
}

static inline std::string jaco_fd_bind(const JacoModelDev& m, const JacoFdOptions* opt, const float* qpos, const float* qvel, const float* ctrl, const JacoFdOut* out,
                                       int num_envs, const float* state_qpos, const float* state_qvel, JacoFdArgs* Q) {
  *Q = JacoFdArgs{};
  const JacoFdOptions defaults = JACO_FD_DEFAULTS;
  JacoFdOpts o;
  memcpy(&o, opt ? opt : &defaults, sizeof(JacoFdOptions));
  if (out) { Q->qacc = out->qacc; Q->qfrc_smooth = out->qfrc_smooth; Q->dqacc_dqpos = out->dqacc_dqpos; Q->dqacc_dqvel = out->dqacc_dqvel; Q->dqacc_dctrl = out->dqacc_dctrl; }
  const std::string why = jaco_fd_resolve(m, o, out != nullptr, Q);
  if (!why.empty()) return "jaco_fd: " + why;
  Q->qpos = qpos ? qpos : state_qpos;
  Q->qvel = qvel ? qvel : state_qvel;
  Q->ctrl = ctrl;
  Q->nenv = num_envs;
  return why;
}

// (the four rollouts: an accepted call with n = 0 launches nothing, which is the entry's to see to)
static inline std::string jaco_rollout_bind(const JacoModelDev& m, const JacoRolloutOptions* opt, const JacoFrame* frame, int n, const int32_t* state_idx, int nstates,
                                            const float* qpos0, const float* qvel0, const float* ctrl, const JacoRolloutOut* out, int num_envs,
                                            const float* state_qpos, const float* state_qvel, JacoRolloutArgs* Q) {
  *Q = JacoRolloutArgs{};
  Q->state_idx = state_idx; Q->qpos0 = qpos0; Q->qvel0 = qvel0; Q->ctrl = ctrl;
  if (out) { Q->qpos = out->qpos; Q->qvel = out->qvel; Q->xpos = out->xpos; Q->xmat = out->xmat; Q->status = out->status; }
  const std::string why = jaco_rollout_resolve(m, reinterpret_cast<const JacoRolloutOpts*>(opt), reinterpret_cast<const JacoQueryFrame*>(frame), n, nstates, num_envs,
                                               out != nullptr, Q);
  if (!why.empty()) return "jaco_rollout: " + why;
  if (!Q->qpos0) { Q->qpos0 = state_qpos; Q->qvel0 = state_qvel; }
  return why;
}

static inline std::string jaco_rollout_fb_bind(const JacoModelDev& m, const JacoRolloutFbOptions* opt, const JacoFrame* frame, int n, const int32_t* state_idx,
                                               int nstates, const float* qpos0, const float* qvel0, const JacoRolloutPlan* plan, const JacoRolloutFbOut* out,
                                               int num_envs, const float* state_qpos, const float* state_qvel, JacoRolloutFbArgs* Q) {
  *Q = JacoRolloutFbArgs{};
  Q->R.state_idx = state_idx; Q->R.qpos0 = qpos0; Q->R.qvel0 = qvel0;
  if (out) { Q->R.qpos = out->qpos; Q->R.qvel = out->qvel; Q->R.xpos = out->xpos; Q->R.xmat = out->xmat; Q->R.status = out->status; Q->ctrl_out = out->ctrl; }
  const std::string why = jaco_rollout_fb_resolve(m, reinterpret_cast<const JacoRolloutFbOpts*>(opt), reinterpret_cast<const JacoQueryFrame*>(frame), n, nstates,
                                                  num_envs, reinterpret_cast<const JacoRolloutFbPlan*>(plan), out != nullptr, Q);
  if (!why.empty()) return "jaco_rollout_fb: " + why;
  if (!Q->R.qpos0) { Q->R.qpos0 = state_qpos; Q->R.qvel0 = state_qvel; }
  return why;
}

static inline std::string jaco_rollout_cost_bind(const JacoModelDev& m, const JacoRolloutCostOptions* opt, const JacoFrame* frame, int n, const int32_t* state_idx,
                                                 int nstates, const float* qpos0, const float* qvel0, const JacoRolloutPlan* plan, const JacoRolloutGoal* goal,
                                                 const JacoRolloutCostOut* out, int num_envs, const float* state_qpos, const float* state_qvel,
                                                 JacoRolloutCostArgs* Q) {
  *Q = JacoRolloutCostArgs{};
  JacoRolloutArgs& R = Q->F.R;
  R.state_idx = state_idx; R.qpos0 = qpos0; R.qvel0 = qvel0;
  if (out) {
    R.qpos = out->qpos; R.qvel = out->qvel; R.xpos = out->xpos; R.xmat = out->xmat; R.status = out->status; Q->F.ctrl_out = out->ctrl;
    Q->cost = out->cost; Q->terms = out->terms;
  }
  const std::string why = jaco_rollout_cost_resolve(m, reinterpret_cast<const JacoRolloutCostOpts*>(opt), reinterpret_cast<const JacoQueryFrame*>(frame), n, nstates,
                                                    num_envs, reinterpret_cast<const JacoRolloutFbPlan*>(plan), reinterpret_cast<const JacoRolloutCostGoal*>(goal),
                                                    out != nullptr, Q);
  if (!why.empty()) return "jaco_rollout_cost: " + why;
  if (!R.qpos0) { R.qpos0 = state_qpos; R.qvel0 = state_qvel; }
  return why;
}

static inline std::string jaco_rollout_osc_bind(const JacoModelDev& m, const JacoRolloutOscOptions* opt, const JacoFrame* frames, int nframes, const JacoFrame* out_frame,
                                                int n, const int32_t* state_idx, int nstates, const float* qpos0, const float* qvel0, const JacoRolloutOscPlan* plan,
                                                const JacoRolloutFbOut* out, int num_envs, const float* state_qpos, const float* state_qvel, JacoRolloutOscArgs* Q) {
  *Q = JacoRolloutOscArgs{};
  Q->R.state_idx = state_idx; Q->R.qpos0 = qpos0; Q->R.qvel0 = qvel0;
  if (out) { Q->R.qpos = out->qpos; Q->R.qvel = out->qvel; Q->R.xpos = out->xpos; Q->R.xmat = out->xmat; Q->R.status = out->status; Q->O.ctrl_out = out->ctrl; }
  const std::string why = jaco_rollout_osc_resolve(m, reinterpret_cast<const JacoRolloutOscOpts*>(opt), reinterpret_cast<const JacoQueryFrame*>(frames), nframes,
                                                   reinterpret_cast<const JacoQueryFrame*>(out_frame), n, nstates, num_envs,
                                                   reinterpret_cast<const JacoRolloutOscTargets*>(plan), out != nullptr, Q);
  if (!why.empty()) return "jaco_rollout_osc: " + why;
  if (!Q->R.qpos0) { Q->R.qpos0 = state_qpos; Q->R.qvel0 = state_qvel; }
  return why;
}
// (n pairs, not tied to num_envs; an accepted call with n = 0 launches nothing, which is the entry's to see to)
static inline std::string jaco_transition_bind(const JacoModelDev& m, const JacoTransitionOptions* opt, int n, const float* qpos, const float* qvel, const float* ctrl,
                                               const JacoTransitionOut* out, int num_envs, const float* state_qpos, const float* state_qvel, JacoTransitionArgs* Q) {
  *Q = JacoTransitionArgs{};
  Q->qpos = qpos; Q->qvel = qvel; Q->ctrl = ctrl;
  if (out) { Q->A = out->A; Q->B = out->B; Q->next_qpos = out->next_qpos; Q->next_qvel = out->next_qvel; Q->status = out->status; }
  const std::string why = jaco_transition_resolve(m, reinterpret_cast<const JacoTransitionOpts*>(opt), n, num_envs, out != nullptr, Q);
  if (!why.empty()) return "jaco_transition_fd: " + why;
  if (!Q->qpos) { Q->qpos = state_qpos; Q->qvel = state_qvel; }
  return why;
}
// (R trajectories of opt->nknots knots, not tied to num_envs and reading nothing of a handle; R = 0 launches nothing, the entry's to see to)
static inline std::string jaco_cost_quad_bind(const JacoModelDev& m, const JacoCostQuadOptions* opt, const JacoFrame* frame, int R, const float* qpos, const float* qvel,
                                              const float* ctrl, const JacoCostQuadGoal* goal, const JacoCostQuadOut* out, JacoCostQuadArgs* Q) {
  *Q = JacoCostQuadArgs{};
  Q->qpos = qpos; Q->qvel = qvel; Q->ctrl = ctrl;
  if (out) Q->out = *reinterpret_cast<const JacoCostQuadOutp*>(out);
  const std::string why = jaco_cost_quad_resolve(m, reinterpret_cast<const JacoCostQuadOpts*>(opt), reinterpret_cast<const JacoQueryFrame*>(frame), R,
                                                 reinterpret_cast<const JacoCostQuadGoals*>(goal), out != nullptr, Q);
  return why.empty() ? why : "jaco_cost_quad: " + why;
}
#endif   // JACO_ENTRY_ARGS_LQR_ONLY
