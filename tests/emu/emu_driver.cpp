// TEST INFRASTRUCTURE: runs the unmodified kernel source under the lockstep wavefront emulator.
// Built by tests/emu/Makefile into every libjaco_emu*.so; used by CPU-side (-m "not gpu") kernel checks: ctrl-level steps (with the
// contact record of jaco_set_contact_record, or with the low words a handle keeps), env-level calls, the ten query-style entries that read
// the model (jaco_query, jaco_ik, jaco_osc, jaco_osc_task, jaco_joint, jaco_fd, jaco_rollout, jaco_rollout_fb, jaco_rollout_cost,
// jaco_rollout_osc) and the host build of the env snapshots (jaco_save_envs / jaco_load_envs).  The argument checks and the reset of one env are the library's own host halves
// (entry_args.h over query.h ... rollout_osc.h, physics_kernel.h, env_logic.h, model_blob.cpp), called here as jaco_env.hip calls them.
#include <algorithm>
#include <cstdio>
#include <functional>
#include <string>
#include <vector>

#include "../../include/jaco_env.h"
#include "../../mujoco_jaco_amd/csrc/model_blob.h"
#include "../../mujoco_jaco_amd/csrc/physics_kernel.h"
#include "../../mujoco_jaco_amd/csrc/snapshot.h"
#include "../../mujoco_jaco_amd/csrc/abi_agreement.h"
#include "../../mujoco_jaco_amd/csrc/entry_args.h"

void emu_run_wave(int block, std::function<void()> body);

extern "C" int emu_dbg_size() { return JDBG_SIZE; }
extern "C" int emu_lds_bytes() { return (int)sizeof(JacoLDS<JacoLight>); }
extern "C" int emu_lds_bytes_heavy() { return (int)sizeof(JacoLDS<JacoHeavy>); }
extern "C" int emu_lds_bytes_medium() { return (int)sizeof(JacoLDS<JacoMedium>); }
extern "C" int emu_lds_bytes_huge() { return (int)sizeof(JacoLDS<JacoHuge>); }
extern "C" int emu_query_lds_bytes() { return (int)sizeof(JacoLDS<JacoArm>); }
extern "C" int emu_contact_words() { return (int)(sizeof(JacoContact) / 4); }
extern "C" int emu_task_floats() { return JTASK_N; }
extern "C" int emu_cache_floats() { return JCACHE_N; }
extern "C" int emu_task_nact(int task_id) { return jaco_task_nact(task_id); }   // width of the task's action row (jaco_dims)

// the message of the last refusal (JACO_EINVAL from an argument check, -1 from the model loader): the text jaco_last_error gives
static std::string g_error;
extern "C" const char* emu_last_error() { return g_error.c_str(); }
static int refuse(const std::string& why) { g_error = why; return JACO_EINVAL; }

// the model of the last call: every entry loads its blob into it (the loader starts from a zeroed model and a fresh hull table)
static JacoModelDev g_model;
static std::vector<float> g_hull, g_qpos0;
static int g_mpr_output = -1;   // -1: the model loader's default
extern "C" void emu_set_mpr_output(int v) { g_mpr_output = v; }
static int load_model(const void* blob, long blob_size) {
  if (jaco_model_from_blob(blob, (size_t)blob_size, &g_model, &g_hull, &g_error, &g_qpos0)) return -1;
  if (g_mpr_output >= 0) g_model.mpr_output = g_mpr_output;
  return 0;
}

static std::vector<int> g_hint;
static int g_use_hints = 0;
static int g_obs_mode = 0;
extern "C" void emu_set_obs_mode(int v) { g_obs_mode = v; }
extern "C" void emu_set_hints(int on) { g_use_hints = on; }
long emu_counter[16] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};   // (8: constrained Newton solves, 9: their Hessian builds = matrix-core passes)
extern "C" long emu_get_counter(int i, int reset) { long v = emu_counter[i & 15]; if (reset) emu_counter[i & 15] = 0; return v; }
static int g_no_pairlist = 0;
static std::vector<float> g_terminal;
extern "C" const float* emu_last_terminal() { return g_terminal.data(); }   // [nenv][2] (success, wb) latched by terminal steps
static int g_sep_cache = 1;
static std::vector<float> g_sepdir;
extern "C" void emu_set_sep_cache(int on) { g_sep_cache = on; g_sepdir.clear(); }   // 0: every hull pair goes through MPR (option "sep_cache" = 0); either call empties the cache
static int g_mpr_pairs = 1;
extern "C" void emu_set_mpr_pairs(int on) { g_mpr_pairs = on; }   // option "mpr_pairs" of the library (counter 10: passes of the two-pair routine)
extern "C" void emu_set_pair_list(int on) { g_no_pairlist = !on; }   // 0: every pair tested in every substep (option "pair_list" = 0 of the library)
static int g_handdown = 0, g_handed_down = 0;
extern "C" void emu_set_handdown(int on) { g_handdown = on; }
extern "C" int emu_handed_down() { return g_handed_down; }   // envs passed from the heavy drain to the second medium drain so far
static int g_no_tier_return = 0;
extern "C" void emu_set_tier_return(int on) { g_no_tier_return = !on; }
static int emu_launch(JacoStepArgs A, int* heavy_envs) {
  A.no_tier_return = g_no_tier_return;
  A.no_pairlist = g_no_pairlist;
  A.mpr_pairs = g_mpr_pairs;
  if (g_sepdir.size() != (size_t)A.nenv * JMAXPAIR * 4) g_sepdir.assign((size_t)A.nenv * JMAXPAIR * 4, 0.f);
  A.sepdir = g_sep_cache ? g_sepdir.data() : nullptr;
  if (g_terminal.size() != (size_t)A.nenv * 2) g_terminal.assign((size_t)A.nenv * 2, 0.f);
  A.terminal = g_terminal.data();
  A.terminal_obs = nullptr;
  A.obs_mode = g_obs_mode;
  std::vector<int> remaining(A.nenv, 0), lists(6 * (size_t)A.nenv, -1);
  int count[3] = {0, 0, 0}, taken[3] = {0, 0, 0}, light_left = A.nenv;
  A.remaining = remaining.data(); A.light_left = &light_left;
  for (int t = 0; t < 3; t++) { A.q[t].list = lists.data() + (size_t)t * 2 * A.nenv; A.q[t].count = &count[t]; A.q[t].taken = &taken[t]; A.q[t].limit = nullptr; A.q[t].reserve = nullptr; }
  A.routed_mark = nullptr; A.launch_id = 1; A.nslots = nullptr;
  if ((int)g_hint.size() != A.nenv) g_hint.assign(A.nenv, 0);
  A.hint = g_use_hints ? g_hint.data() : nullptr; A.hint_mode = g_use_hints;
  emu_grid = A.nenv;
  // (as jaco_env.hip: the step kernel proper serves the real steps (JM_REAL_STEP), every other mode the full-code twin)
  // ... and contact-free steps (disable_contact, models without a collidable pair) the lean kernel, alone
  if ((A.disable_contact || A.model->npair == 0) && JM_REAL_STEP(A.env_mode)) {
    A.disable_contact = 1; A.hint = nullptr;
    for (int e = 0; e < A.nenv; e++) emu_run_wave(e, [&]() { jaco_physics_kernel_arm(A); });
    if (heavy_envs) *heavy_envs = 0;
    return 0;
  }
  for (int e = 0; e < A.nenv; e++) emu_run_wave(e, [&]() { if (!JM_REAL_STEP(A.env_mode)) jaco_physics_kernel_listed(A); else jaco_physics_kernel(A); });
  emu_grid = 1;
  // (the resident workers of the GPU build leave as soon as the light grid is done: here that is always the case, so the
  // drains serve every queue; they are the same serve functions).  Same launch sequence as jaco_env.hip, grids of one workgroup.
  if (count[0] > 0) emu_run_wave(0, [&]() { jaco_physics_kernel_medium(A); });
  emu_run_wave(0, [&]() { jaco_physics_kernel_medium_drain(A); });
  if (count[1] > 0) emu_run_wave(0, [&]() { jaco_physics_kernel_heavy_workers(A); });
  if (g_handdown && A.env_mode == JM_STEP) {
    A.handdown = 1;
    emu_run_wave(0, [&]() { jaco_physics_kernel_heavy_drain(A); });
    A.handdown = 0;
    taken[0] -= 1; taken[1] -= 1;   // (jaco_drain_round2_kernel: each drain workgroup ends one claim beyond the end)
    g_handed_down += count[0] - taken[0];
    emu_run_wave(0, [&]() { jaco_physics_kernel_medium_drain(A); });
  }
  emu_run_wave(0, [&]() { jaco_physics_kernel_heavy_drain(A); });
  if (count[2] > 0) emu_run_wave(0, [&]() { jaco_physics_kernel_huge_workers(A); });
  emu_run_wave(0, [&]() { jaco_physics_kernel_huge_drain(A); });
  if (heavy_envs) *heavy_envs = count[0];
  return 0;
}
// env-level call (mode: JacoMode): JM_STEP = step (nsub = frame_skip), JM_FORWARD = forward only (nsub = 1), JM_HOLD / JM_PREREACH = resets
static int g_auto_reset = 0;
extern "C" void emu_set_auto_reset(int on) { g_auto_reset = on; }
static std::vector<float> g_goal_buf;   // kwarg init_buffer (jaco_set_init_buffer of the library)
static int g_goal_n = 0, g_goal_stride = 0;
extern "C" void emu_set_init_buffer(const float* rows, int nrows, int stride) {
  g_goal_buf.assign(rows, rows + (rows ? (size_t)nrows * stride : 0)); g_goal_n = rows ? nrows : 0; g_goal_stride = rows ? stride : 0;
}
// what jaco_reset does for one env: the argument block jaco_reset fills from the handle, filled from the loaded model, and the routine
// jaco_reset_kernel calls (the state here has no low halves); the forward pass is a JM_FORWARD emu_env_call
extern "C" int emu_reset_env(const void* blob, long blob_size, int task_id, unsigned long long seed, int env, float* qpos, float* qvel, float* qacc_ws,
                             float* task, float* marker) {
  if (load_model(blob, blob_size)) return -1;
  JacoResetArgs R{};
  R.qpos0 = g_qpos0.data(); R.qpos = qpos; R.qvel = qvel; R.qacc_ws = qacc_ws; R.task = task; R.marker = marker; R.marker_rest = &g_model.marker_rest[0][0];
  R.nq = g_model.nq; R.nv = g_model.nv; R.task_id = task_id; R.has_free = g_model.nq >= 23; R.seed = seed;
  for (int k = 0; k < 3; k++) R.base[k] = g_model.base_pos[k];
  R.goals = GoalBuffer{g_goal_buf.empty() ? nullptr : g_goal_buf.data(), g_goal_n, g_goal_stride};
  jaco_reset_env(R, env);
  return 0;
}
extern "C" int emu_env_call(const void* blob, long blob_size, int nenv, int mode, int frame_skip, int task_id, int nact, unsigned long long seed,
                            float* qpos, float* qvel, float* qacc_ws, float* sensordata, unsigned* flags, int* stats, float* task, float* cache,
                            const float* action, const float* noise, float* obs, float* reward, unsigned char* done, float* marker, int* heavy_envs) {
  if (load_model(blob, blob_size)) return -1;
  JacoStepArgs A{};
  A.model = &g_model; A.hull = g_hull.data(); A.qpos = qpos; A.qvel = qvel; A.qacc_ws = qacc_ws; A.ctrl = qvel; A.sensordata = sensordata;
  A.flags = flags; A.stats = stats; A.nenv = nenv; A.nsub = mode == JM_FORWARD ? 1 : frame_skip; A.env_mode = mode; A.task_id = task_id; A.nact = nact;
  A.seed = seed; A.task = task; A.cache = cache; A.action = action; A.noise = noise; A.obs = obs; A.reward = reward; A.done = done; A.marker = marker; A.dbg_env = -1;
  A.auto_reset = g_auto_reset && mode == JM_STEP && jaco_task_auto_resets(task_id); A.qpos0 = g_qpos0.data();
  A.goal_buf = g_goal_buf.empty() ? nullptr : g_goal_buf.data(); A.goal_n = g_goal_n; A.goal_stride = g_goal_stride;
  return emu_launch(A, heavy_envs);
}
// the reset pose the loader reads from the blob (what jaco_create uploads): nq floats; returns nq
extern "C" int emu_qpos0(const void* blob, long blob_size, float* out) {
  if (load_model(blob, blob_size)) return -1;
  std::copy(g_qpos0.begin(), g_qpos0.end(), out);
  return (int)g_qpos0.size();
}
// rest pose of the two task-layer markers (what jaco_reset_state writes): 24 floats
extern "C" int emu_marker_rest(const void* blob, long blob_size, float* out) {
  if (load_model(blob, blob_size)) return -1;
  for (int k = 0; k < 24; k++) out[k] = g_model.marker_rest[k / 12][k % 12];
  return 0;
}

// ctrl-level step (jaco_physics_step): the contact record rec [nenv][cap] / ncon [nenv], or rec = NULL (off; what
// jaco_set_contact_record(h, NULL, ...) leaves); the stage dump dbg of env dbg_env (dbg_env < 0: none)
extern "C" int emu_physics_step(const void* blob, long blob_size, int nenv, int nsub, int disable_contact, float* qpos, float* qvel, float* qacc_ws,
                                const float* ctrl, float* sensordata, unsigned* flags, int* stats, JacoContact* rec, int* ncon, int cap,
                                float* dbg, int dbg_env, int* heavy_envs) {
  if (const char* why = rec ? jaco_contact_record_check(rec, ncon, cap) : nullptr) return refuse(std::string("jaco_set_contact_record: ") + why);
  if (load_model(blob, blob_size)) return -1;
  JacoStepArgs A{};
  A.model = &g_model; A.hull = g_hull.data(); A.qpos = qpos; A.qvel = qvel; A.qacc_ws = qacc_ws; A.ctrl = ctrl; A.sensordata = sensordata;
  A.flags = flags; A.stats = stats; A.nenv = nenv; A.nsub = nsub; A.disable_contact = disable_contact; A.dbg = dbg; A.dbg_env = dbg_env;
  A.con_rec = reinterpret_cast<JacoContactRec*>(rec); A.con_n = rec ? ncon : nullptr; A.con_cap = rec ? cap : 0;
  return emu_launch(A, heavy_envs);
}

// A contact-free ctrl-level step as a handle runs it (jaco_physics_step under option "disable_contact"): like emu_physics_step, with the
// compensated low words the library keeps between calls (qpos_lo / qvel_lo, zeroed by jaco_set_state).
extern "C" int emu_step_lo(const void* blob, long blob_size, int nenv, int nsub, float* qpos, float* qvel, float* qacc_ws, float* qpos_lo, float* qvel_lo,
                           const float* ctrl, unsigned* flags) {
  if (load_model(blob, blob_size)) return -1;
  JacoStepArgs A{};
  A.model = &g_model; A.hull = g_hull.data(); A.qpos = qpos; A.qvel = qvel; A.qacc_ws = qacc_ws; A.qpos_lo = qpos_lo; A.qvel_lo = qvel_lo; A.ctrl = ctrl;
  A.flags = flags; A.nenv = nenv; A.nsub = nsub; A.disable_contact = 1; A.dbg_env = -1;
  return emu_launch(A, nullptr);
}

// ---- the ten query-style entries.  Each is its library entry with the handle taken away: jaco_<entry>_bind of entry_args.h, the very
// function jaco_env.hip calls, turns the arguments into the kernel's block (every check, the defaults, the records by value) or refuses;
// the block gets the host copy of the model and the kernel runs over the grid the library launches, one wavefront per env (per rollout).
// Where the library falls back to the handle's fp32 state, the rollouts are handed it as handle_qpos / handle_qvel [num_envs][..];
// the other entries are always called with their state.
template <class Kernel>
static int run_grid(int grid, Kernel kernel) {   // (the kernels read only blockIdx)
  emu_grid = grid;
  for (int e = 0; e < grid; e++) emu_run_wave(e, kernel);
  return 0;
}

extern "C" int emu_query(const void* blob, long blob_size, int nenv, const float* qpos, const float* qvel, const JacoFrame* frames, int nframes,
                         float* xpos, float* xmat, float* jac, float* qM, float* qfrc_bias) {
  if (load_model(blob, blob_size)) return -1;
  const JacoQueryOut out = {xpos, xmat, jac, qM, qfrc_bias};
  JacoQueryArgs Q;
  const std::string why = jaco_query_bind(g_model, frames, nframes, qpos, qvel, &out, nenv, nullptr, nullptr, &Q);
  if (!why.empty()) return refuse(why);
  Q.model = &g_model;
  return run_grid(nenv, [&]() { jaco_query_kernel(Q); });
}

extern "C" int emu_ik(const void* blob, long blob_size, int nenv, const JacoFrame* frame, const JacoIkOptions* opt, const float* qpos_seed,
                      const float* target_pos, const float* target_quat, float* qpos_out, float* resid, int* status) {
  if (load_model(blob, blob_size)) return -1;
  JacoIkArgs Q;
  const std::string why = jaco_ik_bind(g_model, frame, opt, qpos_seed, target_pos, target_quat, qpos_out, resid, status, nenv, nullptr, &Q);
  if (!why.empty()) return refuse(why);
  Q.model = &g_model;
  return run_grid(nenv, [&]() { jaco_ik_kernel(Q); });
}

extern "C" int emu_osc(const void* blob, long blob_size, int nenv, const JacoFrame* frames, int nframes, const JacoOscOptions* opt,
                       const float* qpos, const float* qvel, const float* target_pos, const float* target_quat, const float* ctrl_in,
                       float* ctrl_out, int* status) {
  if (load_model(blob, blob_size)) return -1;
  JacoOscArgs Q;
  const std::string why = jaco_osc_bind(g_model, frames, nframes, opt, qpos, qvel, target_pos, target_quat, ctrl_in, ctrl_out, status, nenv, nullptr, nullptr, &Q);
  if (!why.empty()) return refuse(why);
  Q.model = &g_model;
  return run_grid(nenv, [&]() { jaco_osc_kernel(Q); });
}

// (a NULL task record forwards to emu_osc, as jaco_osc_task forwards to jaco_osc)
extern "C" int emu_osc_task(const void* blob, long blob_size, int nenv, const JacoFrame* frames, int nframes, const JacoOscOptions* opt,
                            const JacoOscTask* task, const float* qpos, const float* qvel, const float* target_pos, const float* target_quat,
                            const float* rest_qpos, const float* ctrl_in, float* ctrl_out, int* status) {
  if (!task) return emu_osc(blob, blob_size, nenv, frames, nframes, opt, qpos, qvel, target_pos, target_quat, ctrl_in, ctrl_out, status);
  if (load_model(blob, blob_size)) return -1;
  JacoOscTaskArgs T;
  const std::string why = jaco_osc_task_bind(g_model, frames, nframes, opt, task, qpos, qvel, target_pos, target_quat, rest_qpos, ctrl_in, ctrl_out, status, nenv,
                                             nullptr, nullptr, &T);
  if (!why.empty()) return refuse(why);
  T.o.model = &g_model;
  return run_grid(nenv, [&]() { jaco_osc_task_kernel(T); });
}

extern "C" int emu_joint(const void* blob, long blob_size, int nenv, const JacoJointOptions* opt, const float* qpos, const float* qvel,
                         const float* target_qpos, const float* target_qvel, const float* qacc_ff, const float* ctrl_in, float* ctrl_out) {
  if (load_model(blob, blob_size)) return -1;
  JacoJointArgs Q;
  const std::string why = jaco_joint_bind(g_model, opt, qpos, qvel, target_qpos, target_qvel, qacc_ff, ctrl_in, ctrl_out, nenv, nullptr, nullptr, &Q);
  if (!why.empty()) return refuse(why);
  Q.model = &g_model;
  return run_grid(nenv, [&]() { jaco_joint_kernel(Q); });
}

extern "C" int emu_fd(const void* blob, long blob_size, int nenv, const JacoFdOptions* opt, const float* qpos, const float* qvel, const float* ctrl,
                      const JacoFdOut* out) {
  if (load_model(blob, blob_size)) return -1;
  JacoFdArgs Q;
  const std::string why = jaco_fd_bind(g_model, opt, qpos, qvel, ctrl, out, nenv, nullptr, nullptr, &Q);
  if (!why.empty()) return refuse(why);
  Q.model = &g_model;
  return run_grid(nenv, [&]() { jaco_fd_kernel(Q); });
}

extern "C" int emu_rollout(const void* blob, long blob_size, const JacoRolloutOptions* opt, const JacoFrame* frame, int n, const int32_t* state_idx, int nstates,
                           const float* qpos0, const float* qvel0, const float* ctrl, const JacoRolloutOut* out, int num_envs, const float* handle_qpos,
                           const float* handle_qvel) {
  if (load_model(blob, blob_size)) return -1;
  JacoRolloutArgs Q;
  const std::string why = jaco_rollout_bind(g_model, opt, frame, n, state_idx, nstates, qpos0, qvel0, ctrl, out, num_envs, handle_qpos, handle_qvel, &Q);
  if (!why.empty()) return refuse(why);
  Q.model = &g_model;
  return run_grid(n, [&]() { jaco_rollout_kernel(Q); });
}

extern "C" int emu_rollout_fb(const void* blob, long blob_size, const JacoRolloutFbOptions* opt, const JacoFrame* frame, int n, const int32_t* state_idx, int nstates,
                              const float* qpos0, const float* qvel0, const JacoRolloutPlan* plan, const JacoRolloutFbOut* out, int num_envs,
                              const float* handle_qpos, const float* handle_qvel) {
  if (load_model(blob, blob_size)) return -1;
  JacoRolloutFbArgs Q;
  const std::string why = jaco_rollout_fb_bind(g_model, opt, frame, n, state_idx, nstates, qpos0, qvel0, plan, out, num_envs, handle_qpos, handle_qvel, &Q);
  if (!why.empty()) return refuse(why);
  Q.R.model = &g_model;
  return run_grid(n, [&]() { jaco_rollout_fb_kernel(Q); });
}

extern "C" int emu_rollout_cost(const void* blob, long blob_size, const JacoRolloutCostOptions* opt, const JacoFrame* frame, int n, const int32_t* state_idx,
                                int nstates, const float* qpos0, const float* qvel0, const JacoRolloutPlan* plan, const JacoRolloutGoal* goal,
                                const JacoRolloutCostOut* out, int num_envs, const float* handle_qpos, const float* handle_qvel) {
  if (load_model(blob, blob_size)) return -1;
  JacoRolloutCostArgs Q;
  const std::string why = jaco_rollout_cost_bind(g_model, opt, frame, n, state_idx, nstates, qpos0, qvel0, plan, goal, out, num_envs, handle_qpos, handle_qvel, &Q);
  if (!why.empty()) return refuse(why);
  Q.F.R.model = &g_model;
  return run_grid(n, [&]() { jaco_rollout_cost_kernel(Q); });
}

extern "C" int emu_rollout_osc(const void* blob, long blob_size, const JacoRolloutOscOptions* opt, const JacoFrame* frames, int nframes, const JacoFrame* out_frame, int n,
                               const int32_t* state_idx, int nstates, const float* qpos0, const float* qvel0, const JacoRolloutOscPlan* plan,
                               const JacoRolloutFbOut* out, int num_envs, const float* handle_qpos, const float* handle_qvel) {
  if (load_model(blob, blob_size)) return -1;
  JacoRolloutOscArgs Q;
  const std::string why = jaco_rollout_osc_bind(g_model, opt, frames, nframes, out_frame, n, state_idx, nstates, qpos0, qvel0, plan, out, num_envs, handle_qpos,
                                                handle_qvel, &Q);
  if (!why.empty()) return refuse(why);
  Q.R.model = &g_model;
  return run_grid(n, [&]() { jaco_rollout_osc_kernel(Q); });
}

// ---- env snapshots: the table and the save / load routines of snapshot.h -- the very header the GPU kernels jaco_save_envs_kernel /
// jaco_load_envs_kernel are compiled from; here one "lane" walks a whole row ------------------------------------------------------------
extern "C" int snap_nfield() { return JSNAP_NFIELD; }
extern "C" const char* snap_field_name(int i) { return i >= 0 && i < JSNAP_NFIELD ? jaco_snap_field_names[i] : nullptr; }
extern "C" int snap_header_words() { return JSNAP_HEADER_WORDS; }
extern "C" unsigned snap_bad_flag() { return JSNAP_FLAG_BAD; }
// ptrs[JSNAP_NFIELD]: the arrays in table order (NULL = the caller keeps no such array)
static JacoSnapTable table_of(void* const* ptrs, int nq, int nv, int nsensor, int task_id, int nenv) {
  JacoSnapSrc s;
  int i = 0;
#define SNAP_X_PTR(f, w) s.f = ptrs ? ptrs[i] : nullptr; i++;
  JACO_SNAPSHOT_FIELDS(SNAP_X_PTR, 0, 0, 0)
#undef SNAP_X_PTR
  return jaco_snapshot_table(s, nq, nv, nsensor, task_id, nenv);
}
// words[i], off[i] of every field; returns W
extern "C" int snap_table(int nq, int nv, int nsensor, int task_id, int* words, int* off, unsigned* fingerprint) {
  const JacoSnapTable T = table_of(nullptr, nq, nv, nsensor, task_id, 0);
  for (int i = 0; i < JSNAP_NFIELD; i++) { words[i] = T.f[i].words; off[i] = T.f[i].off; }
  if (fingerprint) *fingerprint = T.fingerprint;
  return T.W;
}
// the grids of the two kernels, entry by entry (jaco_env.hip: one wavefront per entry)
extern "C" void snap_save(void* const* ptrs, int nq, int nv, int nsensor, int task_id, int nenv, const int32_t* env_idx, int n, uint32_t* rows) {
  const JacoSnapTable T = table_of(ptrs, nq, nv, nsensor, task_id, nenv);
  for (int i = 0; i < n; i++) {
    int e, r;
    if (jaco_snap_entry(T, env_idx, nullptr, n, i, &e, &r)) jaco_snap_save_entry(T, e, rows + (size_t)i * T.W, 0, 1);
  }
}
extern "C" void snap_load(void* const* ptrs, int nq, int nv, int nsensor, int task_id, int nenv, const int32_t* env_idx, int n, const uint32_t* rows, int nrows,
                          const int32_t* row_idx) {
  const JacoSnapTable T = table_of(ptrs, nq, nv, nsensor, task_id, nenv);
  for (int i = 0; i < n; i++) {
    int e, r;
    if (jaco_snap_entry(T, env_idx, row_idx, nrows, i, &e, &r)) jaco_snap_load_entry(T, e, rows + (size_t)r * T.W, 0, 1);
  }
}
