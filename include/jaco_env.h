/* C ABI of the MI355X-native batched Jaco environment (libjaco_env.so).
 *
 * The reference has no FFI of its own: its only native boundary is mujoco-py's Cython layer
 * (mujoco_py.cymj), crossed at the call sites listed per entry point below (all paths relative to
 * /root/reference).  This library replaces what sits behind those calls, batched over num_envs
 * independent environments, one 64-lane wavefront per environment.
 *
 * Conventions: every function returns 0 on success and a negative JACO_E* code on failure, never
 * throws; jaco_last_error() gives the message.  All "*_dev" arguments are DEVICE pointers supplied and
 * owned by the caller (e.g. torch tensor .data_ptr()); the library owns only its model constants,
 * per-env state and scratch.  Calls are asynchronous on the given HIP stream (hipStream_t passed as
 * void*; NULL = default stream) and perform no hidden synchronisation unless stated.  One handle per
 * GPU; a handle is not thread-safe (the reference is single-threaded: main.py:27).
 *
 * Batched array layout: row-major [num_envs][n] fp32, i.e. the 64 lanes of the wavefront that owns
 * environment e read consecutive addresses of row e.
 */
#ifndef JACO_ENV_H
#define JACO_ENV_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define JACO_OK 0
#define JACO_EINVAL (-1)   /* bad argument / model */
#define JACO_EHIP (-2)     /* HIP runtime error */
#define JACO_ENODEV (-3)   /* no usable gfx950 device */

/* per-env sticky flag bits (jaco_get_flags) */
#define JACO_FLAG_CON_OVERFLOW 1u   /* more contacts than the per-env contact buffer */
#define JACO_FLAG_EFC_OVERFLOW 2u   /* more constraint rows than the per-env row buffer */
#define JACO_FLAG_CAND_OVERFLOW 4u  /* more broadphase survivors than the candidate buffer */
#define JACO_FLAG_NAN 8u            /* non-finite velocity: env should be reset */
#define JACO_FLAG_SOLVER_MAXITER 16u
#define JACO_FLAG_HEAVY_TIER 32u     /* informational: stepped by a bigger tier (128 / 256 / 512 rows) at least once (not an error) */
#define JACO_FLAG_TIER_RETURN 128u   /* informational: the heavy tier gave the env back to the light code in mid-step (overflow was transient) */
#define JACO_FLAG_BAIL_CAUSE_SHIFT 8  /* informational, bits 8..16: which capacity (bit 0 contacts, 1 rows, 2 candidates) made tier 0 / 1 / 2 (3 bits each) hand the env on */
#define JACO_FLAG_OSC_SINGULAR 64u   /* informational: |det(J M^-1 J^T)| < 1e-3, the controller used its pseudo-inverse branch */
#define JACO_FLAG_PREREACH_CAP 0x20000u /* the grasping reset's pre-reach loops (unbounded in the reference) stopped at the substep cap */
#define JACO_FLAG_BAD_SNAPSHOT 0x40000u /* jaco_load_envs was given a row of another build, model, task or layout version for this env: the env was left as it was */

/* task ids (env_script/env_mujoco.py:18-23; only picking/placing return the 4-tuple step() unpacks) */
#define JACO_TASK_PICKING 0
#define JACO_TASK_PLACING 1
#define JACO_TASK_REACHING 2
#define JACO_TASK_GRASPING 3       /* reward env_mujoco_util.py:352-391, termination :521-536 (+ the success flag its 3-tuple lacks), reset pre-reach :123-170 */
#define JACO_TASK_PICKANDPLACE 4   /* reward 0, termination :585-600 with the `picked` flag, 1200-step episodes */
#define JACO_TASK_CARRYING 5       /* reset = in-hand hold :106-117 + pre-reach :123-170; reward 0; every episode ends in its first step (:549-550) */
#define JACO_TASK_RELEASING 6      /* own init pose :186-189, in-hand hold :106-117; reward 0; termination :551-566 (+ success flag) */
#define JACO_TASK_PUSHING 7        /* 6-wide action (env_mujoco.py:79-82); reward 0; every episode ends in its first step (:583-584) */

typedef struct JacoHandle JacoHandle;

typedef struct JacoConfig {
  const void* model_blob;      /* JACOMDL1 bytes (host memory), see mujoco_jaco_amd/modelc */
  size_t model_blob_size;
  int num_envs;
  int device;                  /* HIP device ordinal */
  int frame_skip;              /* physics substeps per env step; reference: 50 (env_mujoco.py:24) */
  int task;                    /* JACO_TASK_* */
  uint64_t seed;               /* counter-based RNG seed for reset / sub-goal noise */
} JacoConfig;

/* JacoMujocoEnvUtil.__init__ -> MujocoConfig(xml) + Mujoco.connect()  (env_mujoco_util.py:28-33,
 * mujoco_config.py:74 mjp.load_model_from_path, mujoco.py:55-56 MjSim + forward). */
int jaco_create(const JacoConfig* cfg, JacoHandle** out);
int jaco_destroy(JacoHandle* h);
/* Message of the last failure on this handle; pass NULL for a failure of jaco_create itself. */
const char* jaco_last_error(const JacoHandle* h);

/* model.nq / nv / nu, len(sensordata); observation and action widths (env_mujoco.py:51-63,79-89). */
int jaco_dims(const JacoHandle* h, int* nq, int* nv, int* nu, int* nsensor, int* nobs, int* nact);
int jaco_num_envs(const JacoHandle* h);

/* sim.get_state()/set_state() + sim.data.qpos/qvel writes (mujoco.py:213-246,332-347).
 * Any pointer may be NULL to skip that field.  qacc_warmstart is part of the state because the
 * constraint solver is warm-started from it, as in MuJoCo. Device-to-device copies on `stream`.
 * Precision: the library carries qpos / qvel as compensated pairs of floats (hi + lo, ~48 significant bits: the integrators
 * advance the pair, every other computation reads the fp32 value `hi`; option "compensated" = 0 turns that off).  get_state
 * returns `hi`, the fp32 rounding of the state; set_state writes `hi` and clears `lo` (the state becomes exactly the floats
 * handed in), so a get -> set round trip rounds the state to fp32 once. */
int jaco_set_state(JacoHandle* h, const float* qpos_dev, const float* qvel_dev, const float* qacc_ws_dev, void* stream);
int jaco_get_state(JacoHandle* h, float* qpos_dev, float* qvel_dev, float* qacc_ws_dev, void* stream);
/* sim.reset() for every env: qpos0, zero velocities (env_mujoco_util.py:93). */
int jaco_reset_state(JacoHandle* h, void* stream);

/* Mujoco.send_forces(u): sim.data.ctrl[:] = u; sim.step()  (mujoco.py:258-278), `nsub` times with
 * the same ctrl, for all envs.  ctrl_dev: [num_envs][nu] fp32.  This is the ctrl-level entry used
 * for oracle parity and the physics benchmark. */
int jaco_physics_step(JacoHandle* h, const float* ctrl_dev, int nsub, void* stream);

/* sim.data.get_sensor(...) for the 20 touch sensors (env_mujoco_util.py:470-475): values computed
 * by the last substep, sensordata order of the XML (EE_touch first). out_dev: [num_envs][nsensor]. */
int jaco_get_sensordata(JacoHandle* h, float* out_dev, void* stream);

/* Per-env sticky error bits / last-substep statistics [num_envs][4] = {ncon, nefc, solver iterations,
 * narrowphase candidates}. */
int jaco_get_flags(JacoHandle* h, uint32_t* out_dev, void* stream);
int jaco_clear_flags(JacoHandle* h, void* stream);
int jaco_get_stats(JacoHandle* h, int32_t* out_dev, void* stream);

/* ---- env level: JacoMujocoEnv.reset / step (env_script/env_mujoco.py:99-139), batched -------------------------
 * jaco_reset: _reset (env_mujoco_util.py:92-174) for the envs whose mask byte is non-zero (NULL = all): counter-based
 *   RNG draws of the per-task initial state (Appendix A of SURVEY.md), sim.forward(), then _get_observation for those
 *   envs into their rows of obs_dev [num_envs][26] (rows of the other envs are left as they are).  Task `placing` runs jaco_placing_hold(mask, 150) between the draws and the observation.
 * jaco_placing_hold: the object part of the placing reset (env_mujoco_util.py:106-117): object to the grasp frame EE_obj
 *   (4 cm back along its x axis), EE target = current EE pose, then nsub x { OSC torque from the current state's M, J, bias
 *   (each iteration follows a sim.forward()), sim.step() with gripper command 0.6, set_obj_xyz: object re-pinned, velocities
 *   of all free bodies zeroed (mujoco.py:217-227) }.  Exposed so that a caller can replay the hold from its own state.
 * jaco_step: np.clip of the action to [-1, 1] (env_mujoco.py:117) is done inside the kernel; then _take_action, frame_skip x
 *   (OSC torque + sim.step()), make_observation, _get_reward, terminal_inspection.  action_dev [num_envs][7] (6 for reaching),
 *   obs_dev [num_envs][26] f32, reward_dev [num_envs] f32, done_dev [num_envs] u8.  By default an env that returned done stays
 *   frozen (done = 1, reward 0, obs row untouched) until jaco_reset is called for it.  With jaco_set_option("auto_reset", 1)
 *   (tasks whose reset is draws + sim.forward(): picking, reaching, pickAndplace, pushing) the wave that ends an episode resets the
 *   env itself: done / reward are the terminal step's, the obs row is the NEW episode's first observation, and the terminal
 *   step's (success, wb) / observation are latched for jaco_get_last_terminal / jaco_get_terminal_obs.
 * jaco_forward: sim.forward() + _get_observation from the current state (after jaco_set_state / jaco_set_task_state).
 * jaco_set_noise: optional [num_envs][12] uniform draws replacing the internal RNG for the rule-based sub-goal noise
 *   (6 for the marker placed in _take_action, 6 for the observation; env_mujoco_util.py:279,295); NULL restores the RNG.
 * Task rows ([num_envs][jaco_task_row_floats()], layout JT_* in csrc/env_logic.h) expose gripper command, step
 *   counters, goals and the success flag (get_wb / accum_succ bookkeeping stay on the host side). */
int jaco_reset(JacoHandle* h, const uint8_t* mask_dev, float* obs_dev, void* stream);
int jaco_placing_hold(JacoHandle* h, const uint8_t* mask_dev, int nsub, void* stream);
/* The pre-reach part of the grasping reset (env_mujoco_util.py:123-170), run by jaco_reset for task grasping after the draws: EE target =
 * [object goal, orientation looking along EE -> object (float16 angles, yaw drawn)]; loop 1 { stop_obj, controller + sim.step } until the
 * EE is within 0.2 m of the object goal or its orientation within pi/6 of the sampled reaching goal's; loop 2 { controller + sim.step }
 * until within 0.15 m; then _get_observation into the masked rows of obs_dev.  The reference's loops are unbounded: max_substeps caps
 * them (jaco_reset uses 4000; an env that hits the cap gets JACO_FLAG_PREREACH_CAP). */
int jaco_grasping_prereach(JacoHandle* h, const uint8_t* mask_dev, int max_substeps, float* obs_dev, void* stream);
int jaco_step(JacoHandle* h, const float* action_dev, float* obs_dev, float* reward_dev, uint8_t* done_dev, void* stream);
int jaco_forward(JacoHandle* h, float* obs_dev, void* stream);
/* The two halves of jaco_step the reference also exposes as public methods of JacoMujocoEnv (env_mujoco.py:144-161):
 * jaco_take_action: take_action(a) alone -- new EE target, gripper command / ramp end points, the two marker poses, 6 noise
 *   draws; no physics.  A following jaco_step would call _take_action again, as the reference's step() does.
 * jaco_terminal_inspection: terminal_inspection() alone -- current_steps += 1, then the task's termination rule on the
 *   poses / touch sensors of the last forward pass; done_dev [num_envs] u8, bonus_dev [num_envs] f32 (the reference's
 *   additional_reward); get_wb / the success flag are then in the task row (JT_WB, JT_SUCC).  Finished envs freeze as in jaco_step. */
int jaco_take_action(JacoHandle* h, const float* action_dev, void* stream);
int jaco_terminal_inspection(JacoHandle* h, uint8_t* done_dev, float* bonus_dev, void* stream);
/* Lifetime: jaco_set_noise / jaco_set_subgoal only record the pointer in the handle; the buffer is read by every later jaco_step /
 * jaco_take_action / jaco_forward / jaco_reset on whatever stream that call uses.  It must stay allocated and unchanged until
 * those calls have completed on the device or the pointer has been replaced (NULL detaches it). */
int jaco_set_noise(JacoHandle* h, const float* noise_dev);
/* Observation branch rulebased_subgoal = False (env_mujoco_util.py:255-270; option "obs_mode" = 1): obs[17:23] is the reaching goal
 * drawn at reset, and _take_action moves the "subgoal_reach" marker to subgoal + previous target (:609) when the caller passes the
 * policy's sub-goal offsets [num_envs][6] here (NULL: the marker stays where it is). */
int jaco_set_subgoal(JacoHandle* h, const float* subgoal_dev);
/* kwarg init_buffer of the reference (env_mujoco_util.py:46,208-212): a buffer of recorded rows from which every reset draws its reaching
 * goal -- random_idx = np.random.randint(0, len(buffer) - 1) (rows 0 .. len - 2), position = row[1:4], orientation = row[4:7], no float16
 * cast -- instead of sampling it (:199-207).  rows_dev [nrows][row_floats] f32 on the device, copied by the library; NULL restores the
 * sampled goal.  nrows >= 2 (numpy's randint(0, 0) raises), row_floats >= 7. */
int jaco_set_init_buffer(JacoHandle* h, const float* rows_dev, int nrows, int row_floats, void* stream);
int jaco_get_task_state(JacoHandle* h, float* out_dev, void* stream);
int jaco_set_task_state(JacoHandle* h, const float* in_dev, void* stream);
int jaco_task_row_floats(void);
/* What the most recent TERMINAL step of every env returned besides (reward, done): out_dev [num_envs][2] f32 = (success flag, wb) -- the
 * `succ` and `wb` of terminal_inspection (env_mujoco.py:125,144-150), latched by the step that ended the episode.  Needed with option
 * "auto_reset", where the task row already belongs to the new episode when jaco_step returns (the reference's accum_succ bookkeeping,
 * env_mujoco.py:129-136, reads succ in the terminal step).  Rows of envs that have not finished an episode yet are (0, 0). */
int jaco_get_last_terminal(JacoHandle* h, float* out_dev, void* stream);
/* ... and the observation of that terminal step, out_dev [num_envs][26] f32, latched by EVERY terminal jaco_step with or without option
 * "auto_reset" (with it the env's obs_dev row already holds the new episode's first observation; a learner bootstrapping the value of a
 * timed-out state needs the last one of the old episode).  Rows of envs that have not finished an episode yet are zero. */
int jaco_get_terminal_obs(JacoHandle* h, float* out_dev, void* stream);
/* Marker poses [num_envs][2][12] f32: {"hand", "subgoal_reach"} x {position, rotation matrix row-major} -- the two mocap bodies
 * _take_action moves every env step (set_mocap_xyz / set_mocap_orientation, mujoco.py:248-256, env_mujoco_util.py:613-615,
 * 644-646).  Their contype-8 geoms collide with the EE axis sticks; jaco_step updates them in-kernel, jaco_reset* park
 * them at their XML pose. */
int jaco_get_markers(JacoHandle* h, float* out_dev, void* stream);
int jaco_set_markers(JacoHandle* h, const float* in_dev, void* stream);
int jaco_set_frame_skip(JacoHandle* h, int frame_skip);

/* ---- env snapshots: sim.get_state() / sim.set_state() (mujoco.py:213-246,332-347) as a FULL-state pair, per env and by index.
 * The reference's MjSimState is everything its sim.step() reads; here that is more than jaco_get_state / jaco_get_task_state /
 * jaco_get_markers hand out (jaco_set_state rounds the compensated state to fp32 and zeroes the tier hints; the controller's cache, the
 * touch values, flags, statistics and the terminal latches have no accessor), and those calls move whole batches.  A snapshot of one env
 * is one ROW of W = jaco_snapshot_words(h) 32-bit words (W a multiple of 4: rows of a [n][W] buffer are 16-byte aligned; the buffer is the
 * caller's, e.g. a torch int32 tensor, and must be 16-byte aligned).  The row holds every word a later launch reads of that env (table and
 * layout: csrc/snapshot.h): both halves of the compensated qpos / qvel, qacc_warmstart, sensordata, flags, stats, tier hint, step cost,
 * task row (draw counter, done flag, counters, goals, target, gripper ramp), controller cache, marker poses, terminal latches.  An env
 * loaded from a row continues BIT FOR BIT as the env the row was saved from did, on any env index of the same handle or of another
 * handle of the same build, model, task and layout version: word 0 of a row is a fingerprint of those.
 * Not in a row: the separating-direction cache (its entries are re-validated before use and cannot change a result; a load leaves the
 * destination's as they are), per-launch scratch, buffers the library only points to (jaco_set_noise / jaco_set_subgoal /
 * jaco_set_contact_record / jaco_set_init_buffer) and handle-wide settings (seed, frame_skip, options).
 * Random numbers: the stream is keyed by (seed, env index, counter) and only the counter is state.  A row loaded into the env index it
 * came from (same seed) continues the same stream; loaded into another index it gives the same physical state on THAT index's stream,
 * from the same counter.  With injected noise (jaco_set_noise) and no reset in the window a clone continues exactly as its source.
 *
 * jaco_save_envs: rows_dev[i] := state of env env_idx_dev[i], i < n.  env_idx_dev NULL: identity (then n must be num_envs).
 * jaco_load_envs: env env_idx_dev[i] := rows_dev[row_idx_dev[i]], i < n.  env_idx_dev NULL: identity (n == num_envs); row_idx_dev NULL:
 *   entry i reads row i (n <= nrows).  nrows = rows in the buffer.  The same row may be loaded into many envs (fan-out); an env index
 *   listed twice is undefined.  "env e := env s" in place is a save into a scratch buffer followed by a load with row_idx_dev.
 * Both: asynchronous on `stream`, ONE kernel launch (none for n == 0), no allocation, no synchronisation, no host copy.  JACO_EINVAL for
 * n < 0, n > num_envs, NULL or misaligned rows, a NULL env index list with n != num_envs.  What only the device can see does not fault
 * and does not stay silent: an env index outside [0, num_envs) or a row index outside [0, nrows) makes that entry a no-op; a row whose
 * fingerprint is not this handle's leaves the env untouched and sets JACO_FLAG_BAD_SNAPSHOT in that env's flags.
 * After a load the next launch prepares its tier queues itself (as after any launch that does not route): envs start in the tier their
 * loaded hint names. */
int jaco_snapshot_words(const JacoHandle* h);
int jaco_save_envs(JacoHandle* h, const int32_t* env_idx_dev, int n, uint32_t* rows_dev, void* stream);
int jaco_load_envs(JacoHandle* h, const int32_t* env_idx_dev, int n, const uint32_t* rows_dev, int nrows, const int32_t* row_idx_dev, void* stream);

/* ---- robot-configuration queries: MujocoConfig.J / M / g / R / quaternion / Tx (mujoco_config.py:201-447) and Mujoco.get_xyz /
 * get_orientation (mujoco.py:148-215), batched.  The values are those of a sim.forward() on the given state: body poses, the
 * Jacobians at the requested points, the dense mass matrix and qfrc_bias.  (The reference's controller, with use_sim_state=True,
 * reads them one substep stale -- SURVEY 3.1; a caller who wants that lag keeps the previous substep's query result.)
 * A frame: `body` = fused body index (-1 = world-fixed), pose (pos, row-major mat) in that body's frame, Jacobian reference `point` in
 * the frame's own coordinates (mujoco_jaco_amd/robot_config.py builds frames from MJCF body names; the body's COM gives mj_jacBodyCom).
 * Outputs (device pointers, fp32, row-major per env; NULL = not wanted, its work is skipped where that is cheap):
 *   xpos [num_envs][nframes][3], xmat [num_envs][nframes][9]  -- frame position and rotation (MuJoCo's xmat layout);
 *   jac [num_envs][nframes][6][nv]  -- rows 0-2 translational, 3-5 rotational Jacobian at the frame's point; a column is zero for a dof
 *        that does not move the frame's body (mj_jacBodyCom / mj_jac);
 *   qM [num_envs][nv][nv]  -- dense, symmetric (mj_fullM);   qfrc_bias [num_envs][nv]  -- Coriolis, centrifugal and gravity forces.
 * State: qpos_dev [num_envs][nq] / qvel_dev [num_envs][nv] override the handle's state (NULL = its current state, the fp32 words
 * jaco_get_state returns).  Nothing of the handle is written: state, task rows, flags and sensordata stay as they are.
 * Asynchronous on `stream`: no allocation, no synchronisation, no host copy (the frames travel in the kernel arguments).
 * JACO_EINVAL when nframes is outside [0, JACO_QUERY_MAX_FRAMES] or a frame's body outside [-1, number of fused bodies). */
#define JACO_QUERY_MAX_FRAMES 16
typedef struct JacoFrame { int body; float pos[3]; float mat[9]; float point[3]; } JacoFrame;
typedef struct JacoQueryOut { float* xpos; float* xmat; float* jac; float* qM; float* qfrc_bias; } JacoQueryOut;
int jaco_query(JacoHandle* h, const JacoFrame* frames_host, int nframes, const float* qpos_dev, const float* qvel_dev,
               const JacoQueryOut* out, void* stream);

/* ---- inverse kinematics: which arm configuration puts this frame at this pose?  A damped least-squares iteration per env, all of it
 * in one kernel launch (mujoco_jaco_amd/csrc/ik.h).  Per env: a seed qpos, a target position and, optionally, a target orientation (unit
 * quaternion, w first).  Per call: one frame -- `point` is the controlled point in the frame's coordinates, the orientation is the
 * frame's -- and the options.  Active dofs: the hinge dofs on the chain of the frame's body, intersected with dof_mask (bit d = dof d)
 * when that is non-zero.  Iteration: p = frame point, e_p = target - p, e_r = rotation vector of R* R^T (0 without an orientation);
 * converged when |e_p| < tol_pos and (no orientation or |e_r| < tol_rot); dq = J^T (J J^T + damping^2 I)^-1 [e_p; e_r] with J the 6 x
 * n_active Jacobian at p (rows 3-5 zero without an orientation); dq scaled uniformly so that max|dq| <= max_step; q += dq; limited joints
 * clamped to their range.  At most max_iters iterations (<= JACO_IK_MAX_ITERS).
 * Inputs (device): qpos_seed_dev [num_envs][nq] (NULL = the handle's current state), target_pos_dev [num_envs][3], target_quat_dev
 * [num_envs][4] (NULL = position only).  Outputs (device): qpos_out_dev [num_envs][nq] = the seed row with the active dofs replaced,
 * every other word copied bit for bit (it may be the seed buffer itself); resid_dev [num_envs][2] = |e_p|, |e_r| of the last evaluation
 * (or NULL); status_dev [num_envs][2] int32 = iterations taken, converged 0 / 1 (or NULL).  opt_host NULL = the defaults of
 * JACO_IK_DEFAULTS.  Nothing of the handle is written: the caller applies the result with jaco_set_state.
 * Asynchronous on `stream` (the handle owns no stream: as every launching call it takes the caller's): one kernel launch, no allocation,
 * no synchronisation, no host copy (frame and options travel in the kernel arguments).
 * JACO_EINVAL for a frame body outside [-1, fused bodies), max_iters outside [0, JACO_IK_MAX_ITERS], a non-positive tolerance, damping
 * or max_step, an empty active set (a world-fixed frame, a free body's frame) and a NULL target position or output. */
#define JACO_IK_MAX_ITERS 256
typedef struct JacoIkOptions {
  float tol_pos, tol_rot;   /* m, rad */
  float damping, max_step;  /* lambda; rad */
  int32_t max_iters, reserved;
  uint64_t dof_mask;        /* 0 = every hinge dof on the frame's chain */
} JacoIkOptions;
#define JACO_IK_DEFAULTS {1e-5f, 1e-4f, 0.02f, 0.3f, 60, 0, 0}
int jaco_ik(JacoHandle* h, const JacoFrame* frame_host, const JacoIkOptions* opt_host, const float* qpos_seed_dev,
            const float* target_pos_dev, const float* target_quat_dev, float* qpos_out_dev, float* resid_dev, int32_t* status_dev, void* stream);

/* ---- operational-space controller: which torques drive this frame towards this pose?  abr_control's OSC(robot_config, kp, ko, kv,
 * vmax).generate() (env_mujoco_util.py:59-63, 85-90) for up to JACO_OSC_MAX_FRAMES frames per env, all of it in one kernel launch
 * (mujoco_jaco_amd/csrc/osc.h).  For each env and each frame f, with the values of a sim.forward() on the given state -- fresh, not one
 * substep stale as the reference's controller reads them; a caller who wants that lag computes from the previous state:
 *   p, R = the frame's point and orientation, composed as jaco_query composes them;  J = the 6 x n Jacobian at p on the frame's active
 *   dofs;  M = the n x n submatrix of qM on those dofs (the reference's M[arm, arm]; not a Schur complement);  bias = qfrc_bias there;
 *   Mx = (J M^-1 J^T)^-1 when |det| >= 1e-3, else the pseudo-inverse that drops singular values < 0.005;
 *   u_task = [p - p*; -vec(q* conj(q_R)) sign(w)], its two halves scaled down to the norms vmax_xyz / kp * kv and vmax_abg / ko * kv
 *   when they exceed them, then multiplied by kp and ko;      u = -kv M dq - J^T Mx u_task + bias.
 * Active dofs of a frame: the hinge dofs on the chain of the frame's body, intersected with dof_mask (bit d = dof d) when that is
 * non-zero; 1 <= n <= 6.  With n < 6 the 6 x 6 rule is applied to the rank-deficient matrix as it stands (M padded with identity, J with
 * zero columns): its determinant is 0, the pseudo-inverse branch runs and the status is 1.
 * Inputs (device): qpos_dev [num_envs][nq] / qvel_dev [num_envs][nv] (NULL = the handle's current state, the fp32 words jaco_get_state
 * returns); target_pos_dev [num_envs][nframes][3]; target_quat_dev [num_envs][nframes][4] (unit quaternions, w first; normalised again
 * in the kernel); ctrl_in_dev [num_envs][nu] (NULL = zeros).  Outputs (device): ctrl_out_dev [num_envs][nu] = the ctrl_in row with u_d
 * written at the motor actuator of every active dof d and every other word copied bit for bit (gripper commands, the other arm); it may
 * be ctrl_in_dev itself.  No clamping here: the step's actuator stage applies ctrlrange / forcerange.  status_dev [num_envs][nframes]
 * int32 (or NULL): 1 = the pseudo-inverse branch ran.  opt_host NULL = JACO_OSC_DEFAULTS (the reference's gains).
 * Nothing of the handle is written.  Asynchronous on `stream`: one kernel launch, no allocation, no synchronisation, no host copy (frames
 * and options travel in the kernel arguments).
 * JACO_EINVAL for nframes outside [1, JACO_OSC_MAX_FRAMES], a frame body outside [0, fused bodies), an empty active set or one larger
 * than 6, active sets of two frames that overlap, an active dof without a motor actuator, a non-positive gain or vmax, NULL targets and
 * a NULL ctrl_out.  Task axes (abr_control's ctrlr_dof) and null-space terms: jaco_osc_task below. */
#define JACO_OSC_MAX_FRAMES 2
typedef struct JacoOscOptions {
  float kp, ko, kv;            /* 50, 180, 20 */
  float vmax_xyz, vmax_abg;    /* 0.4 m/s, 1.0472 rad/s */
  int32_t reserved;
  uint64_t dof_mask;           /* 0 = every hinge dof on the frame's chain */
} JacoOscOptions;
#define JACO_OSC_DEFAULTS {50.f, 180.f, 20.f, 0.4f, 1.0472f, 0, 0}
int jaco_osc(JacoHandle* h, const JacoFrame* frames_host, int nframes, const JacoOscOptions* opt_host, const float* qpos_dev,
             const float* qvel_dev, const float* target_pos_dev, const float* target_quat_dev, const float* ctrl_in_dev, float* ctrl_out_dev,
             int32_t* status_dev, void* stream);

/* ---- ... on chosen task axes, with null-space posture terms: abr_control's OSC(..., ctrlr_dof, null_controllers=[Damping, RestingConfig])
 * .generate(), one kernel launch (mujoco_jaco_amd/csrc/osc_task.h).  Everything is as in jaco_osc -- p, R, J, M, bias, the active dofs,
 * the inputs, ctrl_out and its aliasing, the normalisation of target_quat, status, "nothing of the handle is written" -- except:
 *   rows = the task rows that axes[f] selects (bit 0-2: the world x, y, z rows of J; bit 3-5: the three rotational rows; 0 = all six),
 *   k of them, 1 <= k <= 6;  Js = J[rows] (k x n; abr_control's J[ctrlr_dof]);
 *   Mx = (Js M^-1 Js^T)^-1 when n >= k and |det| >= 1e-3, else the pseudo-inverse that drops singular values < 0.005 (status 1); with
 *   n < k the matrix is exactly rank deficient and the pseudo-inverse always runs;
 *   u_task = [p - p*; -vec(q* conj(q_R)) sign(w)], each half saturated on the norm of its full three components and multiplied by its
 *   gain exactly as in jaco_osc, and only then reduced to the selected rows (abr_control's order);
 *   u = -kv M dq - Js^T Mx u_task[rows] + bias;
 *   u_null = -null_kv M dq                          (Damping; off when null_kv == 0)
 *          + M (rest_kp e - rest_kv v)              (RestingConfig; on when rest_qpos_dev != NULL), where for every active dof d that
 *            rest_mask selects (bit d = dof d; 0 = every active dof) e_d = ((rest_d - q_d + pi) mod 2 pi) - pi in [-pi, pi) (floor-style
 *            modulus) and v_d = dq_d, and e_d = v_d = 0 for the others;
 *   u += u_null - Js^T Mx (Js (M^-1 u_null))        (the null-space filter (I - Js^T Jbar^T) with Jbar = M^-1 Js^T Mx; the same Mx).
 * rest_qpos_dev [num_envs][nq] fp32 is read only at the qpos addresses of the selected dofs: a jaco_ik result row can be handed in as it
 * is.  target_quat_dev may be NULL when no frame selects a rotational row; it is not read then.  task_host NULL = jaco_osc itself (the
 * call forwards to it; rest_qpos_dev is ignored).  One kernel launch, no allocation, no synchronisation, no host copy.
 * JACO_EINVAL for everything jaco_osc refuses, and for an axes word with bits above bit 5, a negative or non-finite null_kv, rest_kp or
 * rest_kv, a rest_mask that leaves no active dof of some frame while rest_qpos_dev is given, and a NULL target_quat_dev with a
 * rotational row selected. */
typedef struct JacoOscTask {
  uint32_t axes[JACO_OSC_MAX_FRAMES]; /* bit r = task row r (x y z, then the three rotational rows); 0 = all six */
  float null_kv;                      /* >= 0; 0 = no damping term */
  float rest_kp, rest_kv;             /* >= 0; used when rest_qpos_dev is given */
  int32_t reserved;
  uint64_t rest_mask;                 /* dofs held by the resting term; 0 = every active dof */
} JacoOscTask;
int jaco_osc_task(JacoHandle* h, const JacoFrame* frames_host, int nframes, const JacoOscOptions* opt_host, const JacoOscTask* task_host,
                  const float* qpos_dev, const float* qvel_dev, const float* target_pos_dev, const float* target_quat_dev,
                  const float* rest_qpos_dev, const float* ctrl_in_dev, float* ctrl_out_dev, int32_t* status_dev, void* stream);

/* ---- joint-space controller and inverse dynamics: which torques drive the arm to this configuration?  abr_control's
 * Joint(robot_config, kp, kv).generate(q, dq, target, target_velocity) with a feed-forward acceleration, for any set of motor-driven hinge
 * dofs, in one kernel launch (mujoco_jaco_amd/csrc/joint.h).  For each env, with the values of a sim.forward() on the given state (qM,
 * qfrc_bias) and the active dof set A = the dofs of dof_mask (bit d = dof d), or every hinge dof with a motor actuator when that is 0 --
 * not limited to six: the two-arm model's twelve go in one call:
 *   e_d = q*_d - q_d for a limited joint; e_d = ((q*_d - q_d + pi) mod 2 pi) - pi in [-pi, pi) (floor-style modulus) for an unlimited
 *         one.  abr_control wraps every joint; a limited joint is never wrapped here, so that a long move (Jaco joint 2: 260 degrees)
 *         is not sent the short way through the limit.  e = 0 without target_qpos_dev;
 *   s   = min(1, (vmax kv / kp) / max over A of |e_d|) when vmax > 0 and kp > 0, else 1: one scale for every dof (the move stays a
 *         straight line in joint space);
 *   a_d = qacc_ff_d + kp s e_d + kv (dq*_d - dq_d) for d in A, 0 for every other dof; a NULL input counts as zeros;
 *   u_d = sum over k in A of M[d][k] a_k + qfrc_bias_d,  M the submatrix of qM on A (as in jaco_osc; not a Schur complement).
 * Joint damping is not compensated.  Modes: kp = kv = 0 with qacc_ff_dev is inverse dynamics (the torques for a wanted joint
 * acceleration); kp = kv = 0 with no target and no qacc_ff_dev is bias compensation (u = qfrc_bias on A; abr_control's Floating); kp = 0,
 * kv > 0 without targets adds the damping -kv M dq to it.
 * Inputs (device): qpos_dev / qvel_dev as in jaco_osc (NULL = the handle's state); target_qpos_dev [num_envs][nq] (or NULL), read only
 * at the qpos addresses of the active dofs, so a jaco_ik result row goes in as it is; target_qvel_dev, qacc_ff_dev [num_envs][nv] (or
 * NULL); ctrl_in_dev [num_envs][nu] (NULL = zeros).  Output: ctrl_out_dev [num_envs][nu] = the ctrl_in row with u_d at the motor
 * actuator of every active dof and every other word copied bit for bit; it may be ctrl_in_dev itself.  No clamping.  opt_host NULL =
 * JACO_JOINT_DEFAULTS.  Nothing of the handle is written.  Asynchronous on `stream`: one kernel launch, no allocation, no
 * synchronisation, no host copy.
 * JACO_EINVAL for a dof_mask bit on a free-joint dof, on a dof without a motor actuator (the finger position servos) or at or beyond nv,
 * an empty active set, a negative or non-finite kp, kv or vmax, kp > 0 with a NULL target_qpos_dev, and a NULL ctrl_out_dev. */
typedef struct JacoJointOptions {
  float kp, kv;        /* >= 0, finite; 50, 20 */
  float vmax;          /* rad/s, >= 0; 0 = no limiting */
  int32_t reserved;
  uint64_t dof_mask;   /* 0 = every hinge dof that has a motor actuator */
} JacoJointOptions;
#define JACO_JOINT_DEFAULTS {50.f, 20.f, 0.f, 0, 0}
int jaco_joint(JacoHandle* h, const JacoJointOptions* opt_host, const float* qpos_dev, const float* qvel_dev, const float* target_qpos_dev,
               const float* target_qvel_dev, const float* qacc_ff_dev, const float* ctrl_in_dev, float* ctrl_out_dev, void* stream);

/* ---- forward dynamics and its linearisation: given state and ctrl, which acceleration results, and how does it change with the state
 * and the ctrl?  MuJoCo's data.qacc_smooth / data.qfrc_smooth after mj_forward and a contact-free mjd_transitionFD, for every env in one
 * kernel launch (mujoco_jaco_amd/csrc/fd.h).  The values are those of a sim.forward() on the given state, per env:
 *   qfrc_smooth = qfrc_passive - qfrc_bias + qfrc_actuator.  Passive: joint damping, and springs where the model has them.  Actuator:
 *                 the step kernel's own actuation stage -- ctrl clamped to ctrlrange, kp (c - q) for the position servos (the fingers),
 *                 then forcerange;
 *   qacc        = M^-1 qfrc_smooth (implicit_damping 0: mj_forward's qacc_smooth), or (M + h D)^-1 qfrc_smooth (implicit_damping 1: what
 *                 the Euler stage applies when no constraint row is active; h the model's timestep, D = diag(joint damping) on the
 *                 damped dof block), solved with the step kernel's block-diagonal elimination.
 * The acceleration is UNCONSTRAINED: no contact rows and no joint-limit rows enter it.
 * Inputs (device): qpos_dev / qvel_dev as in jaco_query (NULL = the handle's fp32 state); ctrl_dev [num_envs][nu] (NULL = zeros).
 * Outputs (device, fp32; each pointer of JacoFdOut may be NULL, its work is skipped).  The derivative outputs hold one contiguous row
 * per perturbation:
 *   qacc, qfrc_smooth [num_envs][nv];
 *   dqacc_dqpos [num_envs][nv][nv]: entry [c][d] = d qacc_d / d q_c (the TRANSPOSED Jacobian) for hinge dof c: a central difference with
 *                 the whole chain re-evaluated at q_c +- eps_qpos (tree walk, mass matrix, bias, passive, actuation -- the servos see
 *                 the moved joint --, solve), divided by the actual difference of the two rounded fp32 coordinates;
 *   dqacc_dqvel [num_envs][nv][nv]: the same for qvel_c +- eps_qvel.  qacc is exactly quadratic in qvel, so this difference has no
 *                 truncation error: its default step is large;
 *   rows c of both that dof_mask (bit c = dof c; 0 = every hinge dof) does not select are written as zeros.  Free-joint dofs cannot be
 *                 selected;
 *   dqacc_dctrl [num_envs][nu][nv]: row a = d qacc / d ctrl_a, analytic: g_a (M or M + h D)^-1 e_dof(a), g_a = kp of a position servo,
 *                 1 of a motor; exactly 0.0 when ctrl_a lies outside its (limited) ctrlrange or the actuator force sits at a forcerange end.
 * opt_host NULL = JACO_FD_DEFAULTS.  Nothing of the handle is written.  Asynchronous on `stream`: one kernel launch, no allocation, no
 * synchronisation, no host copy.
 * JACO_EINVAL for a NULL out or all five outputs NULL, a non-positive or non-finite eps, a dof_mask bit at or beyond nv or on a
 * free-joint dof, and an implicit_damping other than 0 / 1. */
typedef struct JacoFdOptions {
  float eps_qpos, eps_qvel;      /* rad, rad/s: half-width of the central differences; > 0, finite */
  int32_t implicit_damping;      /* 0: qacc = M^-1 qfrc_smooth; 1: qacc = (M + h D)^-1 qfrc_smooth */
  int32_t reserved;
  uint64_t dof_mask;             /* dofs perturbed for the derivative outputs; 0 = every hinge dof */
} JacoFdOptions;
#define JACO_FD_DEFAULTS {0.00390625f, 0.125f, 0, 0, 0}     /* 2^-8 rad, 2^-3 rad/s */
typedef struct JacoFdOut { float* qacc; float* qfrc_smooth; float* dqacc_dqpos; float* dqacc_dqvel; float* dqacc_dctrl; } JacoFdOut;
int jaco_fd(JacoHandle* h, const JacoFdOptions* opt_host, const float* qpos_dev, const float* qvel_dev, const float* ctrl_dev,
            const JacoFdOut* out, void* stream);

/* ---- open-loop rollouts: what happens over the next nknots * hold substeps if this ctrl sequence is applied from this state?
 * mujoco.rollout.rollout(model, data, initial_state, control), contact-free, for n rollouts in ONE kernel launch
 * (mujoco_jaco_amd/csrc/rollout.h): one wavefront per rollout runs the whole loop with the state in LDS and registers.
 * Rollout i starts from state row state_idx_dev[i] (int32 [n]; NULL = row i, so n <= nstates) of qpos0_dev [nstates][nq] / qvel0_dev
 * [nstates][nv] (both given, or both NULL = the handle's fp32 state with nstates = num_envs).  The state is exactly the floats handed
 * in (low-order words zero, as in jaco_query) and qacc_warmstart starts at zero.  K candidate sequences per env share one state row
 * through the index; n is NOT tied to num_envs, and nothing of the handle is read but the model (and its state when no override is
 * given).  Knot k holds the row ctrl_dev[i][k][:] ([n][nknots][nu]) for `hold` substeps.
 * Every substep is the contact-free substep of jaco_physics_step -- what a real step does under option "disable_contact", the same
 * stages in the same order: tree walk, mass matrix and bias, the actuators (ctrlrange, the fingers' position servos, forcerange), the
 * joint-limit rows and their Newton solve warm-started from the previous substep's qacc, Euler with implicit joint damping on the
 * compensated pair (option "compensated"), the position update.  Joint limits are in, CONTACTS ARE NOT; free bodies are integrated like
 * everything else, so they fall.  The solver options are the model's, as the handle has them at the call.
 * Outputs (device, fp32; each pointer of JacoRolloutOut may be NULL, at least one of the first four is required), written after the last
 * substep of knot k into row k:
 *   qpos [n][nknots][nq], qvel [n][nknots][nv]: the fp32 state, as jaco_get_state would return it;
 *   xpos [n][nknots][3], xmat [n][nknots][9]: the pose of the one frame frame_host (NULL: no pose outputs) at that state, composed as
 *                 jaco_query composes frames -- the EE trajectory a sampling planner costs;
 *   status [n] uint32: JACO_FLAG_NAN / JACO_FLAG_SOLVER_MAXITER, sticky over the rollout with the step kernel's rules (the rollout
 *                 goes on, as the step does), or JACO_ROLLOUT_BAD_INDEX.
 * final_only = 1: the arrays have ONE knot row ([n][1][..]) holding the last knot (terminal-cost planners).
 * A state_idx entry outside [0, nstates) is handled as jaco_load_envs handles one: that rollout writes only its status word, with
 * JACO_ROLLOUT_BAD_INDEX set, and leaves its output rows untouched.
 * Nothing of the handle is written.  Asynchronous on `stream`: one kernel launch (none for n == 0, which returns JACO_OK), no
 * allocation, no synchronisation, no host copy; the options and the frame travel in the kernel arguments.
 * JACO_EINVAL, with no output touched, for NULL options; nknots < 1, hold < 1 or nknots * hold > JACO_ROLLOUT_MAX_SUBSTEPS; final_only
 * not 0 / 1; n < 0; a NULL ctrl_dev; a NULL out or all four state / pose outputs NULL; xpos or xmat without a frame; a frame body
 * outside [-1, fused bodies); only one of qpos0_dev / qvel0_dev; nstates != num_envs with the handle's state; nstates < 1 with an
 * override; n > nstates with a NULL state_idx_dev. */
#define JACO_ROLLOUT_MAX_SUBSTEPS 16384        /* nknots * hold */
#define JACO_ROLLOUT_BAD_INDEX 0x80000u
typedef struct JacoRolloutOptions {
  int32_t nknots;       /* >= 1 */
  int32_t hold;         /* substeps per knot, >= 1; 1 */
  int32_t final_only;   /* 0 / 1 */
  int32_t reserved;
} JacoRolloutOptions;
typedef struct JacoRolloutOut { float* qpos; float* qvel; float* xpos; float* xmat; uint32_t* status; } JacoRolloutOut;
int jaco_rollout(JacoHandle* h, const JacoRolloutOptions* opt_host, const JacoFrame* frame_host, int n, const int32_t* state_idx_dev, int nstates,
                 const float* qpos0_dev, const float* qvel0_dev, const float* ctrl_dev, const JacoRolloutOut* out, void* stream);

/* ---- closed-loop rollouts: jaco_rollout with the ctrl of knot k computed inside the kernel from the state at knot k -- the forward
 * pass of iLQR and its line search (u_k = ubar_k + alpha k_k + K_k (x_k - xbar_k)), a plan tracked with TVLQR gains, PD tracking of a joint
 * trajectory, a feedback plan tried from many perturbed starts -- for n rollouts in ONE kernel launch
 * (mujoco_jaco_amd/csrc/rollout_fb.h).  The state arguments (state_idx_dev, nstates, qpos0_dev, qvel0_dev), the substep, the outputs
 * qpos / qvel / xpos / xmat / status, final_only and n == 0 are those of jaco_rollout, word for word.
 * Plans (JacoRolloutPlan, a host record of device pointers): rollout i follows plan p = plan_idx[i] (int32 [n]; NULL = plan i, so
 * n <= nplans); many rollouts share one plan through the index, as they share states.  With nd = ndofs and nx = 2 nd:
 *   ctrl  [nplans][nknots][nu]      the nominal ctrl rows (required);
 *   kff   [nplans][nknots][nu]      the feed-forward step, or NULL;
 *   gain  [nplans][nknots][nu][nx]  the feedback gains, row a = actuator a, or NULL;
 *   xref  [nplans][nknots][nx]      the reference states (required with gain);
 *   alpha [n]                       the line-search step of rollout i, or NULL = 1.0f (needs kff).
 * THE LAW, at an evaluation in knot k; this order of fp32 operations is part of the interface:
 *   x_j = qpos[qposadr(dofs[j])] for j < nd, qvel[dofs[j - nd]] for nd <= j < nx   (the fp32 state, as jaco_get_state would return it)
 *   d_j = x_j - xref[p][k][j]                                                       (one subtraction; NOT wrapped: the law is a local
 *                                                                                    one about a continuous reference)
 *   u_a = kff ? fmaf(alpha_i, kff[p][k][a], ctrl[p][k][a]) : ctrl[p][k][a]
 *   u_a = fmaf(gain[p][k][a][j], d_j, u_a)   for j = 0 .. nx-1, ascending           (gain NULL: skipped)
 * for every actuator a = 0 .. nu-1.  u is the commanded ctrl; the actuator stage clamps it to ctrlrange afterwards, as it clamps any
 * ctrl.  per_substep = 0: the law is evaluated before the first substep of a knot and held for the knot (zero-order hold);
 * per_substep = 1: before every substep, against the same knot's rows.  dofs: ndofs distinct hinge dofs (used only when gain is given).
 * Output ctrl [n][E][nu], E = nknots (per_substep = 0) or nknots * hold: the u of every evaluation, as commanded (before the clamp) --
 * iLQR's new nominal.  It has all E rows whether or not final_only is set.  ctrl counts as an output: at least one of the six pointers
 * of JacoRolloutFbOut is required.
 * A state_idx or plan_idx entry out of range: that rollout writes only its status word, with JACO_ROLLOUT_BAD_INDEX set.
 * Nothing of the handle is written.  Asynchronous on `stream`: one kernel launch (none for n == 0, which returns JACO_OK), no
 * allocation, no synchronisation, no host copy; the options (the dof list included) and the frame travel in the kernel arguments.
 * JACO_EINVAL, with no output touched, for everything jaco_rollout refuses (the ctrl sequences being plan->ctrl, the outputs the six)
 * and for a NULL plan; nplans < 1; n > nplans with a NULL plan_idx; gain without xref; alpha without kff; per_substep not 0 / 1; with
 * gain: ndofs outside [1, JACO_ROLLOUT_FB_MAX_DOFS], a dof outside [0, nv), a dof of a free joint, a dof listed twice. */
#define JACO_ROLLOUT_FB_MAX_DOFS 18
typedef struct JacoRolloutFbOptions {
  int32_t nknots, hold, final_only, per_substep;  /* as JacoRolloutOptions; per_substep 0 / 1 */
  int32_t ndofs;                                  /* 1 .. MAX_DOFS; used only when gain is given */
  int32_t dofs[JACO_ROLLOUT_FB_MAX_DOFS];         /* distinct hinge dofs */
  int32_t reserved;
} JacoRolloutFbOptions;
typedef struct JacoRolloutPlan {                  /* device pointers */
  const float* ctrl;   /* [nplans][nknots][nu]       required */
  const float* kff;    /* [nplans][nknots][nu]       or NULL */
  const float* gain;   /* [nplans][nknots][nu][nx]   or NULL */
  const float* xref;   /* [nplans][nknots][nx]       required with gain */
  const float* alpha;  /* [n]                        or NULL (needs kff) */
  const int32_t* plan_idx; /* [n] or NULL: plan i, so n <= nplans */
  int32_t nplans;
} JacoRolloutPlan;
typedef struct JacoRolloutFbOut { float* qpos; float* qvel; float* xpos; float* xmat; uint32_t* status; float* ctrl; } JacoRolloutFbOut;
int jaco_rollout_fb(JacoHandle* h, const JacoRolloutFbOptions* opt_host, const JacoFrame* frame_host, int n, const int32_t* state_idx_dev, int nstates,
                    const float* qpos0_dev, const float* qvel0_dev, const JacoRolloutPlan* plan_host, const JacoRolloutFbOut* out, void* stream);

/* ---- costed rollouts: jaco_rollout_fb with a per-rollout additive perturbation of the commanded ctrl and a running quadratic cost
 * accumulated inside the kernel -- what a sampling planner (MPPI, CEM, random shooting) and iLQR's line search want of a rollout: one
 * number, not the trajectory -- for n rollouts in ONE kernel launch (mujoco_jaco_amd/csrc/rollout_cost.h).  The state arguments, the
 * plans (JacoRolloutPlan), the law, the substep, the six outputs of JacoRolloutFbOut, final_only and n == 0 are those of
 * jaco_rollout_fb, word for word, with per_substep = 0: the law is evaluated once per knot.
 * THE COMMANDED CTRL, at knot k of rollout i on plan p: u_a is the law's value in its stated fp32 order; then, if noise is given,
 *   u_a = u_a + noise[i][k][a]                                                      (ONE fp32 add; this order is part of the interface)
 * The sum is what the actuators get and what the ctrl output ([n][nknots][nu], before the actuator clamp) holds.
 * THE COST.  With x the fp32 state on the option's dofs (the law's x_j, nx = 2 ndofs), pos the frame's position, T = nknots and
 * g = goal_per_knot ? k : 0:
 *   J_i = sum_{k=0}^{T-1} [ 1/2 sum_a wu[a] u_{k,a}^2 + 1/2 sum_j WX_k[j] (x_{k+1,j} - xgoal[p][g][j])^2 + 1/2 WP_k |pos_{k+1} - pgoal[p][g]|^2 ]
 * where x_{k+1} and pos_{k+1} are the state and the pose after knot k -- the very words row k of the qpos / qvel / xpos outputs holds --
 * and (WX_k, WP_k) = (wx, wp) for k < T - 1, (wxT, wpT) for the last knot.  Differences are NOT wrapped, as in the law.  The fp32 order
 * of the sum is not part of the interface; that two runs of the same call agree bit for bit is, and that cost and terms do not depend
 * on final_only or on which other outputs are asked for.
 * Goals and noise (JacoRolloutGoal, a host record of device pointers, each optional; a NULL record is three NULLs): goals are indexed by
 * the plan index p: xgoal [nplans][G][nx], pgoal [nplans][G][3], G = goal_per_knot ? nknots : 1; noise [n][nknots][nu].
 * The weights travel by value in the options; all must be finite and >= 0, so that every term is non-negative.  The dofs are used when
 * gain is given or a state weight (wx, wxT) is non-zero.  The pose of a knot is composed whenever a pose weight asks for it, whether or
 * not xpos / xmat are asked for.
 * Outputs: the six of JacoRolloutFbOut, plus cost [n] and terms [n][3] = the ctrl, state and pose parts of J (their sum is cost to
 * rounding); at least one of the eight is required; the usual call passes cost and status.  A rollout whose status has JACO_FLAG_NAN gets
 * cost = terms = +inf, so that a softmin ignores it.  A state_idx or plan_idx entry out of range: that rollout writes only its status
 * word, with JACO_ROLLOUT_BAD_INDEX set.
 * Nothing of the handle is written.  Asynchronous on `stream`: one kernel launch (none for n == 0, which returns JACO_OK), no
 * allocation, no synchronisation, no host copy; the options (dofs and weights included) and the frame travel in the kernel arguments.
 * JACO_EINVAL, with no output touched, for everything jaco_rollout_fb refuses (there is no per_substep; the outputs being the eight) and
 * for goal_per_knot not 0 / 1; a model with nu > JACO_ROLLOUT_COST_MAX_NU; a weight that is negative or not finite; a non-zero state
 * weight without xgoal or (gain not given) without dofs -- the dofs then checked as jaco_rollout_fb checks them; a non-zero pose weight
 * without pgoal or without a frame. */
#define JACO_ROLLOUT_COST_MAX_NU 18
typedef struct JacoRolloutCostOptions {
  int32_t nknots, hold, final_only, goal_per_knot;  /* as JacoRolloutOptions; goal_per_knot 0 / 1 */
  int32_t ndofs;                                    /* 1 .. JACO_ROLLOUT_FB_MAX_DOFS; used with gain or a non-zero state weight */
  int32_t dofs[JACO_ROLLOUT_FB_MAX_DOFS];           /* distinct hinge dofs */
  float wx[2 * JACO_ROLLOUT_FB_MAX_DOFS];           /* running state weights, word j of x */
  float wxT[2 * JACO_ROLLOUT_FB_MAX_DOFS];          /* the last knot's */
  float wu[JACO_ROLLOUT_COST_MAX_NU];               /* ctrl weights, actuator a */
  float wp, wpT;                                    /* running and last-knot pose weight */
  int32_t reserved;
} JacoRolloutCostOptions;
typedef struct JacoRolloutGoal {                    /* device pointers, each or NULL */
  const float* noise;  /* [n][nknots][nu] */
  const float* xgoal;  /* [nplans][G][nx] */
  const float* pgoal;  /* [nplans][G][3] */
} JacoRolloutGoal;
typedef struct JacoRolloutCostOut { float* qpos; float* qvel; float* xpos; float* xmat; uint32_t* status; float* ctrl; float* cost; float* terms; } JacoRolloutCostOut;
int jaco_rollout_cost(JacoHandle* h, const JacoRolloutCostOptions* opt_host, const JacoFrame* frame_host, int n, const int32_t* state_idx_dev, int nstates,
                      const float* qpos0_dev, const float* qvel0_dev, const JacoRolloutPlan* plan_host, const JacoRolloutGoal* goal_host,
                      const JacoRolloutCostOut* out, void* stream);

/* ---- rollouts under the operational-space controller: jaco_rollout with the motor words of the ctrl computed inside the kernel by
 * jaco_osc's law towards a plan of frame targets -- "where is the hand after 50 substeps of driving towards this pose?", the rollout of
 * a planner that samples end-effector targets, the env's own substep loop (OSC towards a target, then a substep) -- for n rollouts in
 * ONE kernel launch (mujoco_jaco_amd/csrc/rollout_osc.h).  The state arguments (state_idx_dev, nstates, qpos0_dev, qvel0_dev), the
 * substep, the outputs qpos / qvel / xpos / xmat, final_only and n == 0 are those of jaco_rollout, word for word; the frames, their
 * active dofs, the gains and the law are those of jaco_osc.
 * Plans (JacoRolloutOscPlan, a host record of device pointers): rollout i follows plan p = plan_idx[i] (int32 [n]; NULL = plan i, so
 * n <= nplans); K target samples of one env share its state row through state_idx, and rollouts share plans through plan_idx:
 *   ctrl        [nplans][nknots][nu]           the base ctrl rows, or NULL = zeros: gripper commands and the other arm's words;
 *   target_pos  [nplans][nknots][nframes][3]   the target of frame f in knot k (required);
 *   target_quat [nplans][nknots][nframes][4]   unit quaternions, w first, normalised again in the kernel (required).
 * THE LAW, at an evaluation in knot k: the row ctrl[p][k] with, for every frame f, jaco_osc's u_d (same formula, same fp32 code, on
 * frames_host[f], target_pos[p][k][f], target_quat[p][k][f] and the options' gains) written at the motor actuator of every active dof d;
 * every other word goes through bit for bit.  It is evaluated INSIDE the substep, on that substep's own mass matrix, bias and body
 * poses -- fresh, as jaco_osc's are on the state it is handed, not one substep stale as the reference's controller reads them -- so it
 * costs no forward pass of its own.  per_substep = 1: before every substep's actuator stage (the env's own loop); per_substep = 0: in
 * the first substep of a knot, held over the knot.  The actuator stage clamps u afterwards, as it clamps any ctrl.
 * Outputs (JacoRolloutFbOut; at least one of the six pointers is required): qpos, qvel, xpos, xmat as jaco_rollout -- the pose of the
 * ONE frame out_frame_host (NULL: no pose outputs), which may or may not be a controlled frame -- and
 *   ctrl [n][E][nu], E = nknots (per_substep = 0) or nknots * hold: the commanded row of every evaluation (before the clamp), all E rows
 *                 whether or not final_only is set;
 *   status [n] uint32: JACO_FLAG_NAN / JACO_FLAG_SOLVER_MAXITER as jaco_rollout, JACO_ROLLOUT_OSC_SINGULAR0 / _SINGULAR1 when any
 *                 evaluation of frame 0 / 1 took the pseudo-inverse branch (jaco_osc's status), or JACO_ROLLOUT_BAD_INDEX.
 * A state_idx or plan_idx entry out of range: that rollout writes only its status word, with JACO_ROLLOUT_BAD_INDEX set.
 * Not here: task axes and null-space terms (jaco_osc_task), an in-kernel cost, contacts -- the prediction is jaco_rollout's, the arm in
 * free space with joint limits.
 * Nothing of the handle is written.  Asynchronous on `stream`: one kernel launch (none for n == 0, which returns JACO_OK), no
 * allocation, no synchronisation, no host copy; the options and the frames travel in the kernel arguments.
 * JACO_EINVAL, with no output touched, for everything jaco_rollout refuses (a NULL plan->ctrl is NOT refused; the outputs being the
 * six); a NULL plan; per_substep not 0 / 1; nplans < 1; n > nplans with a NULL plan_idx; the options' nframes != nframes; and for
 * everything jaco_osc refuses of frames, gains and active sets, the arrays required being target_pos and target_quat. */
#define JACO_ROLLOUT_OSC_SINGULAR0 0x200000u   /* status: frame 0 used the pseudo-inverse branch at some evaluation */
#define JACO_ROLLOUT_OSC_SINGULAR1 0x400000u   /* ... frame 1 */
typedef struct JacoRolloutOscOptions {
  int32_t nknots, hold, final_only, per_substep;  /* as JacoRolloutFbOptions */
  int32_t nframes;                                /* 1 .. JACO_OSC_MAX_FRAMES: the frames of a target row */
  int32_t reserved;
  float kp, ko, kv, vmax_xyz, vmax_abg;           /* as JacoOscOptions: 50, 180, 20, 0.4, 1.0472 */
  uint64_t dof_mask;                              /* 0 = every hinge dof on the frame's chain */
} JacoRolloutOscOptions;
typedef struct JacoRolloutOscPlan {               /* device pointers */
  const float* ctrl;         /* [nplans][nknots][nu]            or NULL: zeros */
  const float* target_pos;   /* [nplans][nknots][nframes][3]    required */
  const float* target_quat;  /* [nplans][nknots][nframes][4]    required */
  const int32_t* plan_idx;   /* [n] or NULL: plan i, so n <= nplans */
  int32_t nplans;
} JacoRolloutOscPlan;
int jaco_rollout_osc(JacoHandle* h, const JacoRolloutOscOptions* opt_host, const JacoFrame* frames_host, int nframes, const JacoFrame* out_frame_host, int n,
                     const int32_t* state_idx_dev, int nstates, const float* qpos0_dev, const float* qvel0_dev, const JacoRolloutOscPlan* plan_host,
                     const JacoRolloutFbOut* out, void* stream);

/* ---- the iLQR / TVLQR backward pass, batched: the feed-forward k_t and the gains K_t that jaco_rollout_fb consumes, from the linearisation
 * (jaco_fd) and the cost expansion along a trajectory, the whole T-knot recursion of every problem in ONE launch.
 * Solve i works on problem p = prob_idx[i] and runs t = T-1 .. 0.  Deviations follow dx_{t+1} = A_t dx_t + B_t du_t; the knot cost is
 * 1/2 dx'lxx dx + 1/2 du'luu du + du'lux dx + lx'dx + lu'du, the terminal cost 1/2 dx'Vxx dx + Vx'dx.  At each knot:
 *   Qx = lx + A'Vx          Qu = lu + B'Vx
 *   Qxx = lxx + A'Vxx A     Qux = lux + B'Vxx A     Quu = luu + B'Vxx B
 *   L L' = Quu + mu_i I                    (Cholesky; a pivot <= 0 or a non-finite number: status = JACO_LQR_NOT_PD | t, the solve stops)
 *   K = -(Quu + mu I)^-1 Qux               k = -(Quu + mu I)^-1 Qu
 *   dV1 += k'Qu                            dV2 += 1/2 k'Quu k                     (Quu unregularised here and below)
 *   Vx  = Qx  + K'Quu k + K'Qu  + Qux'k
 *   Vxx = Qxx + K'Quu K + K'Qux + Qux'K;   Vxx = 1/2 (Vxx + Vxx')
 * in jaco_rollout_fb's sign convention: u = u_ref + alpha k + K (x - x_ref).  With mu = 0, lux = lx = lu = NULL, lxx = Q, luu = R and
 * Vxx = Qf, K is the finite-horizon LQR gain.  The fp32 order of operations is NOT part of the interface; that two runs of the same
 * call agree bit for bit is.  A NULL lux / lx / lu / Vx gives what an array of zeros gives, bit for bit.
 * Arrays: every cost array is [nprob][T][..] unless its bit is set in shared_knots (no knot axis: one block per problem) and / or in
 * shared_probs (no problem axis); the terminal Vxx / Vx have no knot axis to begin with.  mu and prob_idx are per solve: one launch can
 * try a ladder of regularisations on every problem.  n is not tied to num_envs; the handle supplies the device, the stream rules and
 * jaco_last_error, the model is not read.
 * Outputs (each may be NULL; at least one of gain / kff / dV / Vxx0 / Vx0): gain [n][T][rows][nx] and kff [n][T][rows], rows = rows_out ?
 * rows_out : nu, control a in row row[a] (rows_out = 0: row a); rows that no control maps to are never written -- with rows_out = the
 * model's nu and row = the motor words the two arrays are JacoRolloutPlan.gain / .kff as they are.  dV [n][2] = (dV1, dV2): the model's
 * predicted cost change of a step alpha is alpha dV1 + alpha^2 dV2.  Vxx0 [n][nx][nx], Vx0 [n][nx]: the cost-to-go at knot 0.
 * status [n]: 0; JACO_LQR_BAD_INDEX (prob_idx out of range: only the status word is written); JACO_LQR_NOT_PD | t (the rows of the
 * knots > t are written, those of the knots <= t are not, neither are dV, Vxx0, Vx0).
 * Asynchronous: one launch, no allocation, no synchronisation, no host copy; n == 0 returns JACO_OK without a launch.  JACO_EINVAL with
 * nothing written: NULL options, problem or out; a dimension out of range; n < 0; nprob < 1; n > nprob without an index; a NULL
 * required array; all five value outputs NULL; rows_out outside [nu, 64] when non-zero; a row out of range or listed twice; a mask bit
 * outside the seven named. */
#define JACO_LQR_MAX_NX 36            /* = 2 * JACO_ROLLOUT_FB_MAX_DOFS */
#define JACO_LQR_MAX_NU 18
#define JACO_LQR_BAD_INDEX 0x80000u   /* = JACO_ROLLOUT_BAD_INDEX */
#define JACO_LQR_NOT_PD 0x100000u     /* Quu + mu I not positive definite, or non-finite, at knot (status & 0xffff) */
/* which cost arrays have no knot axis / no problem axis */
#define JACO_LQR_LXX 1u
#define JACO_LQR_LUU 2u
#define JACO_LQR_LUX 4u
#define JACO_LQR_LX 8u
#define JACO_LQR_LU 16u
#define JACO_LQR_VXX 32u
#define JACO_LQR_VX 64u
typedef struct JacoLqrOptions {
  int32_t nknots, nx, nu;            /* 1..JACO_ROLLOUT_MAX_SUBSTEPS, 1..JACO_LQR_MAX_NX, 1..JACO_LQR_MAX_NU */
  int32_t rows_out;                  /* row count of the gain / kff outputs; 0 = nu */
  int32_t row[JACO_LQR_MAX_NU];      /* used when rows_out != 0: control a goes to output row row[a]; distinct, in [0, rows_out) */
  uint32_t shared_knots, shared_probs;
} JacoLqrOptions;
typedef struct JacoLqrProblem {      /* device pointers */
  const float *A, *B;                /* [nprob][T][nx][nx], [nprob][T][nx][nu]   required */
  const float *lxx, *luu;            /* [nprob][T][nx][nx], [nprob][T][nu][nu]   required (axes dropped per the shared masks) */
  const float *lux, *lx, *lu;        /* [..][nu][nx], [..][nx], [..][nu]          or NULL = zero */
  const float *Vxx, *Vx;             /* terminal: [nprob][nx][nx] required; [nprob][nx] or NULL = zero */
  const float* mu;                   /* [n] or NULL = 0 */
  const int32_t* prob_idx;           /* [n] or NULL: solve i takes problem i, so n <= nprob */
  int32_t nprob;
} JacoLqrProblem;
typedef struct JacoLqrOut { float* gain; float* kff; float* dV; float* Vxx0; float* Vx0; uint32_t* status; } JacoLqrOut;
int jaco_lqr(JacoHandle* h, const JacoLqrOptions* opt_host, int n, const JacoLqrProblem* prob_host, const JacoLqrOut* out, void* stream);

/* ---- transition Jacobians of the rollout step: the A_t, B_t that jaco_lqr reads, from the very step the rollouts simulate.  MuJoCo's
 * mjd_transitionFD: finite differences of the step function itself -- `hold` contact-free substeps with joint-limit rows, their
 * warm-started Newton solve, the compensated Euler stage and the position update, exactly jaco_rollout's substep -- for n (state, ctrl)
 * pairs in ONE kernel launch (mujoco_jaco_amd/csrc/transition.h).  n is NOT tied to num_envs: the typical input is every knot of every
 * trajectory, straight from jaco_rollout_fb's outputs.
 * Inputs (device, fp32): qpos_dev [n][nq] and qvel_dev [n][nv], given together or both NULL = the handle's fp32 state, and then
 * n == num_envs; ctrl_dev [n][nu] (NULL = zeros).  An evaluation starts from a pair exactly as jaco_rollout starts from a state row (low
 * words zero, zero warm start) and holds the ctrl row for `hold` substeps: the nominal evaluation is jaco_rollout(nknots = 1, hold) bit
 * for bit.
 * Coordinates, with nd = ndofs, nx = 2 nd, na = nacts:  x_j = qpos[qposadr(dofs[j])] for j < nd, qvel[dofs[j - nd]] for nd <= j < nx
 * (jaco_rollout_fb's convention and limit);  u_a = ctrl[acts[a]].  Column c perturbs ONE word: x_c +- eps_qpos (c < nd), x_c +- eps_qvel
 * (c < nx) or u_(c - nx) +- eps_ctrl, formed in fp32.
 * THE INCREMENT FORM; this order of fp32 operations is part of the interface.  Every evaluation forms, for j < nx,
 *   D_j = (x'_j.hi - x_j.start) + x'_j.lo
 * x'.hi / x'.lo the compensated pair of the coordinate after the last substep, x_j.start the word the evaluation started from (the
 * perturbed word where j is the perturbed coordinate) -- held as two fp32 words, so that the subtraction costs no rounding where it is
 * not exact (a velocity that decays or changes sign):
 *   D_j.hi = fl(x'_j.hi - x_j.start),   D_j.lo = e_j + x'_j.lo,   e_j = (x'_j.hi - x_j.start) - D_j.hi exactly (two-sum)
 * Then, with H = D_r(+).hi - D_r(-).hi as two words (H.hi the fp32 difference, H.lo its exact rounding error) and
 * L = H.lo + (D_r(+).lo - D_r(-).lo),
 *   A[i][r][c] = (((r == c ? S.hi : 0.0f) + H.hi) + (L + (r == c ? S.lo : 0.0f))) * (1.0f / S.hi)
 *   B[i][r][a] =                           (H.hi  +  L)                           * (1.0f / S.hi)
 * S = c(+) - c(-) (u(+) - u(-)), the perturbed words as actually rounded: S.hi their fp32 difference, S.lo its exact rounding error.  The
 * identity enters as the step itself, before the quotient: 1 + dD / step with dD / step near -1 (a strongly damped velocity) would keep
 * roundings of the size of 1 in an entry near 0.  The reciprocal is the build's fp32 divide.  So an entry differs from the same quotient formed in fp64 from the high words that jaco_rollout returns by the low
 * words, at most half a spacing of x' per side, the reciprocal and the roundings of dD and of the product -- nothing else.  Differencing
 * the increments rather than the end states keeps the fp32 spacing of a joint angle (2.4e-7 .. 4.8e-7 at |q| in [2, 8)) from being
 * divided by 2 eps.  With option "compensated" = 0 the x'.lo are zero and the quotient is that of the end states' words.
 * centered = 0: forward differences, D_r(+) - D_r(0) over c(+) - c0, against the nominal.
 * Outputs (device; each pointer of JacoTransitionOut may be NULL, at least one is required), in the layout jaco_lqr reads:
 *   A [n][nx][nx], B [n][nx][na] fp32;
 *   next_qpos [n][nq], next_qvel [n][nv]: the nominal's fp32 state after the `hold` substeps;
 *   status [n] uint32: the nominal's JACO_FLAG_NAN / JACO_FLAG_SOLVER_MAXITER, as jaco_rollout reports them.  A perturbed evaluation that
 *                 goes non-finite shows as a non-finite entry of its column; no status bit is defined for it.
 * A ctrl word further than eps_ctrl beyond its limited ctrlrange gives a B column of exactly 0.0f (the actuators clamp both sides alike).
 * groups: the columns of a pair are dealt to `groups` wavefronts (column c to c % groups); 0 = the library chooses from n.  No result
 * depends on groups or on which outputs are asked for.
 * Nothing of the handle is written.  Asynchronous on `stream`: one kernel launch (none for n == 0, which returns JACO_OK), no
 * allocation, no synchronisation, no host copy; the options travel in the kernel arguments.
 * JACO_EINVAL, with no output touched, for NULL options; hold outside [1, JACO_TRANSITION_MAX_HOLD]; centered not 0 / 1; n < 0; a NULL
 * out or all five outputs NULL; only one of qpos_dev / qvel_dev; n != num_envs with the handle's state; an eps that is not finite and
 * positive; ndofs outside [1, JACO_ROLLOUT_FB_MAX_DOFS], a dof outside [0, nv), a dof of a free joint, a dof listed twice; nacts outside
 * [0, JACO_ROLLOUT_FB_MAX_DOFS], a ctrl word outside [0, nu) or listed twice; B with nacts = 0; groups outside [0, 2 ndofs + nacts]. */
#define JACO_TRANSITION_MAX_HOLD 1024
typedef struct JacoTransitionOptions {
  int32_t hold;                              /* substeps per evaluation, 1 .. JACO_TRANSITION_MAX_HOLD; 1 */
  int32_t centered;                          /* 1: central differences; 0: forward differences against the nominal; 1 */
  int32_t groups;                            /* wavefronts per pair, 1 .. 2 ndofs + nacts; 0: the library chooses; 0 */
  int32_t ndofs;                             /* 1 .. JACO_ROLLOUT_FB_MAX_DOFS */
  int32_t dofs[JACO_ROLLOUT_FB_MAX_DOFS];    /* distinct hinge dofs */
  int32_t nacts;                             /* 0 .. JACO_ROLLOUT_FB_MAX_DOFS */
  int32_t acts[JACO_ROLLOUT_FB_MAX_DOFS];    /* distinct ctrl words */
  float eps_qpos, eps_qvel, eps_ctrl;        /* rad, rad/s, ctrl units: > 0, finite; 2^-8, 2^-3 (JACO_FD_DEFAULTS'), 2^-6 */
  int32_t reserved;
} JacoTransitionOptions;
typedef struct JacoTransitionOut { float* A; float* B; float* next_qpos; float* next_qvel; uint32_t* status; } JacoTransitionOut;
int jaco_transition_fd(JacoHandle* h, const JacoTransitionOptions* opt_host, int n, const float* qpos_dev, const float* qvel_dev, const float* ctrl_dev,
                       const JacoTransitionOut* out, void* stream);

/* ---- the quadratic expansion of jaco_rollout_cost's cost along trajectories: the lx, lxx, lu, Vx, Vxx that jaco_lqr reads, for R
 * trajectories of T = nknots knots in ONE kernel launch (mujoco_jaco_amd/csrc/cost_quad.h).  R is NOT tied to num_envs and nothing of
 * the handle but its model is read.
 * Inputs (device, fp32), exactly what jaco_rollout_fb / jaco_rollout_cost write: qpos_dev [R][T][nq], qvel_dev [R][T][nv]: the state
 * AFTER knot k, x_(k+1);  ctrl_dev [R][T][nu]: the commanded row of knot k (NULL = zeros).  The start state x_0 is not an input:
 * jaco_rollout_cost does not cost it, so its expansion is zero.
 * Coordinates, with nd = ndofs, nx = 2 nd, na = nacts: x_j = qpos[qposadr(dofs[j])] for j < nd, qvel[dofs[j - nd]] for nd <= j < nx
 * (jaco_rollout_fb's convention);  u_a = ctrl[acts[a]].  wu[a] weighs u_a: it is indexed by the position in acts, where
 * JacoRolloutCostOptions.wu is indexed by the ctrl word.
 * Goals (JacoCostQuadGoal, device): xgoal [ngoals][G][nx], pgoal [ngoals][G][3], G = goal_per_knot ? T : 1; trajectory r takes goal
 * goal_idx[r] (goal_idx NULL: goal r).  Without a state and a pose weight no goal is read and the record may be NULL.
 * THE COST EXPANDED is jaco_rollout_cost's, term for term, re-indexed to jaco_lqr's convention: l_t(x_t, u_t) for t = 0 .. T - 1 plus a
 * terminal cost on x_T.  Work item (r, k):  x = x_(k+1), pos = the position of frame_host's ORIGIN at that state (the point
 * jaco_rollout's xpos reports and the cost uses; JacoFrame.point is ignored), g = goal_per_knot ? k : 0, (W, Wp) = (wx, wp) for
 * k < T - 1 and (wxT, wpT) for k = T - 1,
 *   d_j = x_j - xgoal[.][g][j]   (not wrapped),      e_c = pos_c - pgoal[.][g][c],
 *   Jp [3][nd]: column j the translational Jacobian of dof dofs[j] at pos, exactly 0 where the frame's body is not on that dof's chain
 *               -- jaco_query's jac rows 0 .. 2 for the same frame with point = 0, composed by the same expressions,
 *   gx_j = W_j d_j + [j < nd] Wp sum_c Jp[c][j] e_c,      H_ji = delta_ji W_j + [j, i < nd] Wp sum_c Jp[c][j] Jp[c][i].
 * GAUSS-NEWTON: the pose term's second-order part, e . d2pos/dq2, is dropped, as every iLQR does; H is positive semi-definite.
 * Outputs (device; each pointer of JacoCostQuadOut may be NULL, at least one is required), in the layout jaco_lqr reads:
 *   lx [R][T][nx], lxx [R][T][nx][nx]: row 0 exact zeros (written by item k = 0), row k + 1 = gx, H of item k for k < T - 1;
 *   Vx [R][nx], Vxx [R][nx][nx]: gx, H of item k = T - 1 (the final weights);
 *   lu [R][T][na]: lu_a = wu[a] * u_a of knot k.  luu is the constant diag(wu) and lux is zero: neither is written (hand luu to jaco_lqr
 *                  once, through shared_knots | shared_probs, and leave lux NULL);
 *   l [R][T]: knot k's own summand of jaco_rollout_cost's cost, 1/2 sum_a wu[a] u_a^2 + 1/2 sum_j W_j d_j^2 + 1/2 Wp |e|^2; its sum over k
 *             is that rollout's cost to rounding;
 *   status [R][T] uint32: JACO_FLAG_NAN where a word of the item's qpos / qvel / ctrl rows, a goal word it reads or a result is not
 *             finite; JACO_ROLLOUT_BAD_INDEX for a goal_idx entry outside [0, ngoals), and that item writes nothing else.
 * fp32 order that is part of the interface: where Wp == 0, gx_j = W_j * (x_j - xgoal_j), one subtraction and one multiplication (0.0f
 * where no state weight is set at all); always lu_a = wu[a] * u_a; lxx and Vxx are symmetric bit for bit (H_ji and H_ij are one fmaf
 * chain over c on commuted products); the cross blocks between positions and velocities and the off-diagonal velocity entries are
 * exactly 0.0f.  Two runs of the same call agree bit for bit, and no output depends on which others are asked for.
 * Asynchronous on `stream`: one kernel launch (none for R == 0, which returns JACO_OK), no allocation, no synchronisation, no host copy,
 * nothing of the handle written; the options, the frame and the goal record travel in the kernel arguments.
 * JACO_EINVAL, with no output touched, for NULL options or out, or all seven outputs NULL; R < 0; nknots < 1; goal_per_knot not 0 / 1;
 * R x nknots beyond 2^31 - 1; ndofs outside [1, JACO_ROLLOUT_FB_MAX_DOFS], a dof outside [0, nv), of a free joint or listed twice; nacts
 * outside [0, JACO_ROLLOUT_FB_MAX_DOFS], a ctrl word outside [0, nu) or listed twice; only one of qpos_dev / qvel_dev; a weight that is
 * negative or not finite (every word of wx, wxT and wu is checked; the state weights behind the first 2 ndofs are otherwise not used); a
 * non-zero state weight without xgoal; a non-zero pose weight without pgoal, without a frame or with a frame that is world-fixed or on
 * no body of the model; lu with nacts = 0; a non-zero state or pose weight with qpos_dev or qvel_dev NULL, with ngoals < 1, or with
 * R > ngoals and no goal_idx. */
typedef struct JacoCostQuadOptions {
  int32_t nknots;                            /* T >= 1 */
  int32_t goal_per_knot;                     /* 0: one goal per goal row; 1: one per goal row and knot */
  int32_t ndofs;                             /* 1 .. JACO_ROLLOUT_FB_MAX_DOFS */
  int32_t dofs[JACO_ROLLOUT_FB_MAX_DOFS];    /* distinct hinge dofs */
  int32_t nacts;                             /* 0 .. JACO_ROLLOUT_FB_MAX_DOFS */
  int32_t acts[JACO_ROLLOUT_FB_MAX_DOFS];    /* distinct ctrl words */
  float wx[2 * JACO_ROLLOUT_FB_MAX_DOFS];    /* state weights of the knots k < T - 1; finite, >= 0 */
  float wxT[2 * JACO_ROLLOUT_FB_MAX_DOFS];   /* state weights of the last knot */
  float wu[JACO_ROLLOUT_FB_MAX_DOFS];        /* ctrl weights, by position in acts */
  float wp, wpT;                             /* pose weights: running, last knot */
  int32_t reserved;
} JacoCostQuadOptions;
typedef struct JacoCostQuadGoal { const float* xgoal; const float* pgoal; const int32_t* goal_idx; int32_t ngoals; } JacoCostQuadGoal;   /* device pointers */
typedef struct JacoCostQuadOut { float* lx; float* lxx; float* lu; float* Vx; float* Vxx; float* l; uint32_t* status; } JacoCostQuadOut;
int jaco_cost_quad(JacoHandle* h, const JacoCostQuadOptions* opt_host, const JacoFrame* frame_host, int R, const float* qpos_dev, const float* qvel_dev,
                   const float* ctrl_dev, const JacoCostQuadGoal* goal_host, const JacoCostQuadOut* out, void* stream);

/* ---- contact readout: data.contact and mj_contactForce / efc_force (what the reference reads through sim.data.contact), batched.
 * jaco_set_contact_record turns the record on: from then on every jaco_physics_step (any nsub) and jaco_step writes, for every env, the
 * contacts of the LAST INTEGRATING SUBSTEP of that call -- those of the forward pass at the start of that substep, which is what
 * d.contact / d.efc_force hold after MuJoCo's mj_step -- with their forces in the contact frame:
 *   dist, pos[3], frame[9] (row 0 = the normal, from geom 1 towards geom 2, as MuJoCo);
 *   force[6] as mj_contactForce forms it for the pyramidal cone: force[0] = the sum of the contact's 2 (dim - 1) pyramid-edge forces (its one
 *     row for dim 1), force[k] = mu[k-1] (f[2k-2] - f[2k-1]) for k = 1 .. dim-1 (mu: the pair's friction), the rest 0.  It is the force
 *     geom 1's body exerts on geom 2's body, in the contact frame;
 *   geom[2]: the library's geom ids of the pair (mujoco_jaco_amd/robot_config.py ContactNames maps them to MJCF ids through the model's
 *     f_geom_orig), body[2]: the two geoms' MJCF (unfused) body ids, dim: the contact's condim.
 * ncon_dev[env] is the TRUE contact count, which may exceed `capacity`: records past it are dropped (ncon > capacity says so); the slots from
 * min(ncon, capacity) on keep what they held.  What writes NOTHING: forward passes and resets (jaco_forward, jaco_reset and its placing
 * hold / grasping pre-reach, jaco_take_action / jaco_terminal_inspection) and the forward pass of option "auto_reset" -- so with
 * auto_reset the record after a terminal step holds the TERMINAL step's contacts, like jaco_get_terminal_obs; an env frozen after its
 * episode ended (no auto_reset) keeps the record of its terminal step.  Contact-free steps (option "disable_contact", models without a
 * collidable pair) write ncon = 0.  Every capacity tier writes the record, whichever tier runs the env's last substep.
 * Buffers: rec_dev [num_envs][capacity] JacoContact (16-byte aligned), ncon_dev [num_envs] int32, device memory owned by the caller with the
 * lifetime rules of jaco_set_noise; NULL rec_dev turns the record off (then the step kernels store nothing extra and give bit-identical
 * results either way).  JACO_EINVAL for a capacity outside [1, JACO_CONTACT_MAX_CAPACITY] or a missing count buffer.  Cost: one 96-byte
 * record per contact per env per step call, written after the last substep's solver. */
#define JACO_CONTACT_MAX_CAPACITY 1024
typedef struct JacoContact {
  float dist, pos[3], frame[9], force[6];
  int32_t geom[2], body[2], dim;
} JacoContact;
#ifdef __cplusplus
static_assert(sizeof(JacoContact) == 96, "JacoContact: 24 32-bit words");
#endif
int jaco_set_contact_record(JacoHandle* h, JacoContact* rec_dev, int32_t* ncon_dev, int capacity);

/* Solver / collision options, MuJoCo <option> names: "iterations", "tolerance", "ls_iterations",
 * "disable_contact" (contact flag), "mpr_iterations", "mpr_tolerance", "mpr_output"; "compensated" (1 default, see jaco_set_state).
 * "auto_reset" (0 default): jaco_step resets an env whose step ended its episode inside the same call -- sim.reset(), the draws of _reset
 * (the code and RNG stream of jaco_reset), sim.forward() -- in the wavefront that finished it: reward_dev / done_dev carry the terminal
 * step's values, the env's obs_dev row and task row are the new episode's first.  Bit-identical to jaco_step followed by
 * jaco_reset(done mask); honoured for the tasks whose reset is draws + forward pass (picking, reaching, pickAndplace).
 * Setting a model option (everything in this first group except "disable_contact") SYNCHRONISES the device before the model
 * constants are re-uploaded: it is the one entry point besides the *_debug / *_time_ms hooks that does.
 * Execution options ("schedule", "concurrent_heavy", "heavy_workers", "handdown", "merge_prepare": bit-identical results; "hints" / "tier_return" pick which
 * capacity tier's code steps a substep, and the tiers group their row sums differently: results agree to fp32 rounding): "schedule" (1: launch expensive envs first), "concurrent_heavy" (1: medium / heavy / huge
 * tier workgroups resident next to the light grid), "heavy_workers" (maximum of the medium tier's; the resident number follows the
 * previous step's hand-overs), "tier_return" (1: a bigger tier gives an env back once its overflow is over), "hints" (where an env
 * starts its next step: 0 always the light tier, 1 the biggest tier its last step needed, 2 (default) the tier its last substep
 * needed), "handdown" (1, default: the first heavy drain passes calmed-down envs to a second medium drain instead of keeping them
 * for the rest of the step), "merge_prepare" (1, default: a step's routing kernel also prepares the tier queues of the NEXT launch --
 * the queue state is double-buffered -- so that steps in a row start with one small kernel; 0: every launch prepares its own queues
 * with a kernel of its own; bit-identical results). */
int jaco_set_option(JacoHandle* h, const char* name, double value);

/* Test hook: like jaco_physics_step but also copies the stage dump of environment `env` taken in
 * the last substep (layout: JDBG_* in csrc/physics_kernel.h) to host memory; synchronises. */
int jaco_physics_step_debug(JacoHandle* h, const float* ctrl_dev, int nsub, int env, float* dump_host, int dump_floats);
int jaco_debug_dump_floats(void);
/* Kernel launches issued for this handle since the previous call of this function (host-side counter, no device work):
 * bench.py's launches_per_step. */
long long jaco_launch_count(JacoHandle* h);
/* Diagnostic: control words of the tier queues after the last launch (per tier: envs queued, slots claimed by resident workers,
 * workers started / kept in reserve, envs queued before the launch from last step's hints); returns the number of words. */
int jaco_debug_queue_words(JacoHandle* h, int32_t* out_host, int n);

/* Average device time of the light-tier kernel (jaco_physics_kernel: the dominant kernel, what rocprofv3 --stats lists under that
 * name) over the step launches since jaco_enable_timing, measured with HIP events on the stream the kernel was launched on (bench.py
 * roofline leg); synchronises. */
int jaco_kernel_time_ms(JacoHandle* h, double* avg_ms, int* launches);
/* Same window, the whole launch set of a step (routing and ordering passes, light grid, the tiers' workers and drains): call it
 * BEFORE jaco_kernel_time_ms, which closes the window. */
int jaco_step_time_ms(JacoHandle* h, double* avg_ms);
int jaco_enable_timing(JacoHandle* h, int enable);

/* Diagnostic builds only (-DJACO_PROFILE_STAGES): per-env, per-stage shader-clock sums [num_envs][12] copied to host;
 * the shipped library returns JACO_EINVAL. */
int jaco_stage_profile(JacoHandle* h, uint64_t* out_host, int reset);

#ifdef __cplusplus
}
#endif
#endif /* JACO_ENV_H */
