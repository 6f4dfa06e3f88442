// The per-env arrays of a handle: ONE table.  Every array the library allocates with one row per env is a line below -- name, 32-bit element
// type, words per env -- and the handle's members (JacoEnvArrays), the widths (JacoEnvWords), their allocation and release (jaco_create /
// jaco_destroy) and the snapshot row (snapshot.h) are generated from it.  Host side only.  Needs JTASK_N / JCACHE_N and JACO_TASK_* in front of it.
#pragma once

#define JSNAP_OBS_WORDS 26   // width of an observation row

// What a snapshot row carries (snapshot.h), in row order: a change here bumps JSNAP_LAYOUT_VERSION.  nq / nv / nsensor: the MODEL's widths.
// A row is M(X, name, type, words): JENV_TYPED hands X(name, type, words) on, JENV_PLAIN the X(name, words) of JACO_SNAPSHOT_FIELDS.
#define JACO_SNAPSHOT_ARRAYS(M, X, nq, nv, nsensor)                                                                                   \
  M(X, qpos, float, nq) M(X, qpos_lo, float, nq)   /* compensated state, both halves (physics_kernel.h, comp_add): lo = 0 after a write from outside */ \
  M(X, qvel, float, nv) M(X, qvel_lo, float, nv)                                                                                          \
  M(X, qacc_ws, float, nv)                      /* solver warm start */                                                                \
  M(X, sensordata, float, nsensor)              /* touch values of the last substep (observation, termination rule) */                 \
  M(X, flags, unsigned, 1) M(X, stats, int, 4)     /* sticky bits and last-substep statistics travel with the env */                      \
  M(X, hint, int, 1)                            /* tier the env starts its next step in (tiers agree to fp32 rounding only) */         \
  M(X, cost, unsigned, 1)                       /* shader-clock ticks (>> 4) of the last step: launch order only (bit-neutral), keeps the schedule of a resumed run */ \
  M(X, task, float, JTASK_N)                    /* task row: JT_RNG draw counter, JT_DONE, step / episode counters, goals, target, gripper ramp */ \
  M(X, cache, float, JCACHE_N)                  /* what the controller reads one substep late (JC_*), placing pin */                   \
  M(X, marker, float, 24)                       /* [2][12] mocap poses of "hand" / "subgoal_reach" */                                  \
  M(X, terminal, float, 2)                      /* (success flag, wb) latched by every terminal step */                                \
  M(X, terminal_obs, float, JSNAP_OBS_WORDS)    /* observation of the terminal step (auto_reset) */
// One row per env, but NOT snapshot state, and why: per-launch scratch, rebuilt by every launch before it is read.
#define JACO_SCRATCH_ARRAYS(M, X)                                                                                                   \
  M(X, remaining, int, 1)     /* substeps left for the bigger tiers: written by the light tier / the routing kernel of the same launch */ \
  M(X, routed_mark, int, 1)   /* id of the launch that queued the env for a bigger tier before it started: compared with this launch's id only */ \
  M(X, order, int, 1)         /* launch order of the light grid (scatter pass), list of the masked envs (reset kernel): written by the launch that reads it */
#define JENV_TYPED(X, f, T, w) X(f, T, w)
#define JENV_PLAIN(X, f, T, w) X(f, w)
#define JACO_ENV_ARRAYS(X, nq, nv, nsensor) JACO_SNAPSHOT_ARRAYS(JENV_TYPED, X, nq, nv, nsensor) JACO_SCRATCH_ARRAYS(JENV_TYPED, X)
#define JACO_SNAPSHOT_FIELDS(X, nq, nv, nsensor) JACO_SNAPSHOT_ARRAYS(JENV_PLAIN, X, nq, nv, nsensor)

// the arrays themselves, [nenv][words]; nullptr = not allocated (a handle half built)
#define JENV_X_MEMBER(f, T, w) T* f = nullptr; static_assert(sizeof(T) == 4, "per-env arrays are made of 32-bit words");
struct JacoEnvArrays { JACO_ENV_ARRAYS(JENV_X_MEMBER, 0, 0, 0) };
#undef JENV_X_MEMBER

// words per env of every array, for a model of these widths
#define JENV_X_WORDS(f, T, w) int f;
struct JacoEnvWords { JACO_ENV_ARRAYS(JENV_X_WORDS, 0, 0, 0) };
#undef JENV_X_WORDS
#define JENV_X_SET(f, T, w) (w),
static inline JacoEnvWords jaco_env_words(int nq, int nv, int nsensor) { return JacoEnvWords{JACO_ENV_ARRAYS(JENV_X_SET, nq, nv, nsensor)}; }
#undef JENV_X_SET

// Two rules about task ids the host applies when it fills JacoStepArgs (the library and the CPU tests' driver).  Host only: device code
// tests in place (physics_kernel.h, the note at enum JacoMode).
static inline int jaco_task_nact(int task_id) { return (task_id == JACO_TASK_REACHING || task_id == JACO_TASK_PUSHING) ? 6 : 7; }   // width of an action row (env_mujoco.py:79-82)
// the tasks whose reset is nothing more than draws + sim.forward() + observation, which option "auto_reset" folds into the step wave
// (placing holds the object for 150 substeps, grasping pre-reaches: those keep the explicit jaco_reset)
static inline bool jaco_task_auto_resets(int task_id) { return task_id == JACO_TASK_PICKING || task_id == JACO_TASK_REACHING || task_id == JACO_TASK_PICKANDPLACE || task_id == JACO_TASK_PUSHING; }
