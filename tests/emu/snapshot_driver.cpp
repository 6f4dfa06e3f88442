// TEST INFRASTRUCTURE: host build of the env-snapshot table and its save / load routines (mujoco_jaco_amd/csrc/snapshot.h) -- the very
// header the GPU kernels jaco_save_envs_kernel / jaco_load_envs_kernel are compiled from; here one "lane" walks a whole row.
// Built by tests/snapshot_binding.py into tests/emu/libjaco_snap<layout>.so with the layout flags of tests/emu/Makefile.
#include <hip/hip_runtime.h>

#include "../../include/jaco_env.h"
#include "../../mujoco_jaco_amd/csrc/physics_kernel.h"   // (JTASK_N, JCACHE_N and the layout's model widths; -DJACO_TU=-1: no kernel is defined)
#include "../../mujoco_jaco_amd/csrc/snapshot.h"

static_assert(JSNAP_FLAG_BAD == JACO_FLAG_BAD_SNAPSHOT, "flag bit of snapshot.h and the public header must agree");

extern "C" int snap_nfield() { return JSNAP_NFIELD; }
extern "C" const char* snap_field_name(int i) { return i >= 0 && i < JSNAP_NFIELD ? jaco_snap_field_names[i] : nullptr; }
extern "C" int snap_header_words() { return JSNAP_HEADER_WORDS; }
extern "C" int snap_task_floats() { return JTASK_N; }
extern "C" int snap_cache_floats() { return JCACHE_N; }
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
