// Env snapshots (jaco_save_envs / jaco_load_envs, include/jaco_env.h): the complete per-env state as one row of 32-bit words.
//
// JACO_SNAPSHOT_FIELDS is the snapshot part of the ONE table of the handle's per-env arrays (env_arrays.h).  The handle's members, their
// allocation and release are generated from that table; so are the field enum, the offsets, the row width W, the save and the load routine
// here (the GPU kernels in jaco_env.hip and the CPU tests' host build, tests/emu/emu_driver.cpp, run the same two functions).  Every array of
// the table is in the row or carries, in the table, the reason why not; a new one is one line there (+ JSNAP_LAYOUT_VERSION if it is state).
//
// Row layout: word 0 = fingerprint (layout version, nq, nv, nsensor, JTASK_N, JCACHE_N, task id hashed into one word), words 1-3 zero, then
// the fields in table order, dword-packed, padded with zeros to a multiple of 4 words (rows of a [n][W] buffer are 16-byte aligned).
// A field whose array the build at hand does not have (NULL in JacoSnapSrc: the CPU emulator keeps no compensation words, hints, costs or
// terminal observation) keeps its place in the row: saved as zeros, skipped by a load.  W therefore depends on the model alone.
//
// NOT in the row, and why:
//  * sepdir, the separating-direction cache of the hull narrowphase (12 KB per env).  Every entry is a guess that a support query
//    re-validates before it is used (collision.h, "Separating directions" in the narrowphase: a cached direction only counts while one
//    support query along it still shows the gap; otherwise the pair goes through MPR as without the cache -- "any stale or foreign value
//    is harmless"), which is why option "sep_cache" is bit-neutral.
//    Its content cannot change a result; a load leaves the destination's entries as they are.
//  * per-launch scratch: remaining, routed_mark, order (one row per env: JACO_SCRATCH_ARRAYS of the table, each with its reason), the tier
//    queues (qlist / qctl) and order_ctl.  They are rebuilt by every launch; qctl / order_ctl carry demand and cost figures of the previous
//    launch that size worker grids and bucket the launch order, nothing a result depends on.
//  * what the library only points to (noise, sub-goal and contact-record buffers of the caller), the recorded-goal buffer, and the
//    handle-wide settings (seed, frame_skip, options).
//  * the random STREAM: it is keyed by (seed, env index, counter) and only the counter (task row, JT_RNG) is state.  A row restored into
//    the env index it came from continues the same stream; loaded into another index it gives the same physical state on that index's
//    own stream, from the same counter.
#pragma once
#include <stddef.h>
#include <stdint.h>

#ifndef JTASK_N
#error "snapshot.h needs JTASK_N / JCACHE_N: include physics_kernel.h (env_logic.h) first"
#endif
#include "env_arrays.h"

#define JSNAP_LAYOUT_VERSION 1u
#define JSNAP_HEADER_WORDS 4
#define JSNAP_FLAG_BAD 0x40000u       // JACO_FLAG_BAD_SNAPSHOT of the public header (bit 18: bits 0-7 and 17 are the step kernels', 8-16 the bail causes)

#define JSNAP_X_ENUM(f, w) JSNAP_##f,
enum JacoSnapFieldId { JACO_SNAPSHOT_FIELDS(JSNAP_X_ENUM, 0, 0, 0) JSNAP_NFIELD };
#undef JSNAP_X_ENUM

#define JSNAP_X_NAME(f, w) #f,
static const char* const jaco_snap_field_names[JSNAP_NFIELD] = {JACO_SNAPSHOT_FIELDS(JSNAP_X_NAME, 0, 0, 0)};
#undef JSNAP_X_NAME

// the fields' arrays ([nenv][words], 32-bit elements): the handle's own (jaco_snap_src) or the CPU emulator's; NULL = this build keeps no such array
#define JSNAP_X_MEMBER(f, w) void* f = nullptr;
struct JacoSnapSrc { JACO_SNAPSHOT_FIELDS(JSNAP_X_MEMBER, 0, 0, 0) };
#undef JSNAP_X_MEMBER
#define JSNAP_X_SRC(f, w) s.f = a.f;
static inline JacoSnapSrc jaco_snap_src(const JacoEnvArrays& a) { JacoSnapSrc s; JACO_SNAPSHOT_FIELDS(JSNAP_X_SRC, 0, 0, 0) return s; }
#undef JSNAP_X_SRC

struct JacoSnapField { uint32_t* base; int words, off; };
struct JacoSnapTable {
  JacoSnapField f[JSNAP_NFIELD];
  int W, nenv;             // words per row (multiple of 4); envs of the handle
  uint32_t fingerprint;
};
struct alignas(16) JacoSnapVec { uint32_t x[4]; };   // the snapshot side moves 16 bytes per lane

static inline uint32_t jaco_snap_fingerprint(int nq, int nv, int nsensor, int task_id) {
  const uint32_t in[7] = {JSNAP_LAYOUT_VERSION, (uint32_t)nq, (uint32_t)nv, (uint32_t)nsensor, (uint32_t)JTASK_N, (uint32_t)JCACHE_N, (uint32_t)task_id};
  uint32_t hsh = 2166136261u;   // FNV-1a over the seven words, byte by byte
  for (int i = 0; i < 7; i++) for (int b = 0; b < 4; b++) { hsh ^= (in[i] >> (8 * b)) & 255u; hsh *= 16777619u; }
  return hsh ? hsh : 1u;        // (never 0: a zeroed buffer is not a snapshot)
}

static inline JacoSnapTable jaco_snapshot_table(const JacoSnapSrc& s, int nq, int nv, int nsensor, int task_id, int nenv) {
  JacoSnapTable T{};
  int off = JSNAP_HEADER_WORDS, i = 0;
#define JSNAP_X_ROW(fld, w) T.f[i].base = static_cast<uint32_t*>(s.fld); T.f[i].words = (w); T.f[i].off = off; off += (w); i++;
  JACO_SNAPSHOT_FIELDS(JSNAP_X_ROW, nq, nv, nsensor)
#undef JSNAP_X_ROW
  T.W = (off + 3) & ~3;
  T.nenv = nenv;
  T.fingerprint = jaco_snap_fingerprint(nq, nv, nsensor, task_id);
  return T;
}

// word w of env e's row <-> the library's arrays.  The loop runs over the table with a uniform index (the table sits in kernel arguments:
// scalar registers); at most one field matches a word.
static __host__ __device__ __forceinline__ uint32_t jaco_snap_fetch(const JacoSnapTable& T, int e, int w) {
  uint32_t v = w == 0 ? T.fingerprint : 0u;
  for (int i = 0; i < JSNAP_NFIELD; i++) {
    const int k = w - T.f[i].off;
    if (k >= 0 && k < T.f[i].words && T.f[i].base) v = T.f[i].base[(size_t)e * T.f[i].words + k];
  }
  return v;
}
static __host__ __device__ __forceinline__ void jaco_snap_store(const JacoSnapTable& T, int e, int w, uint32_t v) {
  for (int i = 0; i < JSNAP_NFIELD; i++) {
    const int k = w - T.f[i].off;
    if (k >= 0 && k < T.f[i].words && T.f[i].base) T.f[i].base[(size_t)e * T.f[i].words + k] = v;
  }
}

// row := env e.  Called by the `nlanes` lanes of one wavefront (host build: lane 0 of 1) with e and row uniform: lane l moves the 16-byte
// pieces l, l + nlanes, ... of the row -- consecutive lanes write consecutive 16 bytes of the row and read consecutive groups of 4 dwords
// of the library's arrays (their rows are 23 / 21 / ... words wide: no wider access is aligned there).
static __host__ __device__ __forceinline__ void jaco_snap_save_entry(const JacoSnapTable& T, int e, uint32_t* row, int lane, int nlanes) {
  JacoSnapVec* out = reinterpret_cast<JacoSnapVec*>(row);
  for (int q = lane; q < T.W / 4; q += nlanes) {
    JacoSnapVec v;
    for (int c = 0; c < 4; c++) v.x[c] = jaco_snap_fetch(T, e, 4 * q + c);
    out[q] = v;
  }
}
// env e := row.  A row of another build, model, task or layout version (fingerprint) leaves the env untouched and marks it.
static __host__ __device__ __forceinline__ void jaco_snap_load_entry(const JacoSnapTable& T, int e, const uint32_t* row, int lane, int nlanes) {
  if (row[0] != T.fingerprint) {
    if (lane == 0 && T.f[JSNAP_flags].base) T.f[JSNAP_flags].base[e] |= JSNAP_FLAG_BAD;
    return;
  }
  const JacoSnapVec* in = reinterpret_cast<const JacoSnapVec*>(row);
  for (int q = lane; q < T.W / 4; q += nlanes) {
    const JacoSnapVec v = in[q];
    for (int c = 0; c < 4; c++) jaco_snap_store(T, e, 4 * q + c, v.x[c]);
  }
}
// entry i of a save / load call: which env, which row; false = out of range, the entry is a no-op
static __host__ __device__ __forceinline__ bool jaco_snap_entry(const JacoSnapTable& T, const int32_t* env_idx, const int32_t* row_idx, int nrows, int i, int* e, int* r) {
  *e = env_idx ? env_idx[i] : i;
  *r = row_idx ? row_idx[i] : i;
  return *e >= 0 && *e < T.nenv && *r >= 0 && *r < nrows;
}
