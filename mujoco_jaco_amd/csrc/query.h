// Robot-configuration queries (jaco_query, include/jaco_env.h): body poses, Jacobians, mass matrix and bias forces of every env at a
// given state, what the reference reads through MujocoConfig (mujoco_config.py:201-447) and Mujoco.get_xyz / get_orientation
// (mujoco.py:148-215) -- the values of a sim.forward() on that state.
//
// One 64-lane wavefront per env, the step kernel's own stages on the contact-free LDS type (JacoLDS<JacoArm>: its tree walk skips the
// geom poses, nothing after the mass matrix runs): state load, model tables, tree walk, subtree sums, mass matrix + bias, then the
// outputs.  Nothing is written back to the env's state, task row, cache, flags or sensordata.
// Listed at the tail of physics_kernel.h; the kernel is translation unit 9 (kernels.hip -DJACO_TU=9).
#pragma once
#include <string>

#define JQ_MAXFRAMES 16   // = JACO_QUERY_MAX_FRAMES
struct JacoQueryArgs {
  const JacoModelDev* model;
  const float* qpos;      // [nenv][nq]  (the handle's hi words, or the caller's override)
  const float* qvel;      // [nenv][nv]
  float* xpos;            // [nenv][nframes][3] or nullptr
  float* xmat;            // [nenv][nframes][9] or nullptr
  float* jac;             // [nenv][nframes][6][nv] or nullptr
  float* qM;              // [nenv][nv][nv] or nullptr
  float* bias;            // [nenv][nv] or nullptr
  int nenv, nframes;
  JacoQueryFrame fr[JQ_MAXFRAMES];   // by value: no device buffer, no upload
};

// The host half shared by jaco_query (jaco_env.hip) and the emulator's entry: argument checks, then the frame table and its length into
// the argument block.  Returns an empty string, or what is wrong.
static inline std::string jaco_query_resolve(const JacoModelDev& m, const JacoQueryFrame* frames, int nframes, JacoQueryArgs* Q) {
  if (nframes < 0 || nframes > JQ_MAXFRAMES || (nframes > 0 && !frames))
    return "nframes " + std::to_string(nframes) + " outside [0, " + std::to_string(JQ_MAXFRAMES) + "]";
  for (int f = 0; f < nframes; f++) {
    if (frames[f].body < -1 || frames[f].body >= m.nbody)
      return "frame " + std::to_string(f) + ": body " + std::to_string(frames[f].body) + " outside [-1, " + std::to_string(m.nbody) + ")";
    Q->fr[f] = frames[f];
  }
  Q->nframes = nframes;
  return std::string();
}

template <class L>
JDEV void run_query(const JacoQueryArgs& Q_, L& s, int env, int lane) {
  // The frame table is indexed per lane: read through the kernarg segment pointer (global loads) rather than the by-value parameter,
  // which a dynamic index would copy to scratch.
  const JacoQueryArgs& Q = *kernarg_view(Q_);
  const JacoModelDev* m = opaque_ptr(Q.model);
  const int nq = m->nq, nv = m->nv, nf = Q.nframes;
  // the prologue of run_env, state and model tables only: the state is exactly the floats handed in (low-order words zero)
  if (lane < nq) { s.qpos[lane] = Q.qpos[(size_t)env * nq + lane]; s.qpos_lo[lane] = 0.f; }
  if (lane < nv) { s.qvel[lane] = Q.qvel[(size_t)env * nv + lane]; s.qvel_lo[lane] = 0.f; }
  stage_model(m, s, lane);
  wave_sync();
  stage_walk(m, s, lane, false);
  for (int i = lane; i < JMBLK; i += 64) s.M[i] = 0.f;
  wave_sync();
  const bool want_m = Q.qM != nullptr || Q.bias != nullptr;
  if (want_m) {
    const StagePrefetch pf = stage_prefetch(m, lane);
    stage_accumulate(m, s, lane);
    wave_sync();
    stage_mass_bias(m, s, lane, pf);
    wave_sync();
  }
  // frame poses, lane = frame: composed as ee_frame composes the EE (xpos_b + R_b p, R_b R_f), so that the EE frame reproduces obs[1:4]
  float* P = s.J;   // [JQ_MAXFRAMES][3] world Jacobian points (the row area is free: stage_mass_bias is done with its scratch)
  if (lane < nf) {
    const JacoQueryFrame& F = Q.fr[lane];
    const int b = F.body;
    v3 p = ld3(F.pos);
    m3 R = ldm(F.mat);
    if (b >= 0) {
      const m3 Rb = ldm(s.xmat[b]);
      p = ld3(s.xpos[b]) + mul(Rb, ld3(F.pos));
      R = mul(Rb, ldm(F.mat));
    }
    if (Q.xpos) st3(Q.xpos + ((size_t)env * nf + lane) * 3, p);
    if (Q.xmat) stm(Q.xmat + ((size_t)env * nf + lane) * 9, R);
    st3(P + 3 * lane, p + mul(R, ld3(F.point)));
  }
  wave_sync();
  if (Q.jac && lane < nv) {   // lane = dof: column d of every frame's Jacobian, zero where dof d does not move the frame's body
    const sv S = ldsv(s.cdof[lane]);
    for (int f = 0; f < nf; f++) {
      const int b = Q.fr[f].body;
      const bool on = b >= 0 && ((m->b_chainmask[b >= 0 ? b : 0] >> lane) & 1u) != 0u;
      const v3 jp = S.b + cross(S.a, ld3(P + 3 * f));
      float* J = Q.jac + ((size_t)env * nf + f) * 6 * nv + lane;
      J[0 * nv] = on ? jp.x : 0.f; J[1 * nv] = on ? jp.y : 0.f; J[2 * nv] = on ? jp.z : 0.f;
      J[3 * nv] = on ? S.a.x : 0.f; J[4 * nv] = on ? S.a.y : 0.f; J[5 * nv] = on ? S.a.z : 0.f;
    }
  }
  if (Q.qM) {   // dense and symmetric (mj_fullM): the block-diagonal storage expanded, zero across trees
    for (int i = lane; i < nv * nv; i += 64) {
      const int d = i / nv, j = i - d * nv;
      const bool same = (d < JB0) == (j < JB0) && (d < JB1) == (j < JB1);
      Q.qM[(size_t)env * nv * nv + i] = same ? s.M[m_index(d, j)] : 0.f;
    }
  }
  if (Q.bias && lane < nv) Q.bias[(size_t)env * nv + lane] = s.bias[lane];
}

#if JACO_TU_HAS(9)
JACO_DEFINE_ENTRY(query, JacoQueryArgs, Q.nenv, run_query)
#else
JACO_DECLARE_ENTRY(query, JacoQueryArgs)
#endif
