// Batched inverse kinematics (jaco_ik, include/jaco_env.h): a damped least-squares solve per env -- which arm configuration puts this
// frame's point at this position (and the frame at this orientation)?
//
// One 64-lane wavefront per env on the contact-free LDS type (JacoLDS<JacoArm>), the query kernel's prologue (state floats as handed
// in, low words zero, model tables) and then, per iteration, the step kernel's own tree walk and nothing else: no mass matrix, nothing
// through HBM between iterations.  Iteration k:
//   1. pose of the controlled point, composed exactly as run_query composes it:  p = (xpos_b + R_b pos) + (R_b mat) point,  R = R_b mat;
//   2. e_p = p* - p;  e_r = rotation vector of R* R^T (axis sin from the antisymmetric part, cos from the trace, angle by atan2), 0 without
//      an orientation target;
//   3. converged when |e_p| < tol_pos and (no orientation or |e_r| < tol_rot): stop;    4. stop at k == max_iters, not converged;
//   5. J (6 x n_active): column d = [S_d.b + S_d.a x p ; S_d.a], rows 3-5 zero without an orientation target;
//   6. dq = J^T (J J^T + lambda^2 I_6)^-1 [e_p ; e_r];    7. max|dq| > max_step: dq scaled uniformly to max_step;
//   8. q += dq on the active dofs;    9. limited joints clamped to their range.
// Mapping: pose and error in every lane from same-address LDS reads (broadcasts); lane = dof holds its Jacobian column in registers and
// in the free row area s.J; lanes 0..35 form J J^T; lanes 0..5 eliminate (gj_solve6 of the OSC stage: lambda^2 I keeps the matrix
// definite, no pseudo-inverse branch); dq on the dof's lane; one wave max for the step clamp.  Control flow is wave-uniform (one env per
// wave): a wave leaves as soon as its env has converged.
// Nothing of a handle is read but the model; outputs: qpos_out (the seed row with the active dofs replaced, every other word copied bit
// for bit), resid (|e_p|, |e_r| of the last evaluation), status (iterations taken, converged 0 / 1).
// Listed at the tail of physics_kernel.h; the kernel is translation unit 10 (kernels.hip -DJACO_TU=10).
#pragma once

#define JIK_MAX_ITERS 256   // = JACO_IK_MAX_ITERS
struct JacoIkOpts {         // = JacoIkOptions of include/jaco_env.h (static_assert in abi_agreement.h)
  float tol_pos, tol_rot, damping, max_step;
  int max_iters, reserved;
  unsigned long long dof_mask;   // 0: every hinge dof on the frame's chain
};
struct JacoIkArgs {
  const JacoModelDev* model;
  const float* qpos;        // [nenv][nq] seed
  const float* target_pos;  // [nenv][3]
  const float* target_quat; // [nenv][4] unit quaternions, w first, or nullptr: position only
  float* qpos_out;          // [nenv][nq]
  float* resid;             // [nenv][2] or nullptr
  int* status;              // [nenv][2] or nullptr
  int nenv;
  unsigned active;          // the active dofs, resolved by the host half (jaco_ik_resolve)
  JacoQueryFrame fr;        // by value: no device buffer, no upload
  JacoIkOpts opt;
};

// The host half shared by jaco_ik (jaco_env.hip) and the emulator's entry: argument checks and the active dof set = hinge dofs on the
// chain of the frame's body, intersected with the caller's dof_mask when that is non-zero.  Returns nullptr, or what is wrong.
static inline const char* jaco_ik_resolve(const JacoModelDev& m, const JacoQueryFrame& fr, const JacoIkOpts& o, unsigned* active) {
  if (fr.body < -1 || fr.body >= m.nbody) return "frame body outside [-1, number of fused bodies)";
  if (o.max_iters < 0 || o.max_iters > JIK_MAX_ITERS) return "max_iters outside [0, 256]";
  if (!(o.tol_pos > 0.f) || !(o.tol_rot > 0.f) || !(o.damping > 0.f) || !(o.max_step > 0.f)) return "tol_pos, tol_rot, damping and max_step must be positive";
  unsigned hinge = 0u;
  for (int d = 0; d < m.nv; d++) if (m.d_qadr[d] >= 0) hinge |= 1u << d;
  unsigned a = fr.body >= 0 ? (m.b_chainmask[fr.body] & hinge) : 0u;
  if (o.dof_mask) a &= (unsigned)(o.dof_mask & 0xffffffffull);
  if (!a) return "empty active dof set (a world-fixed frame, a free body's frame, or a dof_mask that removes the whole chain)";
  *active = a;
  return nullptr;
}

template <class L>
JDEV void run_ik(const JacoIkArgs& Q_, L& s, int env, int lane) {
  // (the block is read through the kernarg segment pointer, an s_load per use, nothing carried across the loop)
  const JacoIkArgs& Q = *kernarg_view(Q_);
  const JacoModelDev* m = opaque_ptr(Q.model);
  const int nq = m->nq, nv = m->nv;
  // the prologue of run_query: the state is exactly the floats handed in (low-order words zero), at rest
  unsigned seed_bits = 0u;
  if (lane < nq) {
    seed_bits = reinterpret_cast<const unsigned*>(Q.qpos)[(size_t)env * nq + lane];
    s.qpos[lane] = __builtin_bit_cast(float, seed_bits); s.qpos_lo[lane] = 0.f;
  }
  if (lane < nv) { s.qvel[lane] = 0.f; s.qvel_lo[lane] = 0.f; }
  stage_model(m, s, lane);
  wave_sync();
  // per-lane constants: lane = dof
  const bool act = lane < nv && ((Q.active >> lane) & 1u) != 0u;
  const int bd = act ? s.mc.d_body[lane] : 0;
  const int qa = s.mc.b_qadr[bd];
  const bool limited = act && m->b_limited[bd] != 0;
  const float lo = m->b_range[bd][0], hi = m->b_range[bd][1];
  const bool has_rot = Q.target_quat != nullptr;
  const v3 pt = ld3(Q.target_pos + (size_t)env * 3);
  m3 Rt;
  for (int i = 0; i < 9; i++) Rt.m[i] = (i % 4) == 0 ? 1.f : 0.f;
  if (has_rot) {
    const float* tq = Q.target_quat + (size_t)env * 4;
    float w = tq[0], x = tq[1], y = tq[2], z = tq[3];
    const float n = sqrtf(w * w + x * x + y * y + z * z);
    if (n < JMINVAL) { w = 1.f; x = y = z = 0.f; } else { const float in = 1.f / n; w *= in; x *= in; y *= in; z *= in; }
    Rt = quat2mat(w, x, y, z);
  }
  const float tol_pos = Q.opt.tol_pos, tol_rot = Q.opt.tol_rot, lam2 = Q.opt.damping * Q.opt.damping, max_step = Q.opt.max_step;
  const int max_iters = Q.opt.max_iters;
  float* Jc = s.J;             // [JNV][6] Jacobian columns (the walk's S_d qvel_d area: rewritten by every walk, free after it)
  float* X = s.J + 6 * JNV;    // [6][6] J J^T + lambda^2 I
  float np_ = 0.f, nr_ = 0.f;
  int k = 0, conv = 0;
  for (;; k++) {
    stage_walk(m, s, lane, false);
    wave_sync();
    // frame pose, every lane (same-address LDS reads): as run_query composes it
    const int b = Q.fr.body;
    const m3 Rb = ldm(s.xmat[b]);
    const v3 pf = ld3(s.xpos[b]) + mul(Rb, ld3(Q.fr.pos));
    const m3 R = mul(Rb, ldm(Q.fr.mat));
    const v3 p = pf + mul(R, ld3(Q.fr.point));
    const v3 ep = pt - p;
    v3 er = mk3(0.f, 0.f, 0.f);
    if (has_rot) {   // rotation vector of E = R* R^T
      float E[9];
#pragma unroll
      for (int i = 0; i < 3; i++)
#pragma unroll
        for (int j = 0; j < 3; j++) E[3 * i + j] = Rt.m[3 * i] * R.m[3 * j] + Rt.m[3 * i + 1] * R.m[3 * j + 1] + Rt.m[3 * i + 2] * R.m[3 * j + 2];
      const v3 as = mk3(0.5f * (E[7] - E[5]), 0.5f * (E[2] - E[6]), 0.5f * (E[3] - E[1]));   // axis * sin
      const float cs = 0.5f * (E[0] + E[4] + E[8] - 1.f), sn = norm(as);
      const float ang = atan2f(sn, cs);
      // (sin = 0: no axis to read.  At angle 0 the vector is 0 anyway; at angle pi any axis serves to say "not there yet")
      er = sn < JMINVAL ? (cs < 0.f ? mk3(ang, 0.f, 0.f) : as) : as * (ang / sn);
    }
    np_ = norm(ep); nr_ = norm(er);
    conv = wave_uniform_i((np_ < tol_pos && (!has_rot || nr_ < tol_rot)) ? 1 : 0);
    if (conv || k >= max_iters) break;
    // lane = dof: column of the Jacobian at p (the query kernel's expression), zero for a dof outside the active set
    sv S; S.a = S.b = mk3(0.f, 0.f, 0.f);
    if (act) S = ldsv(s.cdof[lane]);
    v3 jp = S.b + cross(S.a, p), jr = S.a;
    if (!act) jp = mk3(0.f, 0.f, 0.f);
    if (!has_rot || !act) jr = mk3(0.f, 0.f, 0.f);
    if (lane < nv) { st3(Jc + 6 * lane, jp); st3(Jc + 6 * lane + 3, jr); }
    wave_sync();
    if (lane < 36) {   // lane = (i, j): entry of J J^T + lambda^2 I
      const int i = lane / 6, j = lane - 6 * i;
      float a = i == j ? lam2 : 0.f;
      for (int d = 0; d < nv; d++) a = fmaf(Jc[6 * d + i], Jc[6 * d + j], a);
      X[lane] = a;
    }
    wave_sync();
    float A[6], y = 0.f;
#pragma unroll
    for (int j = 0; j < 6; j++) A[j] = lane < 6 ? X[6 * lane + j] : 0.f;
    y = lane == 0 ? ep.x : (lane == 1 ? ep.y : (lane == 2 ? ep.z : (lane == 3 ? er.x : (lane == 4 ? er.y : (lane == 5 ? er.z : 0.f)))));
    gj_solve6(A, y, lane);
    const float y0 = wave_bcast(y, 0), y1 = wave_bcast(y, 1), y2 = wave_bcast(y, 2), y3 = wave_bcast(y, 3), y4 = wave_bcast(y, 4), y5 = wave_bcast(y, 5);
    float dq = act ? jp.x * y0 + jp.y * y1 + jp.z * y2 + jr.x * y3 + jr.y * y4 + jr.z * y5 : 0.f;
    const float mx = wave_max(fabsf(dq));
    if (mx > max_step) dq *= max_step / mx;
    if (act) {
      float q = s.qpos[qa] + dq;
      if (limited) q = fmaxf(lo, fminf(hi, q));
      s.qpos[qa] = q;
    }
    wave_sync();
  }
  if (lane < nq) {   // the seed row with the active dofs replaced: every other word goes out as it came in
    const int d = s.mc.q_dof[lane];
    const bool mine = d >= 0 && ((Q.active >> (d >= 0 ? d : 0)) & 1u) != 0u;
    reinterpret_cast<unsigned*>(Q.qpos_out)[(size_t)env * nq + lane] = mine ? __builtin_bit_cast(unsigned, s.qpos[lane]) : seed_bits;
  }
  if (lane == 0) {
    if (Q.resid) { Q.resid[(size_t)env * 2] = np_; Q.resid[(size_t)env * 2 + 1] = nr_; }
    if (Q.status) { Q.status[(size_t)env * 2] = k; Q.status[(size_t)env * 2 + 1] = conv; }
  }
}

#if JACO_TU_HAS(10)
JACO_DEFINE_ENTRY(ik, JacoIkArgs, Q.nenv, run_ik)
#else
JACO_DECLARE_ENTRY(ik, JacoIkArgs)
#endif
