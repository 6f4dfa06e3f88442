// Batched operational-space controller (jaco_osc, include/jaco_env.h): abr_control's OSC(robot_config, kp, ko, kv, vmax).generate()
// (env_mujoco_util.py:59-63, 85-90) for any frame, any target and any gains -- the torques that drive this frame towards this pose.
//
// One 64-lane wavefront per env on the contact-free LDS type (JacoLDS<JacoArm>): the query kernel's prologue (state floats as handed in,
// low words zero, model tables), the step kernel's tree walk, subtree sums and mass matrix + bias -- the values of a sim.forward() on the
// given state, computed once -- and then, per frame (a wave-uniform loop of at most two), stage_osc_frame: stage_osc_general of
// env_logic.h with the active dofs, the frame pose, the target and the gains as arguments.
//   J  (6 x n): column k = [S_d.b + S_d.a x p ; S_d.a] of the k-th active dof d, at the frame's point p (run_query's composition);
//   M  (n x n): the submatrix of qM on the active dofs (the reference's M[arm, arm]; not a Schur complement);
//   n < 6: M padded with identity and J with zero columns, the 6 x 6 rule applied to the rank-deficient matrix as it stands -- its exact
//          determinant is 0, so such a frame always takes the pseudo-inverse branch (what rounding leaves of the pivots does not decide);
//   Mx = (J M^-1 J^T)^-1 when |det| >= 1e-3, else the pseudo-inverse that drops singular values < 0.005 (pinv6_jacobi);
//   u_task = [p - p* ; -vec(q* conj(q_R)) sign(w)], saturated at vmax / kp * kv and vmax / ko * kv, times the gains;
//   u = -kv M dq - J^T Mx u_task + bias.
// Mapping: lanes 0..5 own rows and columns (lane k = k-th active dof, read off the 32-bit active mask by bit scan: wave-uniform), lanes
// 0..35 own the entries of J M^-1 J^T; scratch is the free row area s.J (stage_mass_bias is done with it).  The branch on the
// determinant goes through a wave-uniform value: a scalar branch.
// Nothing of a handle is read but the model; outputs: ctrl_out (the ctrl_in row with u_d at the motor actuator of every active dof d,
// every other word moved as an integer) and status (1: pseudo-inverse branch).
// Listed at the tail of physics_kernel.h; the kernel is translation unit 11 (kernels.hip -DJACO_TU=11).
#pragma once
#include <string>

#define JOSC_MAXFRAMES 2   // = JACO_OSC_MAX_FRAMES
struct JacoOscOpts {       // = JacoOscOptions of include/jaco_env.h (static_assert in abi_agreement.h)
  float kp, ko, kv, vmax_xyz, vmax_abg;
  int reserved;
  unsigned long long dof_mask;   // 0: every hinge dof on the frame's chain
};
struct JacoOscArgs {
  const JacoModelDev* model;
  const float* qpos;         // [nenv][nq]
  const float* qvel;         // [nenv][nv]
  const float* target_pos;   // [nenv][nframes][3]
  const float* target_quat;  // [nenv][nframes][4] unit quaternions, w first
  const float* ctrl_in;      // [nenv][nu] or nullptr: zeros
  float* ctrl_out;           // [nenv][nu]; may be ctrl_in
  int* status;               // [nenv][nframes] or nullptr
  int nenv, nframes;
  unsigned active[JOSC_MAXFRAMES];   // the active dofs of each frame, resolved by the host half (jaco_osc_resolve)
  float sat_xyz, sat_abg;            // vmax_xyz / kp * kv, vmax_abg / ko * kv (formed once, on the host)
  JacoQueryFrame fr[JOSC_MAXFRAMES]; // by value: no device buffer, no upload
  JacoOscOpts opt;
};

// The controller's part of a host half, shared by jaco_osc_resolve below and jaco_rollout_osc_resolve (rollout_osc.h), with the entry's
// own rule for which arrays must be there (have_arrays, and the message when they are not): the checks of frames, gains, active sets and
// saturation levels; then the frame table, the options, the saturation levels and each frame's active dof set (hinge dofs on the chain of
// its body, intersected with dof_mask when that is non-zero) into the block.  Returns an empty string, or what is wrong.
static inline std::string jaco_osc_resolve_law(const JacoModelDev& m, const JacoQueryFrame* frames, int nframes, const JacoOscOpts& o, bool have_arrays,
                                               const char* no_arrays, JacoOscArgs* Q) {
  if (nframes < 1 || nframes > JOSC_MAXFRAMES || !frames)
    return "nframes " + std::to_string(nframes) + " outside [1, " + std::to_string(JOSC_MAXFRAMES) + "]";
  if (!have_arrays) return no_arrays;
  if (!(o.kp > 0.f) || !(o.ko > 0.f) || !(o.kv > 0.f) || !(o.vmax_xyz > 0.f) || !(o.vmax_abg > 0.f)) return "kp, ko, kv, vmax_xyz and vmax_abg must be positive";
  unsigned hinge = 0u, motor = 0u, seen = 0u;
  for (int d = 0; d < m.nv; d++) if (m.d_qadr[d] >= 0) hinge |= 1u << d;
  for (int a = 0; a < m.nu; a++) if (m.a_position[a] == 0 && m.a_dof[a] >= 0 && m.a_dof[a] < m.nv) motor |= 1u << m.a_dof[a];
  for (int f = 0; f < nframes; f++) {
    const std::string who = "frame " + std::to_string(f) + ": ";
    if (frames[f].body < 0 || frames[f].body >= m.nbody) return who + "body " + std::to_string(frames[f].body) + " outside [0, " + std::to_string(m.nbody) + ")";
    unsigned a = m.b_chainmask[frames[f].body] & hinge;
    if (o.dof_mask) a &= (unsigned)(o.dof_mask & 0xffffffffull);
    if (!a) return who + "empty active dof set (a free body's frame, or a dof_mask that removes the whole chain)";
    if (__builtin_popcount(a) > 6) return who + std::to_string(__builtin_popcount(a)) + " active dofs, at most 6 (narrow the chain with dof_mask)";
    if (a & seen) return who + "its active dofs overlap those of an earlier frame";
    if (a & ~motor) return who + "active dof " + std::to_string(__builtin_ctz(a & ~motor)) + " has no motor actuator";
    seen |= a;
    Q->active[f] = a;
    Q->fr[f] = frames[f];
  }
  Q->nframes = nframes;
  Q->opt = o;
  Q->sat_xyz = o.vmax_xyz / o.kp * o.kv;
  Q->sat_abg = o.vmax_abg / o.ko * o.kv;
  return std::string();
}

// The host half shared by jaco_osc (jaco_env.hip) and the emulator's entry: every argument check, then what jaco_osc_resolve_law puts
// into the argument block, whose pointers the caller has filled in.  Returns an empty string, or what is wrong.
static inline std::string jaco_osc_resolve(const JacoModelDev& m, const JacoQueryFrame* frames, int nframes, const JacoOscOpts& o, JacoOscArgs* Q) {
  return jaco_osc_resolve_law(m, frames, nframes, o, Q->target_pos && Q->target_quat && Q->ctrl_out,
                              "the target positions, the target quaternions and the output ctrl are required", Q);
}

struct OscGains { float kp, ko, kv, sat_xyz, sat_abg; };

// The pieces of run_osc_task (osc_task.h) and run_joint (joint.h).  run_osc below does NOT call them: it holds each of them written out
// (the ctrl word, the gains, the unit quaternion, the ctrl row), hand-kept twins, because its kernel on the shared functions measured
// 1 - 2 % slower on the MI355X and its part of that change was taken back whole.  A change here has to be made in run_osc too.
// this lane's ctrl_in word, read before anything is written (ctrl_out may be ctrl_in): moved as an integer
JDEV unsigned osc_read_ctrl(const float* ctrl_in, int env, int lane, int nu) {
  return (lane < nu && ctrl_in) ? reinterpret_cast<const unsigned*>(ctrl_in)[(size_t)env * nu + lane] : 0u;
}
// the gains out of the argument block
JDEV OscGains osc_gains(const JacoOscArgs& Q) {
  OscGains g;
  g.kp = Q.opt.kp; g.ko = Q.opt.ko; g.kv = Q.opt.kv; g.sat_xyz = Q.sat_xyz; g.sat_abg = Q.sat_abg;
  return g;
}
// the target quaternion, normalised again (a zero one: the identity)
JDEV void osc_unit_quat(const float* tq, float (&qd)[4]) {
  qd[0] = tq[0]; qd[1] = tq[1]; qd[2] = tq[2]; qd[3] = tq[3];
  const float qn = sqrtf(qd[0] * qd[0] + qd[1] * qd[1] + qd[2] * qd[2] + qd[3] * qd[3]);
  if (qn < JMINVAL) { qd[0] = 1.f; qd[1] = qd[2] = qd[3] = 0.f; } else { const float in = 1.f / qn; for (int k = 0; k < 4; k++) qd[k] *= in; }
}
// the ctrl_in row (`word`: this lane's, from osc_read_ctrl) with the motor of every active dof replaced: every other word goes out as
// it came in
JDEV void osc_write_ctrl(const JacoModelDev* m, float* ctrl_out, int env, int lane, unsigned all, unsigned word, const float* Uo) {
  const int nv = m->nv, nu = m->nu;
  if (lane < nu) {
    const int d = m->a_dof[lane];
    const bool mine = m->a_position[lane] == 0 && d >= 0 && d < nv && ((all >> (d >= 0 ? d : 0)) & 1u) != 0u;
    reinterpret_cast<unsigned*>(ctrl_out)[(size_t)env * nu + lane] = mine ? __builtin_bit_cast(unsigned, Uo[mine ? d : 0]) : word;
  }
}

// stage_osc_general (env_logic.h) with its four fixed things made arguments: the active dofs (a 32-bit mask, 1 <= popcount <= 6), the
// frame pose (pe, Re), the target (pt, unit qd) and the gains.  Needs s.cdof, s.M, s.bias, s.qvel; writes u_d to Uo[d] for every
// active dof d; returns 1 when the pseudo-inverse branch ran.  Scratch: s.J[0, 222).
template <class L>
JDEV int stage_osc_frame(L& s, int lane, unsigned active, const v3 pe, const m3& Re, const v3 pt, const float (&qd)[4], const OscGains& g, float* Uo) {
  float* Jm = s.J;            // [6][6] J[r][c], rows: 3 translational, 3 rotational; columns: active dofs
  float* T = s.J + 72;        // M^-1 J^T
  float* X = s.J + 108;       // J M^-1 J^T, then its (pseudo-)inverse Mx
  float* w = s.J + 144;       // Mx u_task
  // the active-dof list: bit scan of the wave-uniform mask (scalar registers, no per-lane array)
  int da[6], n = 0;
  {
    unsigned mk = (unsigned)wave_uniform_i((int)active);
#pragma unroll
    for (int k = 0; k < 6; k++) { da[k] = mk ? __builtin_ctz(mk) : -1; n += mk ? 1 : 0; mk &= mk - 1u; }
  }
  const int r = lane / 6, c = lane - 6 * r;   // lanes 0..35 = matrix entry (r, c)
  const int i = lane < 6 ? lane : 0;
  int di = da[0];
#pragma unroll
  for (int j = 1; j < 6; j++) di = i == j ? da[j] : di;
  const bool real = di >= 0;   // (a padding row / column otherwise)
  const int ds = real ? di : 0;
  // T = M^-1 J^T by elimination on [M | J^T] (lanes 0..5 own rows; row i of J^T is this lane's own Jacobian column)
  float A[6], B[6];
  {
    sv S = ldsv(s.cdof[ds]);
    v3 jp = S.b + cross(S.a, pe);
    B[0] = real ? jp.x : 0.f; B[1] = real ? jp.y : 0.f; B[2] = real ? jp.z : 0.f;
    B[3] = real ? S.a.x : 0.f; B[4] = real ? S.a.y : 0.f; B[5] = real ? S.a.z : 0.f;
  }
  if (lane < 6) {
#pragma unroll
    for (int k = 0; k < 6; k++) Jm[k * 6 + lane] = B[k];
  }
#pragma unroll
  for (int j = 0; j < 6; j++) A[j] = (real && da[j] >= 0) ? s.M[m_index(ds, da[j] >= 0 ? da[j] : 0)] : (i == j ? 1.f : 0.f);
  gj_inverse6(A, B, lane);
  if (lane < 6) for (int j = 0; j < 6; j++) T[lane * 6 + j] = B[j];
  wave_sync();
  if (lane < 36) { float a = 0.f; for (int k = 0; k < 6; k++) a += Jm[r * 6 + k] * T[k * 6 + c]; X[lane] = a; }
  wave_sync();
  // task-space error (uniform across lanes)
  float ut[6];
  ut[0] = pe.x - pt.x; ut[1] = pe.y - pt.y; ut[2] = pe.z - pt.z;
  float qe[4];
  mat_to_quat(Re, qe);
  // q_e = q_d * conj(q_frame)
  float cw = qe[0], cx = -qe[1], cy = -qe[2], cz = -qe[3];
  float ew = qd[0] * cw - qd[1] * cx - qd[2] * cy - qd[3] * cz;
  float ex = qd[0] * cx + qd[1] * cw + qd[2] * cz - qd[3] * cy;
  float ey = qd[0] * cy - qd[1] * cz + qd[2] * cw + qd[3] * cx;
  float ez = qd[0] * cz + qd[1] * cy - qd[2] * cx + qd[3] * cw;
  float sg = ew > 0.f ? 1.f : (ew < 0.f ? -1.f : 0.f);
  ut[3] = -ex * sg; ut[4] = -ey * sg; ut[5] = -ez * sg;
  // velocity limiting then gains: u_task <- kv * scale * lambda * u_task
  float nx = sqrtf(ut[0] * ut[0] + ut[1] * ut[1] + ut[2] * ut[2]), na = sqrtf(ut[3] * ut[3] + ut[4] * ut[4] + ut[5] * ut[5]);
  float sx = nx > g.sat_xyz ? g.sat_xyz / nx : 1.f, sa = na > g.sat_abg ? g.sat_abg / na : 1.f;
  for (int k = 0; k < 3; k++) { ut[k] *= g.kp * sx; ut[3 + k] *= g.ko * sa; }
  // w = Mx u_task:  Mx = X^-1 as a solve when |det X| >= 1e-3 (abr_control's plain inverse), else the SVD pseudo-inverse
  // that drops singular values < 0.005
#pragma unroll
  for (int j = 0; j < 6; j++) A[j] = X[i * 6 + j];
  float wi = ut[0];
#pragma unroll
  for (int j = 1; j < 6; j++) wi = i == j ? ut[j] : wi;
  float det = gj_solve6(A, wi, lane);
  // (a scalar branch; "not >=" so that a determinant that is not a number -- a zero pivot of a rank-deficient matrix -- goes the same way)
  const int sing = wave_uniform_i((n < 6 || !(fabsf(det) >= 1e-3f)) ? 1 : 0);
  if (sing) {
    pinv6_jacobi(X, s.J + 150, s.J + 186, lane);
    wi = 0.f;
#pragma unroll
    for (int k = 0; k < 6; k++) wi += s.J[186 + i * 6 + k] * ut[k];
  }
  if (lane < 6) w[lane] = wi;
  wave_sync();
  if (lane < 6 && real) {
    float u = s.bias[di];
#pragma unroll
    for (int k = 0; k < 6; k++) {   // (k: the k-th active dof in the first term -- a padding column has dq = 0 -- and task row k in the second)
      const int dk = da[k] >= 0 ? da[k] : 0;
      u -= (da[k] >= 0 ? g.kv * s.M[m_index(di, dk)] * s.qvel[dk] : 0.f) + Jm[k * 6 + lane] * w[k];
    }
    Uo[di] = u;
  }
  wave_sync();
  return sing;
}

template <class L>
JDEV void run_osc(const JacoOscArgs& Q_, L& s, int env, int lane) {
  // (the block is read through the kernarg segment pointer, an s_load per use; a by-value parameter indexed by the frame loop's counter
  // would be copied to scratch)
  const JacoOscArgs& Q = *kernarg_view(Q_);
  const JacoModelDev* m = opaque_ptr(Q.model);
  const int nq = m->nq, nv = m->nv, nu = m->nu, nf = Q.nframes;
  // this lane's ctrl word, read before anything is written (ctrl_out may be ctrl_in): moved as an integer
  unsigned word = 0u;
  if (lane < nu && Q.ctrl_in) word = reinterpret_cast<const unsigned*>(Q.ctrl_in)[(size_t)env * nu + lane];
  // the prologue of run_query: the state is exactly the floats handed in (low-order words zero)
  if (lane < nq) { s.qpos[lane] = Q.qpos[(size_t)env * nq + lane]; s.qpos_lo[lane] = 0.f; }
  if (lane < nv) { s.qvel[lane] = Q.qvel[(size_t)env * nv + lane]; s.qvel_lo[lane] = 0.f; }
  stage_model(m, s, lane);
  wave_sync();
  stage_walk(m, s, lane, false);
  for (int i = lane; i < JMBLK; i += 64) s.M[i] = 0.f;
  wave_sync();
  {
    const StagePrefetch pf = stage_prefetch(m, lane);
    stage_accumulate(m, s, lane);
    wave_sync();
    stage_mass_bias(m, s, lane, pf);
    wave_sync();
  }
  float* Uo = s.J + 224;   // [JNV] u_d by dof (behind stage_osc_frame's scratch)
  OscGains g;
  g.kp = Q.opt.kp; g.ko = Q.opt.ko; g.kv = Q.opt.kv; g.sat_xyz = Q.sat_xyz; g.sat_abg = Q.sat_abg;
  unsigned all = 0u;
  for (int f = 0; f < nf; f++) {   // wave-uniform; s.M, s.bias and s.cdof serve every frame
    // frame pose, every lane (same-address LDS reads): as run_query composes it
    const int b = Q.fr[f].body;
    const m3 Rb = ldm(s.xmat[b]);
    const v3 pf = ld3(s.xpos[b]) + mul(Rb, ld3(Q.fr[f].pos));
    const m3 R = mul(Rb, ldm(Q.fr[f].mat));
    const v3 p = pf + mul(R, ld3(Q.fr[f].point));
    const v3 pt = ld3(Q.target_pos + ((size_t)env * nf + f) * 3);
    const float* tq = Q.target_quat + ((size_t)env * nf + f) * 4;
    float qd[4] = {tq[0], tq[1], tq[2], tq[3]};
    const float qn = sqrtf(qd[0] * qd[0] + qd[1] * qd[1] + qd[2] * qd[2] + qd[3] * qd[3]);
    if (qn < JMINVAL) { qd[0] = 1.f; qd[1] = qd[2] = qd[3] = 0.f; } else { const float in = 1.f / qn; for (int k = 0; k < 4; k++) qd[k] *= in; }
    const unsigned act = Q.active[f];
    const int sing = stage_osc_frame(s, lane, act, p, R, pt, qd, g, Uo);
    if (lane == 0 && Q.status) Q.status[(size_t)env * nf + f] = sing;
    all |= act;
  }
  if (lane < nu) {   // the ctrl_in row with the motor of every active dof replaced: every other word goes out as it came in
    const int d = m->a_dof[lane];
    const bool mine = m->a_position[lane] == 0 && d >= 0 && d < nv && ((all >> (d >= 0 ? d : 0)) & 1u) != 0u;
    reinterpret_cast<unsigned*>(Q.ctrl_out)[(size_t)env * nu + lane] = mine ? __builtin_bit_cast(unsigned, Uo[mine ? d : 0]) : word;
  }
}

#if JACO_TU_HAS(11)
JACO_DEFINE_ENTRY(osc, JacoOscArgs, Q.nenv, run_osc)
#else
JACO_DECLARE_ENTRY(osc, JacoOscArgs)
#endif
