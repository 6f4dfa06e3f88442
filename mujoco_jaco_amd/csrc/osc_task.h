// Operational-space controller with task axes and null-space posture terms (jaco_osc_task, include/jaco_env.h): abr_control's
// OSC(robot_config, kp, ko, kv, vmax, ctrlr_dof, null_controllers=[Damping, RestingConfig]).generate().
//
// run_osc of osc.h with another per-frame stage: the same forward pass (entry_state, entry_forward), the same frame pose, then stage_osc_task_frame.
// With rows = the task rows that the frame's 6-bit axis mask selects (k of them) and Js = J[rows]:
//   X  = Js M^-1 Js^T (k x k);  Mx = X^-1 when n >= k and |det X| >= 1e-3, else the pseudo-inverse that drops singular values < 0.005;
//   u_task as in osc.h (both halves saturated on their full three components, then the gains), then its selected rows;
//   z  = -null_kv dq + [d held] (rest_kp e_d - rest_kv dq_d),  e_d = ((rest_d - q_d + pi) mod 2 pi) - pi;   u_null = M z;
//   u  = -kv M dq - Js^T Mx (u_task[rows] + Js z) + u_null + bias.
// The last line is abr_control's u + (I - Js^T Jbar^T) u_null with Jbar = M^-1 Js^T Mx: M^-1 u_null is z itself, so the filter needs no
// solve against M, and Mx is linear, so the filter's product rides on the primary term's right-hand side: one elimination (or one
// 6 x 6 product in the pseudo-inverse branch) serves both.
// The 6 x 6 machinery of osc.h is kept by padding: the unselected rows of J are zero, the unselected diagonal of X is 1, the unselected
// entries of the right-hand side are 0.  Then the determinant and the inverse block are those of the k x k matrix, and the padding's
// singular values are 1 and never dropped.  n < k (exactly rank deficient) is decided from the two counts, both wave-uniform scalars.
// Scratch: stage_osc_frame's s.J[0, 222), Uo at s.J[224, 224 + JNV), and s.J[256, 268) behind it for z and the right-hand side.
// Listed at the tail of physics_kernel.h; the kernel is translation unit 12 (kernels.hip -DJACO_TU=12).
#pragma once
#include <cmath>

struct JacoOscTaskOpts {   // = JacoOscTask of include/jaco_env.h (static_assert in abi_agreement.h)
  unsigned axes[JOSC_MAXFRAMES];   // bit r = task row r; 0 = all six
  float null_kv, rest_kp, rest_kv;
  int reserved;
  unsigned long long rest_mask;    // 0: every active dof
};
struct JacoOscTaskArgs {
  JacoOscArgs o;                     // as jaco_osc's; o.target_quat may be nullptr when no frame selects a rotational row
  const float* rest_qpos;            // [nenv][nq] or nullptr: no resting term
  unsigned axes[JOSC_MAXFRAMES];     // resolved: 1 .. 63
  unsigned held[JOSC_MAXFRAMES];     // the dofs the resting term holds (a subset of o.active[f]); 0 without the term
  float null_kv, rest_kp, rest_kv;
};

// The host half shared by jaco_osc_task (jaco_env.hip) and the emulator's entry: jaco_osc_resolve, then the checks of the task record.
// T->o's pointers and T->rest_qpos are filled in by the caller.  Returns an empty string, or what is wrong.
static inline std::string jaco_osc_task_resolve(const JacoModelDev& m, const JacoQueryFrame* frames, int nframes, const JacoOscOpts& o,
                                                const JacoOscTaskOpts& t, JacoOscTaskArgs* T) {
  const float* const tq = T->o.target_quat;
  if (nframes >= 1 && nframes <= JOSC_MAXFRAMES) {
    for (int f = 0; f < nframes; f++) {
      const std::string who = "frame " + std::to_string(f) + ": ";
      if (t.axes[f] & ~63u) return who + "axes " + std::to_string(t.axes[f]) + " has bits above bit 5";
      T->axes[f] = t.axes[f] ? t.axes[f] : 63u;
      if (!tq && (T->axes[f] & 56u)) return who + "a rotational axis is selected and the target quaternions are missing";
    }
    if (!tq) T->o.target_quat = T->o.target_pos;   // (no rotational row anywhere: jaco_osc_resolve's "required" does not apply to it)
  }
  const std::string why = jaco_osc_resolve(m, frames, nframes, o, &T->o);
  T->o.target_quat = tq;
  if (!why.empty()) return why;
  if (!(t.null_kv >= 0.f) || !(t.rest_kp >= 0.f) || !(t.rest_kv >= 0.f) || std::isinf(t.null_kv) || std::isinf(t.rest_kp) || std::isinf(t.rest_kv))
    return "null_kv, rest_kp and rest_kv must be finite and not negative";
  for (int f = 0; f < nframes; f++) {
    T->held[f] = 0u;
    if (!T->rest_qpos) continue;
    T->held[f] = t.rest_mask ? T->o.active[f] & (unsigned)(t.rest_mask & 0xffffffffull) : T->o.active[f];
    if (!T->held[f]) return "frame " + std::to_string(f) + ": rest_mask leaves none of its active dofs";
  }
  T->null_kv = t.null_kv; T->rest_kp = t.rest_kp; T->rest_kv = t.rest_kv;
  return std::string();
}

struct OscNull { float null_kv, rest_kp, rest_kv; unsigned held; const float* rest; };   // rest: this env's row, or nullptr

// stage_osc_frame (osc.h) on the task rows `axes` (1 .. 63) with the null-space terms `nl`; same needs, same outputs.  m: the model (the
// qpos address of a held dof).  Scratch: s.J[0, 222) and s.J[256, 268).
template <class L>
JDEV int stage_osc_task_frame(const JacoModelDev* m, L& s, int lane, unsigned active, unsigned axes, const v3 pe, const m3& Re, const v3 pt,
                              const float (&qd)[4], const OscGains& g, const OscNull& nl, float* Uo) {
  static_assert(224 + JNV <= 256 && 268 <= sizeof(s.J) / sizeof(float), "the scratch behind Uo must lie inside the row area");
  float* Jm = s.J;            // [6][6] Js padded: J[r][c] of the selected rows r, zero rows otherwise; columns: active dofs
  float* T = s.J + 72;        // M^-1 Js^T
  float* X = s.J + 108;       // Js M^-1 Js^T with 1 on the unselected diagonal, then its (pseudo-)inverse
  float* w = s.J + 144;       // Mx (u_task + Js z)
  float* Z = s.J + 256;       // [6] z by active dof
  float* Rh = s.J + 262;      // [6] the right-hand side u_task + Js z
  int da[6], n = 0;
  {
    unsigned mk = (unsigned)wave_uniform_i((int)active);
#pragma unroll
    for (int k = 0; k < 6; k++) { da[k] = mk ? __builtin_ctz(mk) : -1; n += mk ? 1 : 0; mk &= mk - 1u; }
  }
  const unsigned ax = (unsigned)wave_uniform_i((int)axes);
  const int nrows = __builtin_popcount(ax);
  const int r = lane / 6, c = lane - 6 * r;   // lanes 0..35 = matrix entry (r, c)
  const int i = lane < 6 ? lane : 0;
  int di = da[0];
#pragma unroll
  for (int j = 1; j < 6; j++) di = i == j ? da[j] : di;
  const bool real = di >= 0;   // (a padding row / column otherwise)
  const int ds = real ? di : 0;
  // T = M^-1 Js^T by elimination on [M | Js^T] (lanes 0..5 own rows; row i of Js^T is this lane's own Jacobian column, selected rows)
  float A[6], B[6];
  {
    sv S = ldsv(s.cdof[ds]);
    v3 jp = S.b + cross(S.a, pe);
    const float col[6] = {jp.x, jp.y, jp.z, S.a.x, S.a.y, S.a.z};
#pragma unroll
    for (int k = 0; k < 6; k++) B[k] = (real && ((ax >> k) & 1u)) ? col[k] : 0.f;
  }
  if (lane < 6) {
#pragma unroll
    for (int k = 0; k < 6; k++) Jm[k * 6 + lane] = B[k];
  }
#pragma unroll
  for (int j = 0; j < 6; j++) A[j] = (real && da[j] >= 0) ? s.M[m_index(ds, da[j] >= 0 ? da[j] : 0)] : (i == j ? 1.f : 0.f);
  // z, this lane's dof: the null-space terms before M (a padding lane: 0)
  const bool has_null = nl.null_kv != 0.f || nl.rest != nullptr;   // wave-uniform: kernel arguments
  if (has_null) {
    float z = 0.f;
    if (lane < 6 && real) {
      const float dq = s.qvel[di];
      z = -nl.null_kv * dq;
      if (nl.rest && ((nl.held >> di) & 1u)) {
        const int qa = m->d_qadr[di];
        const float x = nl.rest[qa] - s.qpos[qa] + 3.14159265358979f;
        const float e = x - 6.28318530717959f * floorf(x * 0.159154943091895f) - 3.14159265358979f;
        z += nl.rest_kp * e - nl.rest_kv * dq;
      }
    }
    if (lane < 6) Z[lane] = z;
  }
  gj_inverse6(A, B, lane);
  if (lane < 6) for (int j = 0; j < 6; j++) T[lane * 6 + j] = B[j];
  wave_sync();
  if (lane < 36) {
    float a = 0.f;
    for (int k = 0; k < 6; k++) a += Jm[r * 6 + k] * T[k * 6 + c];
    X[lane] = (r == c && !((ax >> r) & 1u)) ? 1.f : a;
  }
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
  // velocity limiting on the full halves, then the gains, and only then the selected rows (abr_control's order)
  float nx = sqrtf(ut[0] * ut[0] + ut[1] * ut[1] + ut[2] * ut[2]), na = sqrtf(ut[3] * ut[3] + ut[4] * ut[4] + ut[5] * ut[5]);
  float sx = nx > g.sat_xyz ? g.sat_xyz / nx : 1.f, sa = na > g.sat_abg ? g.sat_abg / na : 1.f;
  for (int k = 0; k < 3; k++) { ut[k] *= g.kp * sx; ut[3 + k] *= g.ko * sa; }
#pragma unroll
  for (int k = 0; k < 6; k++) ut[k] = ((ax >> k) & 1u) ? ut[k] : 0.f;
  // the right-hand side, lane i = task row i: u_task + Js z (a zero row of Js keeps an unselected entry 0), and this lane's (M z)_i
  float wi = ut[0];
#pragma unroll
  for (int j = 1; j < 6; j++) wi = i == j ? ut[j] : wi;
  float un = 0.f;
  if (has_null) {
#pragma unroll
    for (int k = 0; k < 6; k++) {
      const float zk = Z[k];
      wi += Jm[i * 6 + k] * zk;
      un += (real && da[k] >= 0) ? s.M[m_index(ds, da[k] >= 0 ? da[k] : 0)] * zk : 0.f;
    }
  }
  if (lane < 6) Rh[lane] = wi;
  // w = Mx rhs:  Mx = X^-1 as a solve when n >= k and |det X| >= 1e-3, else the SVD pseudo-inverse that drops singular values < 0.005
#pragma unroll
  for (int j = 0; j < 6; j++) A[j] = X[i * 6 + j];
  float det = gj_solve6(A, wi, lane);
  // (a scalar branch; "not >=" so that a determinant that is not a number goes the same way; n < k: exactly rank deficient)
  const int sing = wave_uniform_i((n < nrows || !(fabsf(det) >= 1e-3f)) ? 1 : 0);
  if (sing) {
    pinv6_jacobi(X, s.J + 150, s.J + 186, lane);
    wi = 0.f;
#pragma unroll
    for (int k = 0; k < 6; k++) wi += s.J[186 + i * 6 + k] * Rh[k];
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
    Uo[di] = u + un;
  }
  wave_sync();
  return sing;
}

template <class L>
JDEV void run_osc_task(const JacoOscTaskArgs& T_, L& s, int env, int lane) {
  const JacoOscTaskArgs& T = *kernarg_view(T_);   // (as run_osc reads its block)
  const JacoOscArgs& Q = T.o;
  const JacoModelDev* m = opaque_ptr(Q.model);
  const int nq = m->nq, nf = Q.nframes;
  const unsigned word = osc_read_ctrl(Q.ctrl_in, env, lane, m->nu);
  entry_state(m, s, Q.qpos, Q.qvel, nullptr, env, lane);
  entry_forward(m, s, lane);
  float* Uo = s.J + 224;   // [JNV] u_d by dof
  const OscGains g = osc_gains(Q);
  OscNull nl;
  nl.null_kv = T.null_kv; nl.rest_kp = T.rest_kp; nl.rest_kv = T.rest_kv;
  nl.rest = T.rest_qpos ? T.rest_qpos + (size_t)env * nq : nullptr;
  unsigned all = 0u;
  for (int f = 0; f < nf; f++) {   // wave-uniform
    v3 p;
    m3 R;
    body_frame_pose(s, Q.fr[f], &p, &R);   // (the host half lets no world-fixed frame through)
    p = frame_point(p, R, Q.fr[f]);
    const v3 pt = ld3(Q.target_pos + ((size_t)env * nf + f) * 3);
    const unsigned axes = T.axes[f];
    float qd[4] = {1.f, 0.f, 0.f, 0.f};   // (no rotational row: the quaternions are not read, they may be missing)
    if (axes & 56u) osc_unit_quat(Q.target_quat + ((size_t)env * nf + f) * 4, qd);
    const unsigned act = Q.active[f];
    nl.held = T.held[f];
    const int sing = stage_osc_task_frame(m, s, lane, act, axes, p, R, pt, qd, g, nl, Uo);
    if (lane == 0 && Q.status) Q.status[(size_t)env * nf + f] = sing;
    all |= act;
  }
  osc_write_ctrl(m, Q.ctrl_out, env, lane, all, word, Uo);
}

#if JACO_TU_HAS(12)
JACO_DEFINE_ENTRY(osc_task, JacoOscTaskArgs, Q.o.nenv, run_osc_task)
#else
JACO_DECLARE_ENTRY(osc_task, JacoOscTaskArgs)
#endif
