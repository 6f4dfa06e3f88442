// Batched joint-space controller and inverse dynamics (jaco_joint, include/jaco_env.h): abr_control's
// Joint(robot_config, kp, kv).generate(q, dq, target, target_velocity), with a feed-forward acceleration -- the torques that drive the
// arm to this configuration -- and its two degenerate forms, inverse dynamics (kp = kv = 0 with qacc_ff) and bias compensation
// (kp = kv = 0 and nothing else: abr_control's Floating).
//
// One 64-lane wavefront per env on the contact-free LDS type (JacoLDS<JacoArm>): run_osc's prologue and forward pass as they are
// (entry_state_forward: the state floats as handed in, low words zero, model tables, tree walk, subtree sums, mass matrix + bias --
// the values of a sim.forward() on the given state), then, with the active dof set A that the host half resolved (a wave-uniform mask):
//   e_d = q*_d - q_d                                   for a limited joint,
//   e_d = ((q*_d - q_d + pi) mod 2 pi) - pi            for an unlimited one (floor-style modulus: osc_task.h's resting term);  e = 0
//         without target_qpos.  abr_control wraps every joint; here a limited joint is never wrapped, on purpose: on Jaco joint 2 (a
//         range of about 266 degrees) the wrapped difference would send a 260 degree move the short way, through the limit;
//   s   = min(1, sat / max over A of |e_d|),  sat = vmax * kv / kp formed once on the host; applied only when vmax > 0 and kp > 0.  ONE
//         scale for every dof, so the move stays a straight line in joint space (jaco_ik scales max_step the same way);
//   a_d = qacc_ff_d + kp s e_d + kv (dq*_d - dq_d)     for d in A, 0 for every other dof; missing inputs count as zeros;
//   u_d = sum over k in A of M[d][k] a_k + qfrc_bias_d for d in A.  M: the submatrix of qM on A (the reference's M[arm, arm], as in osc.h;
//         not a Schur complement).  Joint damping (d_damping) is NOT compensated: qfrc_bias does not hold it, as in the reference.
// A is not limited to six dofs: the two-arm model's twelve motor dofs, or the 12-hinge arm, go in one call.
// Mapping: lane d owns dof d and row d of M; max |e| is a wave reduction (lanes outside A hold 0); the row sum walks A by bit scan of the
// wave-uniform mask -- a scalar loop -- and takes a_k from lane k by v_readlane.  No LDS beyond the forward pass's but the [JNV] output
// row at s.J[224, 224 + JNV) (the row area is free: stage_mass_bias is done with it), no scratch memory.
// Output: run_osc's epilogue, as osc_write_ctrl states it (run_osc holds a twin of it written out): the ctrl_in row with u_d at the motor actuator of every d in A, every other word
// moved as an integer; ctrl_out may be ctrl_in.  No clamping.  Nothing of a handle is read but the model.
// Listed at the tail of physics_kernel.h; the kernel is translation unit 13 (kernels.hip -DJACO_TU=13).
#pragma once
#include <cmath>
#include <string>

struct JacoJointOpts {   // = JacoJointOptions of include/jaco_env.h (static_assert in abi_agreement.h)
  float kp, kv, vmax;
  int reserved;
  unsigned long long dof_mask;   // 0: every hinge dof that has a motor actuator
};
struct JacoJointArgs {
  const JacoModelDev* model;
  const float* qpos;          // [nenv][nq]
  const float* qvel;          // [nenv][nv]
  const float* target_qpos;   // [nenv][nq] or nullptr: e = 0; read only at the qpos addresses of the active dofs
  const float* target_qvel;   // [nenv][nv] or nullptr: zeros
  const float* qacc_ff;       // [nenv][nv] or nullptr: zeros
  const float* ctrl_in;       // [nenv][nu] or nullptr: zeros
  float* ctrl_out;            // [nenv][nu]; may be ctrl_in
  int nenv;
  unsigned active;            // the active dofs, resolved by the host half (jaco_joint_resolve)
  unsigned wrap;              // those of them whose joint is unlimited: their error is wrapped into [-pi, pi)
  float kp, kv;
  float sat;                  // vmax * kv / kp (formed once, on the host); 0: no limiting
};

// The host half shared by jaco_joint (jaco_env.hip) and the emulator's entry: every argument check; then the active dof set (dof_mask,
// or every hinge dof with a motor actuator when that is 0), the dofs to wrap, the gains and the saturation level into the argument block,
// whose pointers the caller has filled in.  Returns an empty string, or what is wrong.
static inline std::string jaco_joint_resolve(const JacoModelDev& m, const JacoJointOpts& o, JacoJointArgs* Q) {
  if (!Q->ctrl_out) return "the output ctrl is required";
  if (!(o.kp >= 0.f) || !(o.kv >= 0.f) || !(o.vmax >= 0.f) || std::isinf(o.kp) || std::isinf(o.kv) || std::isinf(o.vmax))
    return "kp, kv and vmax must be finite and not negative";
  unsigned hinge = 0u, motor = 0u;
  for (int d = 0; d < m.nv; d++) if (m.d_qadr[d] >= 0) hinge |= 1u << d;
  for (int a = 0; a < m.nu; a++) if (m.a_position[a] == 0 && m.a_dof[a] >= 0 && m.a_dof[a] < m.nv) motor |= 1u << m.a_dof[a];
  const unsigned long long valid = m.nv >= 64 ? ~0ull : (1ull << m.nv) - 1ull;
  if (o.dof_mask & ~valid) return "dof_mask bit " + std::to_string(__builtin_ctzll(o.dof_mask & ~valid)) + " is at or beyond nv = " + std::to_string(m.nv);
  const unsigned a = o.dof_mask ? (unsigned)o.dof_mask : hinge & motor;
  if (a & ~hinge) return "active dof " + std::to_string(__builtin_ctz(a & ~hinge)) + " belongs to a free joint";
  if (a & ~motor) return "active dof " + std::to_string(__builtin_ctz(a & ~motor)) + " has no motor actuator";
  if (!a) return "empty active dof set (the model has no hinge dof with a motor actuator)";
  if (o.kp > 0.f && !Q->target_qpos) return "kp > 0 and the target qpos is missing (kp = 0: no position term)";
  unsigned wrap = 0u;
  for (int d = 0; d < m.nv; d++) if (((a >> d) & 1u) && !m.b_limited[m.d_body[d]]) wrap |= 1u << d;
  Q->active = a;
  Q->wrap = wrap;
  Q->kp = o.kp; Q->kv = o.kv;
  Q->sat = (o.vmax > 0.f && o.kp > 0.f) ? o.vmax * o.kv / o.kp : 0.f;
  return std::string();
}

template <class L>
JDEV void run_joint(const JacoJointArgs& Q_, L& s, int env, int lane) {
  static_assert(JNV <= 32, "the active dof set is a 32-bit mask");
  const JacoJointArgs& Q = *kernarg_view(Q_);   // (as run_osc reads its block)
  const JacoModelDev* m = opaque_ptr(Q.model);
  const int nq = m->nq, nv = m->nv, nu = m->nu;
  // this lane's ctrl word, read before anything is written (ctrl_out may be ctrl_in): moved as an integer
  unsigned word = 0u;
  if (lane < nu && Q.ctrl_in) word = reinterpret_cast<const unsigned*>(Q.ctrl_in)[(size_t)env * nu + lane];
  entry_state_forward(m, s, Q.qpos, Q.qvel, env, lane);
  const unsigned act = (unsigned)wave_uniform_i((int)Q.active);
  const bool mine = lane < nv && ((act >> (lane & 31)) & 1u) != 0u;   // (every active dof is < nv <= JNV)
  const int d = mine ? lane : 0;
  // e, this lane's dof: plain for a limited joint, wrapped for an unlimited one (a lane outside A: 0)
  float e = 0.f;
  if (mine && Q.target_qpos) {
    const int qa = m->d_qadr[d];
    const float x = Q.target_qpos[(size_t)env * nq + qa] - s.qpos[qa];
    const float y = x + 3.14159265358979f;
    e = ((Q.wrap >> d) & 1u) ? y - 6.28318530717959f * floorf(y * 0.159154943091895f) - 3.14159265358979f : x;
  }
  // one scale for every dof: the largest |e| over A (lanes outside A hold 0) against the saturation level
  float sc = 1.f;
  if (Q.sat > 0.f) {   // wave-uniform: a kernel argument
    const float mx = wave_max(fabsf(e));
    sc = mx > Q.sat ? Q.sat / mx : 1.f;
  }
  float a = 0.f;
  if (mine) {
    const float ff = Q.qacc_ff ? Q.qacc_ff[(size_t)env * nv + d] : 0.f;
    const float dqt = Q.target_qvel ? Q.target_qvel[(size_t)env * nv + d] : 0.f;
    a = ff + Q.kp * sc * e + Q.kv * (dqt - s.qvel[d]);
  }
  // u_d = sum over k in A of M[d][k] a_k + bias_d: a scalar loop over the set bits, a_k read from lane k (dofs of another tree: M is 0)
  float u = 0.f;
  for (unsigned mk = act; mk; mk &= mk - 1u) {
    const int k = __builtin_ctz(mk);
    const float ak = wave_bcast(a, k);
    const bool same = (d < JB0) == (k < JB0) && (d < JB1) == (k < JB1);
    u += same ? s.M[m_index(d, same ? k : d)] * ak : 0.f;
  }
  float* Uo = s.J + 224;   // [JNV] u_d by dof (where run_osc keeps it)
  if (mine) Uo[d] = u + s.bias[d];
  wave_sync();
  osc_write_ctrl(m, Q.ctrl_out, env, lane, act, word, Uo);
}

#if JACO_TU_HAS(13)
JACO_DEFINE_ENTRY(joint, JacoJointArgs, Q.nenv, run_joint)
#else
JACO_DECLARE_ENTRY(joint, JacoJointArgs)
#endif
