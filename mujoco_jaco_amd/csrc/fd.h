// Batched forward dynamics and its linearisation (jaco_fd, include/jaco_env.h): given state and ctrl, which acceleration results, and
// how does it change with the state and the ctrl?  MuJoCo's data.qacc_smooth after mj_forward, and a contact-free mjd_transitionFD.
//
// One 64-lane wavefront per env on the contact-free LDS type (JacoLDS<JacoArm>).  The state is exactly the floats handed in (low words
// zero) and stage_model runs once (entry_state); everything from the tree walk on is one pass (fd_pass) made of the step kernel's own stages, called
// as they are:
//   stage_walk, stage_accumulate, stage_mass_bias (s.smooth = passive - bias), stage_actuation with act_fetch's constants (ctrl clamped
//   to ctrlrange, kp (c - q) for the position servos, forcerange: s.smooth += qfrc_actuator), then row `lane` of the block-diagonal
//   mass matrix into registers and ldl_solve_blocks: qacc = M^-1 qfrc_smooth, or (M + h D)^-1 qfrc_smooth with implicit_damping (h D on
//   the diagonal of the damped block JDAMPED_BLOCKS only, as the Euler stage forms it).
// UNCONSTRAINED: no contact rows, no joint-limit rows.
// Mapping: lane d owns dof d and row d of M.
//   * dqacc_dctrl is analytic: actuator a's gate g_a (kp for a servo, 1 for a motor; 0 when ctrl_a is outside a limited ctrlrange or the
//     force sits at a forcerange end) is formed by lane a from the base state and read by v_readlane; one elimination of the dof's block
//     per actuator with the right-hand side g_a e_dof(a), the rows reloaded from s.M (still the base state's).  A closed gate skips the
//     elimination: the row is exactly 0.0.
//   * dqacc_dqpos / dqacc_dqvel: a wave-uniform bit scan of the resolved mask, plus / minus inside.  Lane 0 rewrites the one LDS state
//     word (x0 + eps, x0 - eps, then x0 again), fd_pass runs, the plus side's acceleration waits in a register, and the quotient by the
//     actual difference of the two rounded coordinates goes straight to global memory: row c of the output is one contiguous [nv] row, so
//     the lanes store consecutive words.  Rows the mask does not select are written as zeros.  A NULL output skips its loop.
// No LDS beyond the forward pass's, no scratch memory.  Nothing of a handle is read but the model.
// Listed at the tail of physics_kernel.h; the kernel is translation unit 14 (kernels.hip -DJACO_TU=14).
#pragma once
#include <cmath>
#include <string>

struct JacoFdOpts {   // = JacoFdOptions of include/jaco_env.h (static_assert in abi_agreement.h)
  float eps_qpos, eps_qvel;
  int implicit_damping;
  int reserved;
  unsigned long long dof_mask;   // 0: every hinge dof
};
struct JacoFdArgs {
  const JacoModelDev* model;
  const float* qpos;          // [nenv][nq]
  const float* qvel;          // [nenv][nv]
  const float* ctrl;          // [nenv][nu] or nullptr: zeros
  float* qacc;                // [nenv][nv] or nullptr
  float* qfrc_smooth;         // [nenv][nv] or nullptr
  float* dqacc_dqpos;         // [nenv][nv][nv] or nullptr: row c = d qacc / d qpos_c
  float* dqacc_dqvel;         // [nenv][nv][nv] or nullptr: row c = d qacc / d qvel_c
  float* dqacc_dctrl;         // [nenv][nu][nv] or nullptr: row a = d qacc / d ctrl_a
  int nenv;
  unsigned mask;              // the perturbed dofs, resolved by the host half (jaco_fd_resolve)
  float eps_qpos, eps_qvel;
  int implicit_damping;
};

// The host half shared by jaco_fd (jaco_env.hip) and the emulator's entry: every argument check, then the resolved mask (dof_mask, or
// every hinge dof when that is 0) and the steps into the argument block, whose pointers the caller has filled in (have_out: the output
// record was not NULL).  Returns an empty string, or what is wrong.
static inline std::string jaco_fd_resolve(const JacoModelDev& m, const JacoFdOpts& o, bool have_out, JacoFdArgs* Q) {
  if (!have_out) return "the output record is required";
  if (!Q->qacc && !Q->qfrc_smooth && !Q->dqacc_dqpos && !Q->dqacc_dqvel && !Q->dqacc_dctrl) return "at least one output is required";
  if (!(o.eps_qpos > 0.f) || !(o.eps_qvel > 0.f) || std::isinf(o.eps_qpos) || std::isinf(o.eps_qvel)) return "eps_qpos and eps_qvel must be finite and positive";
  if (o.implicit_damping != 0 && o.implicit_damping != 1) return "implicit_damping must be 0 or 1";
  unsigned hinge = 0u;
  for (int d = 0; d < m.nv; d++) if (m.d_qadr[d] >= 0) hinge |= 1u << d;
  const unsigned long long valid = m.nv >= 64 ? ~0ull : (1ull << m.nv) - 1ull;
  if (o.dof_mask & ~valid) return "dof_mask bit " + std::to_string(__builtin_ctzll(o.dof_mask & ~valid)) + " is at or beyond nv = " + std::to_string(m.nv);
  const unsigned a = o.dof_mask ? (unsigned)o.dof_mask : hinge;
  if (a & ~hinge) return "perturbed dof " + std::to_string(__builtin_ctz(a & ~hinge)) + " belongs to a free joint";
  Q->mask = a;
  Q->eps_qpos = o.eps_qpos; Q->eps_qvel = o.eps_qvel;
  Q->implicit_damping = o.implicit_damping;
  return std::string();
}

// row `lane` of M (mass_row) + hd on the diagonal; lanes >= nv hold identity rows
template <class L>
JDEV void fd_rows(float (&h)[JNV], const L& s, int lane, int nv, float hd) {
  mass_row(h, s, lane, nv);
#pragma unroll
  for (int j = 0; j < JNV; j++) h[j] += lane == j ? (lane < nv ? hd : 1.f) : 0.f;
}

// h D of the Euler stage for this lane's dof: on the damped block only
JDEV float fd_hdamp(const JacoModelDev* m, int lane, int implicit, float damping) {
  return (implicit && m->has_damping && lane < m->nv && lane < JB0 && (JDAMPED_BLOCKS & 1)) ? m->timestep * damping : 0.f;
}

// One forward pass from the tree walk on, on the state in LDS: leaves s.M, s.bias and s.smooth (= qfrc_smooth) behind, returns qacc.
template <class L>
JDEV float fd_pass(const JacoModelDev* m, L& s, int lane, int implicit, int blockmask) {
  // (as run_env's substep loop: with the pointer's provenance and the lane id hidden, the optimiser cannot hoist the pass's model loads
  // and lane-derived addresses out of the perturbation loop and keep them alive, spilled, across all of it)
  m = opaque_ptr(m);
  lane = wave_opaque_i(lane);
  const int nv = m->nv;
  entry_walk(m, s, lane);
  // (fetched per pass, as the step kernel fetches them per substep: held over the whole loop they would cost the solve its registers)
  const ActParams actp = act_fetch(m, lane);
  const StagePrefetch pf = entry_mass_bias(m, s, lane);
  stage_actuation(m, s, lane, actp);
  wave_sync();
  float h[JNV];
  fd_rows(h, s, lane, nv, fd_hdamp(m, lane, implicit, pf.damping));
  const float smooth = lane < nv ? s.smooth[lane] : 0.f;
  return ldl_solve_blocks(h, smooth, lane, blockmask);
}

template <class L>
JDEV void run_fd(const JacoFdArgs& Q_, L& s, int env, int lane) {
  static_assert(JNV <= 32, "the perturbed dof set is a 32-bit mask");
  const JacoFdArgs& Q = *kernarg_view(Q_);   // (as run_osc reads its block)
  const JacoModelDev* m = opaque_ptr(Q.model);
  const int nv = m->nv, nu = m->nu;
  entry_state<ENTRY_CTRL>(m, s, Q.qpos, Q.qvel, Q.ctrl, env, lane);
  const int implicit = Q.implicit_damping;
  const int blockmask = 1 | (nv > JB0 ? 2 : 0) | (nv > JB1 ? 4 : 0);
  const float qacc = fd_pass(m, s, lane, implicit, blockmask);
  if (lane < nv) {
    if (Q.qacc) Q.qacc[(size_t)env * nv + lane] = qacc;
    if (Q.qfrc_smooth) Q.qfrc_smooth[(size_t)env * nv + lane] = s.smooth[lane];
  }
  if (Q.dqacc_dctrl) {   // analytic, on the base state's M (still in s.M)
    const ActParams actp = act_fetch(m, lane);
    const float hd = fd_hdamp(m, lane, implicit, m->d_damping[lane < JNV ? lane : 0]);
    float g = 0.f;       // lane a: the gate of actuator a
    if (lane < nu) {
      const float c = s.ctrl[lane];
      const bool ctrl_open = !actp.ctrllimited || (c >= actp.c0 && c <= actp.c1);
      const float f = actp.position ? actp.kp * (c - s.qpos[actp.qadr]) : c;
      const bool force_open = !actp.forcelimited || (f > actp.f0 && f < actp.f1);
      g = (ctrl_open && force_open) ? (actp.position ? actp.kp : 1.f) : 0.f;
    }
    for (int a = 0; a < nu; a++) {
      const float ga = wave_bcast(g, a);
      const int dof = wave_bcast_i(actp.dof, a);
      float x = 0.f;
      if (ga != 0.f) {   // (wave-uniform)
        float h[JNV];
        fd_rows(h, s, lane, nv, hd);
        x = ldl_solve_blocks(h, lane == dof ? ga : 0.f, lane, dof < JB0 ? 1 : (dof < JB1 ? 2 : 4));
      }
      if (lane < nv) Q.dqacc_dctrl[((size_t)env * nu + a) * nv + lane] = x;
    }
  }
  wave_sync();
  const unsigned mask = (unsigned)wave_uniform_i((int)Q.mask);
  const unsigned all = nv >= 32 ? ~0u : (1u << nv) - 1u;
  for (int kind = 0; kind < 2; kind++) {   // 0: qpos, 1: qvel
    float* out = kind ? Q.dqacc_dqvel : Q.dqacc_dqpos;
    if (!out) continue;
    const float eps = kind ? Q.eps_qvel : Q.eps_qpos;
    for (unsigned z = all & ~mask; z; z &= z - 1u) {
      const int c = __builtin_ctz(z);
      if (lane < nv) out[((size_t)env * nv + c) * nv + lane] = 0.f;
    }
    for (unsigned mk = mask; mk; mk &= mk - 1u) {
      const int c = __builtin_ctz(mk);
      float* w = kind ? &s.qvel[c] : &s.qpos[m->d_qadr[c]];
      const float x0 = *w, xp = x0 + eps, xm = x0 - eps;
      wave_sync();
      float ap = 0.f, quot = 0.f;
#pragma nounroll
      for (int side = 0; side < 2; side++) {
        if (lane == 0) *w = side ? xm : xp;
        wave_sync();
        const float a = fd_pass(m, s, lane, implicit, blockmask);
        if (side == 0) ap = a; else quot = (ap - a) * (1.f / (xp - xm));
      }
      if (lane == 0) *w = x0;
      if (lane < nv) out[((size_t)env * nv + c) * nv + lane] = quot;
      wave_sync();
    }
  }
}

#if JACO_TU_HAS(14)
JACO_DEFINE_ENTRY(fd, JacoFdArgs, Q.nenv, run_fd)
#else
JACO_DECLARE_ENTRY(fd, JacoFdArgs)
#endif
