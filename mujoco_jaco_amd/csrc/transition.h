// Transition Jacobians of the rollout step (jaco_transition_fd, include/jaco_env.h): how does the state after `hold` substeps change with
// the state and the ctrl it started from?  MuJoCo's mjd_transitionFD on the rollouts' own step function, batched over n (state, ctrl)
// pairs that are inputs -- every knot of every trajectory, straight from jaco_rollout_fb's outputs -- and so all run in parallel.
//
// One 64-lane wavefront per work item on JacoLDS<JacoArm>; the grid is n * groups, item w serves pair i = w / groups and the columns c
// with c % groups == w % groups, ascending.  Columns: nd position words of the chosen hinge dofs, nd velocity words, na chosen ctrl words
// (ncol = 2 nd + na; the dof list is jaco_rollout_fb's, checked by the same function).  stage_model runs once per work item.
// AN EVALUATION restores the start exactly as a rollout starts (transition_restore: row i into the high words, low words zero, zero warm
// start, zero row counters, s.ctrl = row i of ctrl: loads of one row, no second prologue), lane 0 rewrites the one perturbed word
// (x0 + eps or x0 - eps in fp32), and entry_walk + rollout_substep of rollout.h -- called as it is, limit rows, warm-started Newton solve,
// compensated Euler stage and position update included -- run `hold` times.  The nominal evaluation is jaco_rollout(nknots = 1) bit for bit.
// THE INCREMENT FORM (the order of operations is part of the interface: tests recompute it).  Lane j < nx forms after the last substep
//   D_j = (x'_j.hi - xs_j) + x'_j.lo      as TWO fp32 words:  D_j.hi = fl(x'_j.hi - xs_j),  D_j.lo = e_j + x'_j.lo
// xs_j its start word: word j of the pair's row, or the perturbed word where j is the perturbed coordinate (formed again from the row
// by the same fp32 operation, not carried); e_j the rounding error of that subtraction, exactly (two-sum, transition_increment)
// -- the increment, exact to the low word, where the difference of two end states would carry the fp32 rounding of a joint angle divided
// by 2 eps.  The second word is what makes that true of velocities as well: x'.hi - xs is an exact fp32 subtraction while x'.hi stays
// within a factor 2 of xs (a joint angle over a few substeps), not for a velocity that decays or changes sign, and rounded to one word
// D would be off by up to half a spacing of xs, over 2 eps.  A column is
//   (((r == c ? S.hi : 0.0f) + H.hi) + (H.lo + (D_r(+).lo - D_r(-).lo) + (r == c ? S.lo : 0.0f))) * (1.0f / S.hi)      (B: no own term)
// H = D_r(+).hi - D_r(-).hi as two words likewise,
// S = c(+) - c(-) as two words (S.hi the fp32 difference, S.lo its exact rounding error) -- the identity as the step itself, added
// before the quotient; forward differences (centered = 0) take D_r(+) - D_r(0) and c(+) - c0, each group running the nominal
// once.
// Lane r stores entry [r][c]: stride nx (A) or na (B) words, every entry written exactly once, in the layout jaco_lqr reads.
// Per lane only D(+) (or D(0)) and loop state live across an evaluation; the argument block, the model pointer and the lane id are
// re-read per substep as run_rollout and fd_pass do, for the reason written there, and the block is read afresh (transition_args) on
// either side of an evaluation too: what it says of the dof list, the mode and the outputs would otherwise wait in scalar registers
// across the substeps, which have none to spare, and be spilled into vector registers.
// The nominal also runs in group 0 when next_qpos, next_qvel or status is asked for; no result depends on groups or on which outputs are
// asked for.  No LDS beyond the step's, no scratch memory.  Nothing of a handle is read but the model (and its fp32 state when no state is
// given).  Listed at the tail of physics_kernel.h; the kernel is translation unit 20 (kernels.hip -DJACO_TU=20).
#pragma once
#include <cmath>
#include <string>

#define JTRANSITION_MAX_HOLD 1024   // = JACO_TRANSITION_MAX_HOLD
struct JacoTransitionOpts {   // = JacoTransitionOptions of include/jaco_env.h (static_assert in abi_agreement.h)
  int hold, centered, groups;
  int ndofs;
  int dofs[JROLLOUT_FB_MAX_DOFS];
  int nacts;
  int acts[JROLLOUT_FB_MAX_DOFS];
  float eps_qpos, eps_qvel, eps_ctrl;
  int reserved;
};
struct JacoTransitionOutp {   // = JacoTransitionOut of include/jaco_env.h
  float* A;
  float* B;
  float* next_qpos;
  float* next_qvel;
  unsigned* status;
};
struct JacoTransitionArgs {
  const JacoModelDev* model;
  const float* qpos;          // [n][nq]  (the handle's hi words, or the caller's)
  const float* qvel;          // [n][nv]
  const float* ctrl;          // [n][nu] or nullptr: zeros
  float* A;                   // [n][nx][nx] or nullptr
  float* B;                   // [n][nx][na] or nullptr
  float* next_qpos;           // [n][nq] or nullptr
  float* next_qvel;           // [n][nv] or nullptr
  unsigned* status;           // [n] or nullptr
  int n, groups, hold, centered, ndofs, nacts;
  float eps_qpos, eps_qvel, eps_ctrl;
  int dofs[JROLLOUT_FB_MAX_DOFS], acts[JROLLOUT_FB_MAX_DOFS];
};

// The library's choice for groups = 0: as many column groups as it takes to reach JTRANSITION_FILL work items, at most one group per
// column.  Measured on the MI355X at 27 columns (profiles/transition_fd_bench.txt): one group per column is the fastest at 64 pairs
// (0.041 ms against 0.48 ms for one group) and still at 4 096 (110 592 items: 0.67 against 0.76 ms); at 204 800 pairs one group and
// three tie (30.7 ms), nine cost 2 % and 27 cost 4.5 %: each further work item pays stage_model and a launch slot for fewer evaluations.
#define JTRANSITION_FILL 131072
static inline int jaco_transition_groups(int n, int ncol) {
  if (n < 1) return 1;
  const int g = (JTRANSITION_FILL + n - 1) / n;
  return g < 1 ? 1 : (g > ncol ? ncol : g);
}

// The host half shared by jaco_transition_fd (jaco_env.hip) and the emulator's entry: every refusal, then the options into the argument
// block, whose pointers the caller has filled in as they were handed over (qpos / qvel nullptr: the handle's state of num_envs rows, which
// the caller puts in afterwards; have_out: the output record was not NULL).  Returns an empty string, or what is wrong.
static inline std::string jaco_transition_resolve(const JacoModelDev& m, const JacoTransitionOpts* o, int n, int num_envs, bool have_out, JacoTransitionArgs* Q) {
  if (!o) return "the options are required";
  if (o->hold < 1 || o->hold > JTRANSITION_MAX_HOLD) return "hold " + std::to_string(o->hold) + " outside [1, " + std::to_string(JTRANSITION_MAX_HOLD) + "]";
  if (o->centered != 0 && o->centered != 1) return "centered must be 0 or 1";
  if (n < 0) return "n " + std::to_string(n) + " is negative";
  if (!have_out) return "the output record is required";
  if (!Q->A && !Q->B && !Q->next_qpos && !Q->next_qvel && !Q->status) return "at least one of the outputs A, B, next_qpos, next_qvel and status is required";
  if ((Q->qpos != nullptr) != (Q->qvel != nullptr)) return "qpos and qvel are given together or not at all";
  if (!Q->qpos && n != num_envs) return "n " + std::to_string(n) + " with the handle's state of " + std::to_string(num_envs) + " envs";
  if (!(o->eps_qpos > 0.f) || !(o->eps_qvel > 0.f) || !(o->eps_ctrl > 0.f) || std::isinf(o->eps_qpos) || std::isinf(o->eps_qvel) || std::isinf(o->eps_ctrl))
    return "eps_qpos, eps_qvel and eps_ctrl must be finite and positive";
  {
    JacoRolloutFbArgs F{};   // (the dof list is jaco_rollout_fb's: its check, its messages)
    const std::string why = jaco_rollout_fb_dofs(m, o->ndofs, o->dofs, &F);
    if (!why.empty()) return why;
    for (int j = 0; j < F.ndofs; j++) Q->dofs[j] = F.dofs[j];
    Q->ndofs = F.ndofs;
  }
  if (o->nacts < 0 || o->nacts > JROLLOUT_FB_MAX_DOFS) return "nacts " + std::to_string(o->nacts) + " outside [0, " + std::to_string(JROLLOUT_FB_MAX_DOFS) + "]";
  for (int j = 0; j < o->nacts; j++) {
    const int a = o->acts[j];
    if (a < 0 || a >= m.nu) return "ctrl word " + std::to_string(a) + " outside [0, " + std::to_string(m.nu) + ")";
    for (int k = 0; k < j; k++) if (o->acts[k] == a) return "ctrl word " + std::to_string(a) + " is listed twice";
    Q->acts[j] = a;
  }
  Q->nacts = o->nacts;
  if (Q->B && o->nacts < 1) return "B needs at least one ctrl word";
  const int ncol = 2 * Q->ndofs + Q->nacts;
  if (o->groups < 0 || o->groups > ncol) return "groups " + std::to_string(o->groups) + " outside [0, " + std::to_string(ncol) + "]";
  // (the library's choice: one group when no column is asked for -- the nominal is group 0's alone, any other group would only stage the model)
  Q->groups = o->groups ? o->groups : ((Q->A || Q->B) ? jaco_transition_groups(n, ncol) : 1);
  if ((long long)n * Q->groups > 0x7fffffffLL) return "n " + std::to_string(n) + " x groups " + std::to_string(Q->groups) + " is beyond the largest grid";
  Q->n = n; Q->hold = o->hold; Q->centered = o->centered;
  Q->eps_qpos = o->eps_qpos; Q->eps_qvel = o->eps_qvel; Q->eps_ctrl = o->eps_ctrl;
  return std::string();
}

// The start of an evaluation: pair i exactly as a rollout starts from it (entry_state<ENTRY_SUBSTEPS> without its stage_model call, plus
// the ctrl row a rollout loads per knot).
template <class L>
JDEV void transition_restore(const JacoTransitionArgs* Q, const JacoModelDev* m, L& s, int i, int lane) {
  const int nq = m->nq, nv = m->nv, nu = m->nu;
  if (lane < nq) { s.qpos[lane] = Q->qpos[(size_t)i * nq + lane]; s.qpos_lo[lane] = 0.f; }
  if (lane < nv) { s.qvel[lane] = Q->qvel[(size_t)i * nv + lane]; s.qvel_lo[lane] = 0.f; s.qacc_ws[lane] = 0.f; }
  if (lane < nu) s.ctrl[lane] = Q->ctrl ? Q->ctrl[(size_t)i * nu + lane] : 0.f;
  if (lane == 0) { s.ncon = 0; s.nefc = 0; s.ncand = 0; s.nlimit = 0; s.nsphere = 0; s.nside = 0; s.nside_cand = 0; }
  wave_sync();
}

// An increment as an unevaluated sum of two fp32 words: hi = fl(x'.hi - xs), lo = the exact rounding error of that subtraction (Knuth's
// two-sum: exact whatever the magnitudes) + x'.lo.
struct TransitionInc { float hi, lo; };
// Where the kept increment's low word waits during an evaluation.  0: in a register of its own.  1: in the flags word handed to
// rollout_substep -- for the d30 layout alone, which has no register left for it (129 VGPRs with one, 128 without).  THIS RESTS ON WHAT
// rollout_substep (rollout.h) DOES WITH THE WORD when no law is passed: it never reads it and only ever ORs JFLAG_SOLVER_MAXITER and
// JFLAG_NAN into it.  Those two bit positions of the carried word wait in two wave ballots (scalar registers) and are put back after
// the evaluation, so the carry is exact; a substep that set any other bit, or read the word, would corrupt the columns of the d30 build
// -- which the two-arm model's cases of tests/transition_binding.py (the formula recomputed from jaco_rollout on every hinge dof, the
// groups and the forward differences, where the word waits over many evaluations) would show, on the emulator and on the device.
#ifndef JTRANSITION_CARRY_IN_FLAGS
#define JTRANSITION_CARRY_IN_FLAGS (JNV > 24)
#endif
#define TRANSITION_STATUS0 ((unsigned)JFLAG_NAN)
#define TRANSITION_STATUS1 ((unsigned)JFLAG_SOLVER_MAXITER)
#define TRANSITION_STATUS (TRANSITION_STATUS0 | TRANSITION_STATUS1)
static_assert(TRANSITION_STATUS0 != TRANSITION_STATUS1 && (TRANSITION_STATUS0 & (TRANSITION_STATUS0 - 1u)) == 0u && (TRANSITION_STATUS1 & (TRANSITION_STATUS1 - 1u)) == 0u,
              "the two status bits rollout_substep sets are two single bits: each waits in one wave ballot");
JDEV TransitionInc transition_increment(float xhi, float xlo, float xs) {
  const float d = xhi - xs, v = d - xhi;
  const float err = (xhi - (d - v)) + (-xs - v);
  return TransitionInc{d, err + xlo};
}
// (own + ((a.hi - b.hi) + (a.lo - b.lo))) * (reciprocal); own: the step c(+) - c(-) itself for the column's own coordinate, where the
// entry is 1 + dD / step, and 0.0f elsewhere.  The identity goes in BEFORE the quotient: a strongly damped velocity (a finger under its
// servo) has dD / step near -1, and 1.0f + that would keep the product's rounding at the size of 1, not of the entry.
// (own: as two words, the second the exact rounding error of the step's own subtraction -- with dD / step near -1 that error, 2^-25 of
// the step, is as large against the entry as the entry is small against 1)
JDEV float transition_entry(TransitionInc own, TransitionInc a, TransitionInc b, float rcp) {
  const TransitionInc d = transition_increment(a.hi, a.lo - b.lo, b.hi);   // a.hi - b.hi without its rounding, and the low words' difference
  return ((own.hi + d.hi) + (d.lo + own.lo)) * rcp;
}

// Column c of pair i: the word it perturbs as handed in (x0; a NULL ctrl: 0.0f) and the two perturbed words as fp32 rounds them.
struct TransitionStep { float x0, xp, xm; };
JDEV TransitionStep transition_step(const JacoTransitionArgs* Q, const JacoModelDev* m, int i, int c) {
  const int nd = Q->ndofs, nx = 2 * nd;
  float x0, eps;
  if (c < nd) { x0 = Q->qpos[(size_t)i * m->nq + m->d_qadr[Q->dofs[c]]]; eps = Q->eps_qpos; }
  else if (c < nx) { x0 = Q->qvel[(size_t)i * m->nv + Q->dofs[c - nd]]; eps = Q->eps_qvel; }
  else { x0 = Q->ctrl ? Q->ctrl[(size_t)i * m->nu + Q->acts[c - nx]] : 0.f; eps = Q->eps_ctrl; }
  return TransitionStep{x0, x0 + eps, x0 - eps};
}

// The argument block read afresh from the kernarg segment, the pointer's provenance hidden (args_view's twin for this block): what is
// loaded through it is loaded again after an evaluation, not kept across it.
#ifdef JACO_EMULATED
JDEV const JacoTransitionArgs* transition_args(const JacoTransitionArgs& A) { return &A; }
#else
JDEV const JacoTransitionArgs* transition_args(const JacoTransitionArgs&) {
  typedef const JacoTransitionArgs __attribute__((address_space(4))) * KP;
  KP p = (KP)__builtin_amdgcn_kernarg_segment_ptr();
  asm volatile("" : "+s"(p));
  return (const JacoTransitionArgs*)p;
}
#endif

// D into the kept pair: its low word into the flags word, or into its own register
#if JTRANSITION_CARRY_IN_FLAGS
JDEV void transition_keep(TransitionInc D, float& hi, unsigned& flags) { hi = D.hi; flags = __float_as_uint(D.lo); }
#define TRANSITION_KEEP_LO flags
#else
JDEV void transition_keep(TransitionInc D, float& hi, float& lo) { hi = D.hi; lo = D.lo; }
#define TRANSITION_KEEP_LO keep_lo
#endif

template <class L>
JDEV void run_transition(const JacoTransitionArgs& Q_, L& s, int w, int lane) {
  // loop state: the pair i, the column c (the nominal, where it runs, is the "column" in front of the group's first: c = g - groups < 0;
  // group 0's, c == -groups, is the one that reports), the side, and in `keep` D(+) across the minus side (centered) or D(0) across
  // the columns (forward)
  int i, c;
  {
    const JacoTransitionArgs* Q = transition_args(Q_);
    const int groups = Q->groups, nx = 2 * Q->ndofs, ncol = nx + Q->nacts;
    i = wave_uniform_i(w / groups);
    const int g = wave_uniform_i(w - i * groups);
    const bool report = g == 0 && (Q->next_qpos != nullptr || Q->next_qvel != nullptr || Q->status != nullptr);
    const int first_b = g >= nx ? g : g + (nx - g + groups - 1) / groups * groups;   // the group's first ctrl column, if below ncol
    const bool any_column = (Q->A != nullptr && g < nx) || (Q->B != nullptr && first_b < ncol);
    c = (report || (Q->centered == 0 && any_column)) ? g - groups : g;
    stage_model(opaque_ptr(Q->model), s, lane);
  }
  int side = 0;
  float keep_hi = 0.f;
  unsigned flags = 0u;   // (JTRANSITION_CARRY_IN_FLAGS: between evaluations the kept low word's bits; during one, those and the status bits)
#if !JTRANSITION_CARRY_IN_FLAGS
  float keep_lo = 0.f;
#endif
#pragma nounroll
  while (true) {
    {
      const JacoTransitionArgs* Q = transition_args(Q_);
      const int nx = 2 * Q->ndofs;
      if (c >= nx + Q->nacts) break;
      if (c >= 0 && (c < nx ? Q->A == nullptr : Q->B == nullptr)) { c += Q->groups; continue; }
      const JacoModelDev* m = opaque_ptr(Q->model);
      transition_restore(Q, m, s, i, lane);
      if (c >= 0) {   // the one perturbed word: x0 + eps or x0 - eps in fp32, written by one lane
        const int nd = Q->ndofs;
        float* word = c < nd ? &s.qpos[m->d_qadr[Q->dofs[c]]] : (c < nx ? &s.qvel[Q->dofs[c - nd]] : &s.ctrl[Q->acts[c - nx]]);
        const TransitionStep t = transition_step(Q, m, i, c);
        if (lane == 0) *word = side ? t.xm : t.xp;
        wave_sync();
      }
    }
#if JTRANSITION_CARRY_IN_FLAGS
    const unsigned long long carry0 = wave_ballot((flags & TRANSITION_STATUS0) != 0u), carry1 = wave_ballot((flags & TRANSITION_STATUS1) != 0u);
    flags = c < 0 ? 0u : flags & ~TRANSITION_STATUS;
#else
    flags = 0u;
#endif
    {
      const int hold = transition_args(Q_)->hold;
#pragma nounroll
      for (int sub = 0; sub < hold; sub++) {
        // (as run_rollout's substep loop: the block re-read, the pointer's provenance and the lane id hidden, or the substep's model loads
        // and lane-derived addresses are hoisted out of the column loop and kept alive, spilled, across all of it)
        const JacoModelDev* m = opaque_ptr(transition_args(Q_)->model);
        lane = wave_opaque_i(lane);
        entry_walk(m, s, lane);
        rollout_substep(m, s, lane, flags);
      }
    }
    const JacoTransitionArgs* Q = transition_args(Q_);
    const JacoModelDev* m = opaque_ptr(Q->model);
    const int nd = Q->ndofs, nx = 2 * nd;
    const bool nom = c < 0, centered = Q->centered != 0;
    // (the steps and the start words are formed again from the pair's row, the same fp32 operations on the same words)
    TransitionStep t{0.f, 0.f, 0.f};
    if (!nom) t = transition_step(Q, m, i, c);
#if JTRANSITION_CARRY_IN_FLAGS
    const TransitionInc keep{keep_hi, __uint_as_float((flags & ~TRANSITION_STATUS) | (((carry0 >> lane) & 1ull) ? TRANSITION_STATUS0 : 0u) |
                                                      (((carry1 >> lane) & 1ull) ? TRANSITION_STATUS1 : 0u))};
    const unsigned reported = flags;       // (the nominal's: its word started from zero)
    flags = __float_as_uint(keep.lo);      // the carried word again as it was: forward differences keep D(0) over all the columns
#else
    const TransitionInc keep{keep_hi, keep_lo};
    const unsigned reported = flags;
#endif
    TransitionInc D{0.f, 0.f};
    if (lane < nx) {
      const int dof = Q->dofs[lane < nd ? lane : lane - nd];
      const int at = lane < nd ? m->d_qadr[dof] : dof;
      float xs = lane < nd ? Q->qpos[(size_t)i * m->nq + at] : Q->qvel[(size_t)i * m->nv + at];
      if (lane == c) xs = side ? t.xm : t.xp;   // (lane < nx: a state column's own coordinate)
      const float hi = lane < nd ? s.qpos[at] : s.qvel[at], lo = lane < nd ? s.qpos_lo[at] : s.qvel_lo[at];
      D = transition_increment(hi, lo, xs);
    }
    if (nom) {
      if (c == -Q->groups) {
        const int nq = m->nq, nv = m->nv;
        if (Q->next_qpos && lane < nq) Q->next_qpos[(size_t)i * nq + lane] = s.qpos[lane];
        if (Q->next_qvel && lane < nv) Q->next_qvel[(size_t)i * nv + lane] = s.qvel[lane];
        if (Q->status) {   // the lanes' sticky flags, or-reduced over the wavefront, as run_rollout reports them
          const unsigned f = wave_or(reported);
          if (lane == 0) Q->status[i] = f;
        }
      }
      transition_keep(D, keep_hi, TRANSITION_KEEP_LO);
      c += Q->groups;
    } else if (centered && side == 0) {
      transition_keep(D, keep_hi, TRANSITION_KEEP_LO);
      side = 1;
    } else {
      const TransitionInc step = transition_increment(t.xp, 0.f, centered ? t.xm : t.x0);   // c(+) - c(-), or c(+) - c0
      const TransitionInc own = (c < nx && lane == c) ? step : TransitionInc{0.f, 0.f};
      const float quot = centered ? transition_entry(own, keep, D, 1.0f / step.hi) : transition_entry(own, D, keep, 1.0f / step.hi);
      if (lane < nx) {   // lane r stores entry [r][c]
        if (c < nx) Q->A[((size_t)i * nx + lane) * nx + c] = quot;
        else Q->B[((size_t)i * nx + lane) * Q->nacts + (c - nx)] = quot;
      }
      side = 0;
      c += Q->groups;
    }
    wave_sync();
  }
}

#if JACO_TU_HAS(20)
JACO_DEFINE_ENTRY(transition_fd, JacoTransitionArgs, Q.n * Q.groups, run_transition)
#else
JACO_DECLARE_ENTRY(transition_fd, JacoTransitionArgs)
#endif
