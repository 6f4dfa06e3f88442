// The quadratic expansion of jaco_rollout_cost's cost along trajectories (jaco_cost_quad, include/jaco_env.h): the lx, lxx, lu, Vx, Vxx
// that jaco_lqr reads, for R trajectories of T knots that are inputs -- jaco_rollout_fb's / jaco_rollout_cost's qpos, qvel and ctrl
// outputs as they are -- in one launch.  The cost is rollout_cost.h's, term for term, re-indexed to jaco_lqr's convention (l_t(x_t, u_t)
// for t < T, a terminal cost on x_T): the start state is not costed, so row 0 of lx / lxx is zero.
//
// One 64-lane wavefront per work item w = r * T + k on JacoLDS<JacoArm>: x = x_(k+1) (row k of qpos / qvel), u = row k of ctrl,
// g = goal_per_knot ? k : 0, (W, Wp) = (wx, wp) for k < T - 1 and (wxT, wpT) for the last knot.  With nd = ndofs, nx = 2 nd, na = nacts:
//   d_j  = x_j - xgoal[p][g][j]                    (not wrapped, as in the cost; 0 where no state weight is set at all)
//   e_c  = pos_c - pgoal[p][g][c]                  pos: the frame's ORIGIN, the point rollout_pose reports; JacoFrame.point is ignored
//   Jp[c][j]: the translational Jacobian of dof dofs[j] at pos, run_query's words: S.b + cross(S.a, pos), exactly 0 off the body's chain
//   gx_j = W_j * d_j                               with Wp == 0: one subtract, one multiply
//        = fmaf(Wp, (Jp[0][j] e_0 then fmaf over c = 1, 2), W_j * d_j)        for j < nd with Wp != 0
//   H_ji = fmaf(Wp, (Jp[0][j] Jp[0][i] then fmaf over c = 1, 2), j == i ? W_j : 0)   for j, i < nd with Wp != 0
//        = j == i ? W_j : 0.0f                     elsewhere: the position / velocity cross blocks and the off-diagonal velocity entries
// GAUSS-NEWTON: the pose term's second-order part e . d2pos/dq2 is dropped, as every iLQR does; H is positive semi-definite.
// H_ji and H_ij are the same fmaf chain on commuted products: lxx and Vxx are symmetric bit for bit.
//   lu_a = wu[a] * u[acts[a]]                      (luu = diag(wu) is constant and lux zero: neither is written)
//   l    = (1/2 sum_a wu[a] u_a^2 + 1/2 sum_j W_j d_j^2) + 1/2 Wp |e|^2      knot k's own summand of jaco_rollout_cost's J
// Outputs: row 0 of lx / lxx exact zeros (by item k = 0); row k + 1 gets gx, H of item k < T - 1; Vx / Vxx get those of item k = T - 1;
// lu, l, status at [r][k].  status: JFLAG_NAN where a word of the item's qpos / qvel / ctrl rows, a goal word it reads or a result is not
// finite; JROLLOUT_BAD_INDEX for a goal_idx entry out of range, and then nothing else is written.
// Mapping: with Wp == 0 (wave-uniform per item) neither the model tables nor the tree walk run and x comes from global memory alone.
// Otherwise entry_state / entry_walk of entry_common.h, every lane composes the frame's pose (frame_pose), lane j < nd forms column j
// of Jp into the row area s.J, which is free after the walk ([3][JROLLOUT_FB_MAX_DOFS], then H [nd][nd] behind it: lane j forms row j).
// The nx x nx block is stored by one flat lane-strided loop (consecutive lanes, consecutive words: zeros and coalescing for free).
// No output depends on which others are asked for.  No LDS beyond the query kernel's, no scratch memory.
// Listed at the tail of physics_kernel.h; the kernel is translation unit 21 (kernels.hip -DJACO_TU=21).
#pragma once
#include <cmath>
#include <string>

#define JCQ_NX (2 * JROLLOUT_FB_MAX_DOFS)
#define JCQ_H_OFF (3 * JROLLOUT_FB_MAX_DOFS)   // floats of s.J in front of the H block: Jp
static_assert(JCQ_H_OFF + JROLLOUT_FB_MAX_DOFS * JROLLOUT_FB_MAX_DOFS <= JSCRATCH, "Jp and the nd x nd block fit the row area's early scratch");

struct JacoCostQuadOpts {   // = JacoCostQuadOptions of include/jaco_env.h (static_assert in abi_agreement.h)
  int nknots, goal_per_knot;
  int ndofs;
  int dofs[JROLLOUT_FB_MAX_DOFS];
  int nacts;
  int acts[JROLLOUT_FB_MAX_DOFS];
  float wx[JCQ_NX], wxT[JCQ_NX], wu[JROLLOUT_FB_MAX_DOFS], wp, wpT;
  int reserved;
};
struct JacoCostQuadGoals {   // = JacoCostQuadGoal of include/jaco_env.h
  const float* xgoal;      // [ngoals][G][nx] or nullptr; G = goal_per_knot ? nknots : 1
  const float* pgoal;      // [ngoals][G][3] or nullptr
  const int* goal_idx;     // [R] or nullptr: trajectory r takes goal r
  int ngoals;
};
struct JacoCostQuadOutp {   // = JacoCostQuadOut of include/jaco_env.h
  float* lx;
  float* lxx;
  float* lu;
  float* Vx;
  float* Vxx;
  float* l;
  unsigned* status;
};
struct JacoCostQuadArgs {
  const JacoModelDev* model;
  const float* qpos;          // [R][T][nq] or nullptr (no state and no pose weight)
  const float* qvel;          // [R][T][nv] or nullptr
  const float* ctrl;          // [R][T][nu] or nullptr: zeros
  JacoCostQuadGoals goal;     // (xgoal nullptr: no state weight is set; pgoal nullptr: no pose weight)
  JacoCostQuadOutp out;
  int R, T, goal_per_knot, ndofs, nacts;
  float wp, wpT;
  int dofs[JROLLOUT_FB_MAX_DOFS], acts[JROLLOUT_FB_MAX_DOFS];
  float wx[JCQ_NX], wxT[JCQ_NX], wu[JROLLOUT_FB_MAX_DOFS];
  JacoQueryFrame fr;
};

// The host half shared by jaco_cost_quad (jaco_env.hip) and the emulator's entry: every refusal, then the options into the argument
// block, whose state, ctrl and output pointers the caller has filled in as they were handed over (have_out: the output record was not
// NULL).  Returns an empty string, or what is wrong.
static inline std::string jaco_cost_quad_resolve(const JacoModelDev& m, const JacoCostQuadOpts* o, const JacoQueryFrame* frame, int R, const JacoCostQuadGoals* goal,
                                                 bool have_out, JacoCostQuadArgs* Q) {
  if (!o) return "the options are required";
  if (!have_out) return "the output record is required";
  if (!Q->out.lx && !Q->out.lxx && !Q->out.lu && !Q->out.Vx && !Q->out.Vxx && !Q->out.l && !Q->out.status)
    return "at least one of the outputs lx, lxx, lu, Vx, Vxx, l and status is required";
  if (R < 0) return "R " + std::to_string(R) + " is negative";
  if (o->nknots < 1) return "nknots " + std::to_string(o->nknots) + " is below 1";
  if (o->goal_per_knot != 0 && o->goal_per_knot != 1) return "goal_per_knot must be 0 or 1";
  if ((long long)R * o->nknots > 0x7fffffffLL) return "R " + std::to_string(R) + " x nknots " + std::to_string(o->nknots) + " is beyond the largest grid";
  {
    JacoRolloutFbArgs F{};   // (the dof list is jaco_rollout_fb's: its check, its messages)
    const std::string why = jaco_rollout_fb_dofs(m, o->ndofs, o->dofs, &F);
    if (!why.empty()) return why;
    for (int j = 0; j < F.ndofs; j++) Q->dofs[j] = F.dofs[j];
    Q->ndofs = F.ndofs;
  }
  // (the ctrl words are jaco_transition_fd's: its checks, its messages)
  if (o->nacts < 0 || o->nacts > JROLLOUT_FB_MAX_DOFS) return "nacts " + std::to_string(o->nacts) + " outside [0, " + std::to_string(JROLLOUT_FB_MAX_DOFS) + "]";
  for (int j = 0; j < o->nacts; j++) {
    const int a = o->acts[j];
    if (a < 0 || a >= m.nu) return "ctrl word " + std::to_string(a) + " outside [0, " + std::to_string(m.nu) + ")";
    for (int k = 0; k < j; k++) if (o->acts[k] == a) return "ctrl word " + std::to_string(a) + " is listed twice";
    Q->acts[j] = a;
  }
  Q->nacts = o->nacts;
  if ((Q->qpos != nullptr) != (Q->qvel != nullptr)) return "qpos and qvel are given together or not at all";
  bool state = false;   // (a state weight of the words the kernel reads, j < 2 ndofs; the words behind them are checked and not used)
  const auto bad = [](float w) { return !(w >= 0.f) || !std::isfinite(w); };
  for (int j = 0; j < JCQ_NX; j++) {
    if (bad(o->wx[j])) return "weight wx[" + std::to_string(j) + "] is negative or not finite";
    if (bad(o->wxT[j])) return "weight wxT[" + std::to_string(j) + "] is negative or not finite";
    state = state || (j < 2 * Q->ndofs && (o->wx[j] != 0.f || o->wxT[j] != 0.f));
  }
  for (int a = 0; a < JROLLOUT_FB_MAX_DOFS; a++)
    if (bad(o->wu[a])) return "weight wu[" + std::to_string(a) + "] is negative or not finite";
  if (bad(o->wp)) return "weight wp is negative or not finite";
  if (bad(o->wpT)) return "weight wpT is negative or not finite";
  const bool pose = o->wp != 0.f || o->wpT != 0.f;
  if (state && !(goal && goal->xgoal)) return "a non-zero state weight needs xgoal";
  if (pose && !(goal && goal->pgoal)) return "a non-zero pose weight needs pgoal";
  if (pose && !frame) return "a non-zero pose weight needs a frame";
  if (pose && (frame->body < 0 || frame->body >= m.nbody))
    return frame->body == -1 ? std::string("a non-zero pose weight needs a frame on a body: a world-fixed frame has no Jacobian")
                             : "frame body " + std::to_string(frame->body) + " outside [0, " + std::to_string(m.nbody) + ")";
  if (Q->out.lu && o->nacts < 1) return "lu needs at least one ctrl word";
  if ((state || pose) && !Q->qpos) return "a non-zero state or pose weight needs qpos and qvel";
  Q->goal = JacoCostQuadGoals{};
  if (state || pose) {   // (without either no goal is read, and the goal record is ignored)
    if (goal->ngoals < 1) return "ngoals " + std::to_string(goal->ngoals) + ": at least one goal is required";
    if (!goal->goal_idx && R > goal->ngoals) return "R " + std::to_string(R) + " trajectories from " + std::to_string(goal->ngoals) + " goals without a goal index";
    Q->goal = *goal;
    if (!state) Q->goal.xgoal = nullptr;
    if (!pose) Q->goal.pgoal = nullptr;
  }
  if (pose) Q->fr = *frame;
  Q->R = R; Q->T = o->nknots; Q->goal_per_knot = o->goal_per_knot;
  Q->wp = o->wp; Q->wpT = o->wpT;
  for (int j = 0; j < JCQ_NX; j++) { Q->wx[j] = o->wx[j]; Q->wxT[j] = o->wxT[j]; }
  for (int a = 0; a < JROLLOUT_FB_MAX_DOFS; a++) Q->wu[a] = o->wu[a];
  return std::string();
}

JDEV bool cost_quad_bad(float v) { return !(fabsf(v) <= 3.402823466e38f); }   // NaN or infinite

template <class L>
JDEV void run_cost_quad(const JacoCostQuadArgs& Q_, L& s, int w, int lane) {
  // The dof, ctrl-word and weight tables are indexed per lane: read through the kernarg segment pointer, as run_query reads its frames.
  const JacoCostQuadArgs& Q = *kernarg_view(Q_);
  const int T = Q.T, nd = Q.ndofs, nx = 2 * nd, na = Q.nacts;
  const int r = wave_uniform_i(w / T), k = wave_uniform_i(w - r * T);
  const bool last = k == T - 1;
  const bool goals = Q.goal.xgoal != nullptr || Q.goal.pgoal != nullptr;
  int p = r;
  if (goals && Q.goal.goal_idx) p = wave_uniform_i(Q.goal.goal_idx[r]);
  if (goals && (p < 0 || p >= Q.goal.ngoals)) {
    if (lane == 0 && Q.out.status) Q.out.status[w] = JROLLOUT_BAD_INDEX;
    return;
  }
  const size_t grow = Q.goal_per_knot ? (size_t)p * T + k : (size_t)p;
  const float Wp = last ? Q.wpT : Q.wp;
  const bool posed = Wp != 0.f;   // (wave-uniform; the host half has seen to the frame, pgoal and the state rows)
  bool bad = false;

  const JacoModelDev* m = opaque_ptr(Q.model);
  const int nq = m->nq, nv = m->nv, nu = m->nu;
  // the item's input rows, every word looked at once
  if (Q.qpos && lane < nq) bad = bad || cost_quad_bad(Q.qpos[(size_t)w * nq + lane]);   // (each row guarded by its own pointer)
  if (Q.qvel && lane < nv) bad = bad || cost_quad_bad(Q.qvel[(size_t)w * nv + lane]);
  if (Q.ctrl && lane < nu) bad = bad || cost_quad_bad(Q.ctrl[(size_t)w * nu + lane]);

  // the state part on lanes j < nx, from the rows' own words
  float Wj = 0.f, d = 0.f, gx = 0.f;
  if (lane < nx) {
    Wj = last ? Q.wxT[lane] : Q.wx[lane];
    if (Q.goal.xgoal) {
      const int dof = Q.dofs[lane < nd ? lane : lane - nd];
      const float x = lane < nd ? Q.qpos[(size_t)w * nq + m->d_qadr[dof]] : Q.qvel[(size_t)w * nv + dof];
      const float g = Q.goal.xgoal[grow * nx + lane];
      bad = bad || cost_quad_bad(g);
      d = x - g;
      gx = Wj * d;
    }
  }
  float acc = 0.f;   // the lane's share of l: lanes j < nx the state words, JRC_LANE_U + a the ctrl words, JRC_LANE_P + c the pose
  if (lane < nx) acc = (0.5f * Wj) * (d * d);
  {
    const int a = lane - JRC_LANE_U;
    if (a >= 0 && a < na) {
      const float u = Q.ctrl ? Q.ctrl[(size_t)w * nu + Q.acts[a]] : 0.f;
      acc = (0.5f * Q.wu[a]) * (u * u);
    }
  }
  if (Q.out.lu && lane < na) {
    const float u = Q.ctrl ? Q.ctrl[(size_t)w * nu + Q.acts[lane]] : 0.f;
    Q.out.lu[(size_t)w * na + lane] = Q.wu[lane] * u;
  }

  float* Jp = s.J;               // [3][JROLLOUT_FB_MAX_DOFS]
  float* Hb = s.J + JCQ_H_OFF;   // [nd][nd]
  if (posed) {
    entry_state(m, s, Q.qpos, Q.qvel, nullptr, w, lane);
    entry_walk(m, s, lane);
    v3 pos;
    m3 Rf;
    frame_pose(s, Q.fr, &pos, &Rf);
    const float* pg = Q.goal.pgoal + grow * 3;
    const v3 e = v3{pos.x - pg[0], pos.y - pg[1], pos.z - pg[2]};
    bad = bad || cost_quad_bad(pg[0]) || cost_quad_bad(pg[1]) || cost_quad_bad(pg[2]);
    const int c = lane - JRC_LANE_P;
    if (c >= 0 && c < 3) {
      const float ec = c == 0 ? e.x : (c == 1 ? e.y : e.z);
      acc = (0.5f * Wp) * (ec * ec);
    }
    if (lane < nd) {   // column j of Jp: run_query's words on the frame's origin
      const int dof = Q.dofs[lane], b = Q.fr.body;
      const sv S = ldsv(s.cdof[dof]);
      const bool on = ((m->b_chainmask[b] >> dof) & 1u) != 0u;
      const v3 jp = S.b + cross(S.a, pos);
      const float j0 = on ? jp.x : 0.f, j1 = on ? jp.y : 0.f, j2 = on ? jp.z : 0.f;
      Jp[0 * JROLLOUT_FB_MAX_DOFS + lane] = j0; Jp[1 * JROLLOUT_FB_MAX_DOFS + lane] = j1; Jp[2 * JROLLOUT_FB_MAX_DOFS + lane] = j2;
      gx = fmaf(Wp, fmaf(j2, e.z, fmaf(j1, e.y, j0 * e.x)), gx);
    }
    wave_sync();
    if (lane < nd) {   // row j of the nd x nd block
      const float j0 = Jp[0 * JROLLOUT_FB_MAX_DOFS + lane], j1 = Jp[1 * JROLLOUT_FB_MAX_DOFS + lane], j2 = Jp[2 * JROLLOUT_FB_MAX_DOFS + lane];
      for (int i = 0; i < nd; i++) {
        const float t = fmaf(j2, Jp[2 * JROLLOUT_FB_MAX_DOFS + i], fmaf(j1, Jp[1 * JROLLOUT_FB_MAX_DOFS + i], j0 * Jp[0 * JROLLOUT_FB_MAX_DOFS + i]));
        const float h = fmaf(Wp, t, i == lane ? Wj : 0.f);
        bad = bad || cost_quad_bad(h);
        Hb[lane * nd + i] = h;
      }
    }
    wave_sync();
  }
  bad = bad || cost_quad_bad(gx);

  // l: the three terms reduced as rollout_cost_finish reduces them
  const float tx = wave_sum(lane < JRC_LANE_U ? acc : 0.f);
  const float tu = wave_sum(lane >= JRC_LANE_U && lane < JRC_LANE_P ? acc : 0.f);
  const float tp = wave_sum(lane >= JRC_LANE_P ? acc : 0.f);
  const float l = (tu + tx) + tp;
  bad = bad || cost_quad_bad(l);
  if (Q.out.l && lane == 0) Q.out.l[w] = l;

  // the gradient and the block: row k + 1 of lx / lxx, or Vx / Vxx for the last knot; item 0 also writes the zero row 0
  float* gdst = last ? (Q.out.Vx ? Q.out.Vx + (size_t)r * nx : nullptr) : (Q.out.lx ? Q.out.lx + ((size_t)w + 1) * nx : nullptr);
  float* hdst = last ? (Q.out.Vxx ? Q.out.Vxx + (size_t)r * nx * nx : nullptr) : (Q.out.lxx ? Q.out.lxx + ((size_t)w + 1) * nx * nx : nullptr);
  if (gdst && lane < nx) gdst[lane] = gx;
  if (k == 0 && Q.out.lx && lane < nx) Q.out.lx[(size_t)w * nx + lane] = 0.f;
  if (hdst) {
    int row = 0, col = lane;
    for (int i = lane; i < nx * nx; i += 64) {
      while (col >= nx) { col -= nx; row++; }
      float h = row == col ? (last ? Q.wxT[row] : Q.wx[row]) : 0.f;
      if (posed && row < nd && col < nd) h = Hb[row * nd + col];
      hdst[i] = h;
      col += 64;
    }
  }
  if (k == 0 && Q.out.lxx) {
    float* z = Q.out.lxx + (size_t)w * nx * nx;
    for (int i = lane; i < nx * nx; i += 64) z[i] = 0.f;
  }
  if (Q.out.status) {
    const unsigned f = wave_or(bad ? (unsigned)JFLAG_NAN : 0u);
    if (lane == 0) Q.out.status[w] = f;
  }
}

#if JACO_TU_HAS(21)
JACO_DEFINE_ENTRY(cost_quad, JacoCostQuadArgs, Q.R * Q.T, run_cost_quad)
#else
JACO_DECLARE_ENTRY(cost_quad, JacoCostQuadArgs)
#endif
