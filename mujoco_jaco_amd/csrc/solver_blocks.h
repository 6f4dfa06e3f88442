// Dense solver blocks on one wave, one matrix row per lane, registers only: the LDL^T solves of the mass matrix and the Newton Hessian
// (ldl_solve, ldl_block, ldl_block0_dual, ldl_solve_blocks) and the 6 x 6 Gauss-Jordan eliminations of the controllers (gj_inverse6, gj_solve6).
// Plain linear algebra: nothing here knows a model beyond the dof blocks [0, JB0) [JB0, JB1) [JB1, JNV) of jaco/model_dev.h.
//
// Every routine is a sequence of pivot steps, and every step is a preamble (pivot broadcast, reciprocal, multiplier) followed by
// "subtract multiplier x lane k's row from my row".  The preambles are written once.  The subtraction has two forms:
//   read-lane: lane k's elements come through v_readlane_b32 into SGPRs, then one fma each (ldl_update, ldl_back_step, gj_update: plain
//              functions called from unrolled loops, since the pivot is only a lane index);
//   DPP:       where the whole block lies in one 16-lane row, a DPP operand (row_newbcast:K = lane K of the lane's own row) reads the
//              element inside the multiply-add itself (wave_ops.h row_bcast_fnmac / row_bcast_fmac2): one VALU instruction instead of two.
//              Recursive templates over the pivot (*_row), because the lane a DPP operand reads is part of the instruction.
// Each routine chooses between the two once.  -DJACO_SOLVER_DPP=0 (A/B and bit-equality builds, tools/build_variant.sh solverbcast): the
// read-lane forms everywhere; both forms give the same bits (tests/test_gpu_solver_dpp.py).
#pragma once
#include <jaco/model_dev.h>
#include <jaco/wave_ops.h>
#ifndef JACO_SOLVER_DPP
#define JACO_SOLVER_DPP 1
#endif
#ifdef JACO_EMULATED   // (the host emulator has no DPP operands: its builds keep the read-lane forms, bit for bit what they were)
#undef JACO_SOLVER_DPP
#define JACO_SOLVER_DPP 0
#endif
// Kernels whose register budget the statements' operands would raise keep the read-lane forms too (profiles/solver_dpp.txt): in the 12-hinge
// layout the huge tier's worker kernel (one more AGPR) and the open-loop rollout kernel (one more VGPR).
#if defined(JACO_TU) && JNV == 18 && JB0 == 12 && (JACO_TU == 6 || JACO_TU == 15)
#undef JACO_SOLVER_DPP
#define JACO_SOLVER_DPP 0
#endif

// ---------------------------------------------------------------- LDL^T solve, one matrix row per lane
// h[j] = A[lane][j] (lanes >= n must hold identity rows), b = rhs[lane]; returns x[lane]. Registers only.
// FULL = false: A is block diagonal over the dof blocks [0,JB0) [JB0,JB1) [JB1,JNV) (always true for the mass
// matrix; true for the Newton Hessian unless an active row couples two blocks): 66 instead of 210 eliminations.
// The lane masks of the eliminations.  Forward pass: lane i is a row below pivot k when i > k (and i < HI: a singular pivot's inf stays out of
// the other blocks' rows); that one predicate per pivot also says who takes 1 / d_k as its own (every lane with k <= i does, pivot after
// pivot, so lane i ends with 1 / d_i) and, negated, who takes x in the back-substitution (every lane with i <= k does, k descending, so
// lane i ends with the value of step k = i).  The back-substitution's sum needs no mask at all: lane i reads `acc` once, at step k = i,
// before that step's add, and every add it has seen by then had i < k; what steps k <= i add afterwards (the row's own entries times x_k,
// possibly inf or NaN in lanes outside the block) is never read -- x is taken before, lanes outside [LO, HI) never keep x, and the
// return is masked.  The terms keep their rounding: the first is h x + 0 in one fma, the others a rounded product and an add, as the
// masked sum compiled.  -DJACO_SOLVER_MASKS=1 (A/B and bit-equality builds, tools/build_variant.sh solvermasks): one compare per role and
// the masked sum, as before (solver_blocks_masks.h).
#ifndef JACO_SOLVER_MASKS
#define JACO_SOLVER_MASKS 0
#endif
#define JLDL_NSH 6   // ldl_block0_dual: the pivots its two systems share
#if JACO_SOLVER_MASKS
#include "solver_blocks_masks.h"
#else
// acc + a * b with the product rounded on its own, whatever the build's contraction mode (fmul_rn alone does not stop the add from fusing)
JDEV float add_rounded_product(float acc, float a, float b) {
#pragma clang fp contract(off)
  return acc + a * b;
}
// this lane's row index if it is below HI, else -1 (no row of the block): `ldl_row > k` is "below pivot k, inside the block" in one compare
template <int HI>
JDEV int ldl_row(int lane) { return wave_opaque_i(lane < HI ? lane : -1); }

// Preamble of forward pivot k, the same whatever form the updates take: the pivot d_k in every lane (through v_readlane in both forms: the
// reciprocal wants it everywhere), who keeps 1 / d_k (`below` still is the pivot before's: row >= k), who lies below (row > k), and the
// multiplier of lane k's row (0 elsewhere).
JDEV float ldl_pivot(float hk, float& dinv, bool& below, int row, int k) {
  const float inv = 1.f / wave_bcast(hk, k);
  dinv = below ? inv : dinv;
  below = row > k;
  return below ? hk * inv : 0.f;
}
// ... of ldl_block0_dual's trailing pivots: two systems (h, g) under one `below`
JDEV void ldl_dual_pivot(float hk, float gk, float& dinv, float& dinvd, bool& below, int row, int k, float& lik, float& likd) {
  const float dk = wave_bcast(hk, k), dkd = wave_bcast(gk, k);
  const float inv = 1.f / dk, invd = 1.f / dkd;
  dinv = below ? inv : dinv;
  dinvd = below ? invd : dinvd;
  below = row > k;
  lik = below ? hk * inv : 0.f;
  likd = below ? gk * invd : 0.f;
}
// Preamble of back-substitution step k: who takes x (row <= k: lane i ends with the value of step k = i)
JDEV float ldl_take_x(float x, float z, float dinv, float acc, int row, int k) { return row > k ? x : z - dinv * acc; }

// The read-lane updates.  h[j] -= lik * (lane k's h[j]) for the columns k < j < ce, and b likewise.  All of the pivot row's broadcasts first,
// then the updates: a v_readlane straight in front of the VALU that reads its SGPR costs two wait states on gfx950, and the compiler pairs
// them up when the source does.
JDEV void ldl_update(float (&h)[JNV], float& b, float lik, int k, int ce) {
  float pk[JNV];
#pragma unroll
  for (int j = k + 1; j < ce; j++) pk[j] = wave_bcast(h[j], k);
  const float bk = wave_bcast(b, k);
#pragma unroll
  for (int j = k + 1; j < ce; j++) h[j] -= lik * pk[j];
  b -= lik * bk;
}
template <int NG>
JDEV void ldl_dual_update(float (&h)[JNV], float (&g)[NG], float& b, float& bd, float lik, float likd, int k, int ce) {
  float pk[JNV], pg[JNV];
#pragma unroll
  for (int j = k + 1; j < ce; j++) { pk[j] = wave_bcast(h[j], k); pg[j] = wave_bcast(g[j - JLDL_NSH], k); }
  const float bk = wave_bcast(b, k), bdk = wave_bcast(bd, k);
#pragma unroll
  for (int j = k + 1; j < ce; j++) { h[j] -= lik * pk[j]; g[j - JLDL_NSH] -= likd * pg[j]; }
  b -= lik * bk;
  bd -= likd * bdk;
}
// step k of a back-substitution over the rows below hi: the first term is h x + 0 in one fma, the others a rounded product and an add
JDEV void ldl_back_step(const float (&h)[JNV], float z, float dinv, float& acc, float& x, int row, int k, int hi) {
  x = ldl_take_x(x, z, dinv, acc, row, k);
  const float xk = wave_bcast(x, k);
  acc = k == hi - 1 ? fmaf(h[k], xk, 0.f) : add_rounded_product(acc, h[k], xk);
}
#if JACO_SOLVER_DPP
// The DPP updates, for a block inside one 16-lane row (RM: that row's bit): pivots K .. PE - 1 of a forward elimination over the columns up to
// CE, steps K .. LO of a back-substitution.  Per pivot one statement holds all the multiply-adds, elements in ascending order as in the
// read-lane form; a statement's instructions cannot be dropped one by one as dead, so it names only the live columns (K < j < CE) and b.
// The same expressions in every lane of the block's row; the lanes of the other rows, which added -0 * p_k in the read-lane form, are left
// alone.  The back-substitution's x_k is the DPP operand of its rounded product (wave_ops.h row_bcast).
template <int K, int PE, int CE, int RM>
JDEV void ldl_fwd_row(float (&h)[JNV], float& b, float& dinv, bool& below, int row) {
  if constexpr (K < PE) {
    const float lik = ldl_pivot(h[K], dinv, below, row, K);
    row_bcast_fnmac_cols<K % 16, RM, K + 1>(h, b, lik, std::make_integer_sequence<int, CE - 1 - K>{});
    ldl_fwd_row<K + 1, PE, CE, RM>(h, b, dinv, below, row);
  }
}
template <int K, int LO, int HI>
JDEV void ldl_back_row(float (&h)[JNV], float z, float dinv, float& acc, float& x, int row) {
  if constexpr (K >= LO) {
    x = ldl_take_x(x, z, dinv, acc, row, K);
    acc = K == HI - 1 ? fmaf(h[K], row_bcast<K % 16>(x), 0.f) : add_rounded_product(acc, h[K], row_bcast<K % 16>(x));
    ldl_back_row<K - 1, LO, HI>(h, z, dinv, acc, x, row);
  }
}
// ... of ldl_block0_dual: its trailing pivots and its back-substitution, both systems
template <int K, int B0>
JDEV void ldl_dual_fwd_row(float (&h)[JNV], float (&g)[B0 - JLDL_NSH], float& b, float& bd, float& dinv, float& dinvd, bool& below, int row) {
  if constexpr (K < B0) {
    float lik, likd;
    ldl_dual_pivot(h[K], g[K - JLDL_NSH], dinv, dinvd, below, row, K, lik, likd);
    row_bcast_fnmac_cols<K, 1, K + 1>(h, b, lik, std::make_integer_sequence<int, B0 - 1 - K>{});
    row_bcast_fnmac_cols<K, 1, K + 1 - JLDL_NSH>(g, bd, likd, std::make_integer_sequence<int, B0 - 1 - K>{});
    ldl_dual_fwd_row<K + 1, B0>(h, g, b, bd, dinv, dinvd, below, row);
  }
}
template <int K, int B0>
JDEV void ldl_dual_back_row(float (&h)[JNV], float (&g)[B0 - JLDL_NSH], float z, float zd, float dinv, float dinvd, float& acc, float& accd, float& x, float& xd, int row, int lane) {
  if constexpr (K >= 0) {
    x = ldl_take_x(x, z, dinv, acc, row, K);
    xd = ldl_take_x(xd, zd, dinvd, accd, row, K);
    const float hk = h[K];
    float multd = hk;   // (the damped system's multiplier: see the read-lane step in ldl_block0_dual)
    if constexpr (K >= JLDL_NSH) { const float gk = g[K - JLDL_NSH]; multd = lane >= JLDL_NSH ? gk : hk; }
    multd = lane < K ? multd : 0.f;
    row_bcast_fmac2<K, 1>(acc, x, hk, accd, xd, multd);
    ldl_dual_back_row<K - 1, B0>(h, g, z, zd, dinv, dinvd, acc, accd, x, xd, row, lane);
  }
}
#endif

template <bool FULL>
JDEV float ldl_solve(float (&h)[JNV], float b, int lane) {
  float dinv = 1.f;
  bool below = true;   // of the pivot before: lane >= k
#pragma unroll
  for (int k = 0; k < JNV; k++) {
    const int jend = FULL ? JNV : (k < JB0 ? JB0 : (k < JB1 ? JB1 : JNV));
    ldl_update(h, b, ldl_pivot(h[k], dinv, below, lane, k), k, jend);
  }
  // now: b = y (L y = rhs); h[k>lane] = d_lane * L[k][lane]
  float z = b * dinv, acc = 0.f, x = 0.f;   // (lanes >= JNV never take x: 0)
#pragma unroll
  for (int k = JNV - 1; k >= 0; k--) ldl_back_step(h, z, dinv, acc, x, lane, k, JNV);
  return x;
}
// One dof block [LO, HI) of a block-diagonal matrix; x = 0 in the lanes outside it.
template <int LO, int HI>
JDEV float ldl_block(float (&h)[JNV], float b, int lane) {
  const int row = ldl_row<HI>(lane);
  float dinv = 1.f;
  bool below = true;
#if JACO_SOLVER_DPP
  if constexpr (LO / 16 == (HI - 1) / 16) {   // inside one 16-lane row: [0, JB0) and [JB0, JB1) of the default layout
    ldl_fwd_row<LO, HI, HI, 1 << (LO / 16)>(h, b, dinv, below, row);
    float z = b * dinv, acc = 0.f, x = 0.f;
    ldl_back_row<HI - 1, LO, HI>(h, z, dinv, acc, x, row);
    return row >= LO ? x : 0.f;
  } else
#endif
  {
#pragma unroll
    for (int k = LO; k < HI; k++) ldl_update(h, b, ldl_pivot(h[k], dinv, below, row, k), k, HI);
    float z = b * dinv, acc = 0.f, x = 0.f;
#pragma unroll
    for (int k = HI - 1; k >= LO; k--) ldl_back_step(h, z, dinv, acc, x, row, k, HI);
    return row >= LO ? x : 0.f;
  }
}
// Arm/finger block [0, JB0) with implicit joint damping: x = M^-1 b and xd = (M + diag(hd))^-1 b from ONE elimination where
// the two matrices agree.  hd is non-zero only on the last JB0 - NSH dofs (the finger joints, leaves of the arm's tree), so
// the first NSH pivots, their multipliers and the forward-substituted right-hand side are identical; only the trailing
// (JB0 - NSH) x (JB0 - NSH) Schur complement differs (by hd on its diagonal).  Returns x, *xd_out = xd (0 outside the block).
template <int B0 = JB0>   // (a parameter so that the one-row form below is compiled only where the block fits a row)
JDEV float ldl_block0_dual(float (&h)[JNV], float b, float hd, int lane, float* xd_out) {
  const int row = ldl_row<JB0>(lane);
  float dinv = 1.f;
  bool below = true;
#if JACO_SOLVER_DPP
  if constexpr (B0 <= 16) {   // inside lanes 0..15.  (Both back-substitution sums are fused multiply-adds in either form, as they always compiled.)
    ldl_fwd_row<0, JLDL_NSH, B0, 1>(h, b, dinv, below, row);
    float g[B0 - JLDL_NSH], bd = b, dinvd = dinv;
#pragma unroll
    for (int j = JLDL_NSH; j < B0; j++) g[j - JLDL_NSH] = h[j] + (lane == j ? hd : 0.f);
    ldl_dual_fwd_row<JLDL_NSH, B0>(h, g, b, bd, dinv, dinvd, below, row);
    float z = b * dinv, zd = bd * dinvd, acc = 0.f, accd = 0.f, x = 0.f, xd = 0.f;
    ldl_dual_back_row<B0 - 1, B0>(h, g, z, zd, dinv, dinvd, acc, accd, x, xd, row, lane);
    *xd_out = row >= 0 ? xd : 0.f;
    return row >= 0 ? x : 0.f;
  }
#endif
#pragma unroll
  for (int k = 0; k < JLDL_NSH; k++) {
    // (ldl_update written out: called from here, the 12-hinge and 30-dof rollout kernels compile to reordered code -- same instructions, other
    // registers -- and the read-lane build of the default layout's to one s_nop more)
    const float lik = ldl_pivot(h[k], dinv, below, row, k);
    float pk[JNV];
#pragma unroll
    for (int j = k + 1; j < JB0; j++) pk[j] = wave_bcast(h[j], k);
    const float bk = wave_bcast(b, k);
#pragma unroll
    for (int j = k + 1; j < JB0; j++) h[j] -= lik * pk[j];
    b -= lik * bk;
  }
  // trailing block, twice: plain (h, b, dinv) and damped (g, bd, dinvd)
  float g[JB0 - JLDL_NSH], bd = b, dinvd = dinv;
#pragma unroll
  for (int j = JLDL_NSH; j < JB0; j++) g[j - JLDL_NSH] = h[j] + (lane == j ? hd : 0.f);
#pragma unroll
  for (int k = JLDL_NSH; k < JB0; k++) {
    float lik, likd;
    ldl_dual_pivot(h[k], g[k - JLDL_NSH], dinv, dinvd, below, row, k, lik, likd);
    ldl_dual_update(h, g, b, bd, lik, likd, k, JB0);
  }
  // back-substitution: h[k > lane] = d_lane * L[k][lane] (rows < NSH use h for both systems)
  float z = b * dinv, zd = bd * dinvd, acc = 0.f, accd = 0.f, x = 0.f, xd = 0.f;
#pragma unroll
  for (int k = JB0 - 1; k >= 0; k--) {
    x = ldl_take_x(x, z, dinv, acc, row, k);
    xd = ldl_take_x(xd, zd, dinvd, accd, row, k);
    float xk = wave_bcast(x, k), xdk = wave_bcast(xd, k);
    // multiplier of row k in column `lane`: the damped system's differs only inside the trailing block.  It is a select already and
    // keeps its lane mask: with both sums unmasked the rollout kernels of the 30-dof layout need 144 registers instead of 126
    // (tests/test_rollout_cost_budget.py holds them to 128), with either one masked they need what they did
    float multd = (lane < k) ? ((k >= JLDL_NSH && lane >= JLDL_NSH) ? g[k - JLDL_NSH] : h[k]) : 0.f;
    acc += h[k] * xk;
    accd += multd * xdk;
  }
  *xd_out = row >= 0 ? xd : 0.f;
  return row >= 0 ? x : 0.f;
}
#endif
// Block-diagonal solve that factors only the dof blocks named in `mask` (bit 0: [0,JB0), bit 1: [JB0,JB1), bit 2: [JB1,JNV));
// lanes of skipped blocks get x = 0.
JDEV float ldl_solve_blocks(float (&h)[JNV], float b, int lane, int mask) {
  float x = 0.f;
  if (mask & 1) x += ldl_block<0, JB0>(h, b, lane);
  if (mask & 2) x += ldl_block<JB0, JB1>(h, b, lane);
  if (mask & 4) x += ldl_block<JB1, JNV>(h, b, lane);
  return x;
}
JDEV void load_rows(float (&h)[JNV], const float* M, int nv, int lane) {
#pragma unroll
  for (int j = 0; j < JNV; j++) h[j] = lane < nv ? M[lane * JNV + j] : (lane == j ? 1.f : 0.f);
}

// ---------------------------------------------------------------- 6x6 Gauss-Jordan, one matrix row per lane (lanes 0..5)
// No pivoting (SPD input).  gj_inverse6: B in: identity row; out: inverse row.  gj_solve6: a single right-hand side.  One elimination for
// both: they differ only in the right-hand side, six columns or one.  (A is left in no defined state; no caller reads it afterwards.)
// Preamble of pivot k: the pivot in every lane, the determinant, lane k's row scaled to a unit pivot; returns the multiplier of that row.
JDEV void gj_scale(float (&A)[6], float (&B)[6], float sc) {
#pragma unroll
  for (int j = 0; j < 6; j++) { A[j] *= sc; B[j] *= sc; }
}
JDEV void gj_scale(float (&A)[6], float& b, float sc) {
#pragma unroll
  for (int j = 0; j < 6; j++) A[j] *= sc;
  b *= sc;
}
template <class RHS>   // float[6] or float
JDEV float gj_pivot(float (&A)[6], RHS& B, float& det, int lane, int k) {
  const float piv = wave_bcast(A[k], k);
  det *= piv;
  const float inv = 1.f / piv, sc = lane == k ? inv : 1.f;
  gj_scale(A, B, sc);
  return lane == k ? 0.f : A[k];
}
#if JACO_SOLVER_DPP
// The DPP update (rows 0..5 lie in the first 16-lane row; what lanes 16..63 hold is no row of the matrix and is read by nobody).  Only the live
// elements are named, as in ldl_fwd_row: the columns of A right of the pivot (a column is last read at its own pivot), all of B.
template <int K, int... I>
JDEV void gj_update_row(float (&A)[6], float (&B)[6], float f, std::integer_sequence<int, I...>) {
  row_bcast_fnmac<K, 1>(f, A[K + 1 + I]..., B[0], B[1], B[2], B[3], B[4], B[5]);
}
template <int K, int... I>
JDEV void gj_update_row(float (&A)[6], float& b, float f, std::integer_sequence<int, I...>) { row_bcast_fnmac<K, 1>(f, A[K + 1 + I]..., b); }
template <int K, class RHS>
JDEV void gj_eliminate_row(float (&A)[6], RHS& B, float& det, int lane) {
  if constexpr (K < 6) {
    const float f = gj_pivot(A, B, det, lane, K);
    gj_update_row<K>(A, B, f, std::make_integer_sequence<int, 5 - K>{});
    gj_eliminate_row<K + 1>(A, B, det, lane);
  }
}
#else
// The read-lane update (broadcasts first, then the updates: ldl_update)
JDEV void gj_update(float (&A)[6], float (&B)[6], float f, int k) {
  float pa[6], pb[6];
#pragma unroll
  for (int j = 0; j < 6; j++) { pa[j] = wave_bcast(A[j], k); pb[j] = wave_bcast(B[j], k); }
#pragma unroll
  for (int j = 0; j < 6; j++) { A[j] -= f * pa[j]; B[j] -= f * pb[j]; }
}
JDEV void gj_update(float (&A)[6], float& b, float f, int k) {
  float pa[6];
#pragma unroll
  for (int j = 0; j < 6; j++) pa[j] = wave_bcast(A[j], k);
  const float pbk = wave_bcast(b, k);
#pragma unroll
  for (int j = 0; j < 6; j++) A[j] -= f * pa[j];
  b -= f * pbk;
}
#endif
template <class RHS>
JDEV float gj_eliminate(float (&A)[6], RHS& B, int lane) {
  float det = 1.f;
#if JACO_SOLVER_DPP
  gj_eliminate_row<0>(A, B, det, lane);
#else
#pragma unroll
  for (int k = 0; k < 6; k++) gj_update(A, B, gj_pivot(A, B, det, lane, k), k);
#endif
  return det;
}
JDEV float gj_inverse6(float (&A)[6], float (&B)[6], int lane) { return gj_eliminate(A, B, lane); }
JDEV float gj_solve6(float (&A)[6], float& b, int lane) { return gj_eliminate(A, b, lane); }   // returns det, b becomes (A^-1 b)[lane]
