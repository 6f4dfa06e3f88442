// The dense LDL^T blocks as they were before the lean forms of solver_blocks.h: one lane compare per role, the back-substitution sum under its
// lane mask.  Frozen: solver_blocks.h includes this file under -DJACO_SOLVER_MASKS=1 (tools/build_variant.sh solvermasks, tests/emu_solver), and
// the bit-equality tests (tests/test_gpu_solver_blocks.py, tests/test_solver_blocks_emu.py) hold the lean forms to it.  Not for editing.
#pragma once
template <bool FULL>
JDEV float ldl_solve(float (&h)[JNV], float b, int lane) {
  float dinv = 1.f;
#pragma unroll
  for (int k = 0; k < JNV; k++) {
    const int jend = FULL ? JNV : (k < JB0 ? JB0 : (k < JB1 ? JB1 : JNV));
    float dk = wave_bcast(h[k], k);
    float inv = 1.f / dk;
    dinv = lane == k ? inv : dinv;
    float lik = lane > k ? h[k] * inv : 0.f;
    // (all of the pivot row's broadcasts first, then the updates: a v_readlane straight in front of the VALU that reads its SGPR
    // costs two wait states on gfx950, and the compiler pairs them up when the source does)
    float pk[JNV];
#pragma unroll
    for (int j = k + 1; j < jend; j++) pk[j] = wave_bcast(h[j], k);
    const float bk = wave_bcast(b, k);
#pragma unroll
    for (int j = k + 1; j < jend; j++) h[j] -= lik * pk[j];
    b -= lik * bk;
  }
  // now: b = y (L y = rhs); h[k>lane] = d_lane * L[k][lane]
  float z = b * dinv, acc = 0.f, x = 0.f;
#pragma unroll
  for (int k = JNV - 1; k >= 0; k--) {
    x = lane == k ? z - dinv * acc : x;
    float xk = wave_bcast(x, k);
    acc += lane < k ? h[k] * xk : 0.f;
  }
  return x;
}
// Block-diagonal variant that factors only the dof blocks named in `mask` (bit 0: [0,JB0), bit 1: [JB0,JB1), bit 2: [JB1,JNV));
// lanes of skipped blocks get x = 0.
template <int LO, int HI>
JDEV float ldl_block(float (&h)[JNV], float b, int lane) {
  float dinv = 1.f;
#pragma unroll
  for (int k = LO; k < HI; k++) {
    float dk = wave_bcast(h[k], k);
    float inv = 1.f / dk;
    dinv = lane == k ? inv : dinv;
    float lik = (lane > k && lane < HI) ? h[k] * inv : 0.f;
    float pk[JNV];
#pragma unroll
    for (int j = k + 1; j < HI; j++) pk[j] = wave_bcast(h[j], k);
    const float bk = wave_bcast(b, k);
#pragma unroll
    for (int j = k + 1; j < HI; j++) h[j] -= lik * pk[j];
    b -= lik * bk;
  }
  float z = b * dinv, acc = 0.f, x = 0.f;
#pragma unroll
  for (int k = HI - 1; k >= LO; k--) {
    x = lane == k ? z - dinv * acc : x;
    float xk = wave_bcast(x, k);
    acc += (lane < k && lane >= LO) ? h[k] * xk : 0.f;
  }
  return (lane >= LO && lane < HI) ? x : 0.f;
}
// Arm/finger block [0, JB0) with implicit joint damping: x = M^-1 b and xd = (M + diag(hd))^-1 b from ONE elimination where
// the two matrices agree.  hd is non-zero only on the last JB0 - NSH dofs (the finger joints, leaves of the arm's tree), so
// the first NSH pivots, their multipliers and the forward-substituted right-hand side are identical; only the trailing
// (JB0 - NSH) x (JB0 - NSH) Schur complement differs (by hd on its diagonal).  Returns x, *xd_out = xd (0 outside the block).
JDEV float ldl_block0_dual(float (&h)[JNV], float b, float hd, int lane, float* xd_out) {
  float dinv = 1.f;
#pragma unroll
  for (int k = 0; k < JLDL_NSH; k++) {
    float dk = wave_bcast(h[k], k);
    float inv = 1.f / dk;
    dinv = lane == k ? inv : dinv;
    float lik = (lane > k && lane < JB0) ? h[k] * inv : 0.f;
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
    float dk = wave_bcast(h[k], k), dkd = wave_bcast(g[k - JLDL_NSH], k);
    float inv = 1.f / dk, invd = 1.f / dkd;
    dinv = lane == k ? inv : dinv;
    dinvd = lane == k ? invd : dinvd;
    const bool below = lane > k && lane < JB0;
    float lik = below ? h[k] * inv : 0.f, likd = below ? g[k - JLDL_NSH] * invd : 0.f;
    float pk[JNV], pg[JNV];
#pragma unroll
    for (int j = k + 1; j < JB0; j++) { pk[j] = wave_bcast(h[j], k); pg[j] = wave_bcast(g[j - JLDL_NSH], k); }
    const float bk = wave_bcast(b, k), bdk = wave_bcast(bd, k);
#pragma unroll
    for (int j = k + 1; j < JB0; j++) { h[j] -= lik * pk[j]; g[j - JLDL_NSH] -= likd * pg[j]; }
    b -= lik * bk;
    bd -= likd * bdk;
  }
  // back-substitution: h[k > lane] = d_lane * L[k][lane] (shared for k < NSH columns... rows < NSH use h for both systems)
  float z = b * dinv, zd = bd * dinvd, acc = 0.f, accd = 0.f, x = 0.f, xd = 0.f;
#pragma unroll
  for (int k = JB0 - 1; k >= 0; k--) {
    x = lane == k ? z - dinv * acc : x;
    xd = lane == k ? zd - dinvd * accd : xd;
    float xk = wave_bcast(x, k), xdk = wave_bcast(xd, k);
    // multiplier of row k in column `lane`: the damped system's differs only inside the trailing block
    float mult = lane < k ? h[k] : 0.f;
    float multd = (lane < k) ? ((k >= JLDL_NSH && lane >= JLDL_NSH) ? g[k - JLDL_NSH] : h[k]) : 0.f;
    acc += mult * xk;
    accd += multd * xdk;
  }
  *xd_out = lane < JB0 ? xd : 0.f;
  return lane < JB0 ? x : 0.f;
}
