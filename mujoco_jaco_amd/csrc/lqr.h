// The batched iLQR / TVLQR backward pass (jaco_lqr, include/jaco_env.h): the k_t and K_t that jaco_rollout_fb's law consumes, the
// expected cost change of a step and the cost-to-go at knot 0, from the linearisation and the cost expansion along a trajectory.
//
// Solve i works on problem p = prob_idx[i] (NULL: i) and runs t = T-1 .. 0 (nx states, nu controls, T knots):
//   Qx = lx + A'Vx          Qu = lu + B'Vx
//   Qxx = lxx + A'Vxx A     Qux = lux + B'Vxx A     Quu = luu + B'Vxx B
//   L L' = Quu + mu_i I                     (a pivot <= 0 or a non-finite number: status = JLQR_NOT_PD | t, the solve stops)
//   K = -(Quu + mu I)^-1 Qux               k = -(Quu + mu I)^-1 Qu
//   dV1 += k'Qu                            dV2 += 1/2 k'Quu k                      (Quu unregularised here and below)
//   Vx  = Qx  + K'(Quu k + Qu)  + Qux'k
//   Vxx = Qxx + K'(Quu K + Qux) + Qux'K;   Vxx = 1/2 (Vxx + Vxx')
// The fp32 order of operations is not part of the interface; that two runs of the same call agree bit for bit is (every sum below has a
// fixed order and no atomics).  A NULL lux / lx / lu / Vx is the array of zeros, bit for bit: the term is added as 0.0f.
//
// Mapping: one 64-lane wavefront per solve, blockIdx.x = i, the whole recursion in the one launch.  Vxx and Vx stay in LDS across the
// knots; per knot A, B and the cost rows come in from memory and K, k go out, nothing else.  Knot t-1's A and B are loaded into
// registers while knot t computes (21 + 11 words per lane at nx = 36, nu = 18) and stored to LDS when knot t-1 begins: otherwise every
// knot would expose a full memory latency, as rollout_fb.h's gain row would.  The cost arrays are read where they are added, each
// load issued before the product loop whose result it joins.
// Arithmetic: register-tiled VALU fmaf over LDS operands (lqr_gemm: 2 x 4 outputs per lane, one 16-byte LDS read and two 4-byte reads per
// 8 fmas; the inner loops unrolled JLQR_UNROLL = 4 times, chosen by measurement: DESIGN.md).  OPEN: wave_mfma_16x16x4 for the four
// nx x nx products has not been built or timed against this, so VALU is what exists, not a measured choice between the two.
// The solve: one wave-level Cholesky of Quu + mu I (lane r owns row r of the column in flight), then both triangular solves
// against the nx + 1 right-hand sides (Qux | Qu) together, lane c owning column c.
// LDS map (words; rows padded to multiples of 4 so that every 4-wide tile read is 16-byte aligned): Vxx, A, W 36 x 36 each; B, Y 36 x 20;
// Qa = (Qux | Qu) 18 x 40; Quu, L 18 x 20; vectors.  W = Vxx A is dead once Qxx and Qux are formed and holds G = Quu (K | k) + Qa from
// then on; B is dead by then too and holds (K | k).  27 440 B: five workgroups per CU.  No scratch memory.
// Failure: a solve that stops at knot t has written the rows of the knots > t and nothing else but its status word; a knot's rows go
// out only after that knot's K, k, Vxx and Vx were all found finite.  An index out of range writes JLQR_BAD_INDEX and nothing else.
// The header needs jaco/wave_ops.h and nothing of the model: the CPU tests build it on its own.  In the library it is the last of the entry
// headers listed at the tail of physics_kernel.h; the kernel is translation unit 17 (kernels.hip -DJACO_TU=17).
#pragma once
#include <cmath>
#include <string>
#include <jaco/wave_ops.h>
#ifndef JACO_TU_HAS
#define JACO_TU_HAS(n) 1
#endif

#define JLQR_MAX_NX 36           // = JACO_LQR_MAX_NX
#define JLQR_MAX_NU 18           // = JACO_LQR_MAX_NU
#define JLQR_MAX_KNOTS 16384     // = JACO_ROLLOUT_MAX_SUBSTEPS
#define JLQR_MAX_ROWS 64
#define JLQR_BAD_INDEX 0x80000u  // = JACO_LQR_BAD_INDEX
#define JLQR_NOT_PD 0x100000u    // = JACO_LQR_NOT_PD
enum { JLQR_LXX = 1, JLQR_LUU = 2, JLQR_LUX = 4, JLQR_LX = 8, JLQR_LU = 16, JLQR_VXX = 32, JLQR_VX = 64, JLQR_ALL = 127 };
struct JacoLqrOpts {   // = JacoLqrOptions of include/jaco_env.h (static_assert in abi_agreement.h)
  int nknots, nx, nu;
  int rows_out;
  int row[JLQR_MAX_NU];
  unsigned shared_knots, shared_probs;
};
struct JacoLqrProb {   // = JacoLqrProblem of include/jaco_env.h
  const float *A, *B;
  const float *lxx, *luu;
  const float *lux, *lx, *lu;
  const float *Vxx, *Vx;
  const float* mu;
  const int* prob_idx;
  int nprob;
};
struct JacoLqrOutp {   // = JacoLqrOut of include/jaco_env.h
  float *gain, *kff, *dV, *Vxx0, *Vx0;
  unsigned* status;
};
struct JacoLqrArgs {
  JacoLqrOpts o;       // row[] filled in for rows_out == 0 too (the identity)
  JacoLqrProb p;
  JacoLqrOutp out;
  int n, rows;         // rows = rows_out ? rows_out : nu
};

// The host half shared by jaco_lqr (jaco_env.hip) and the emulator's entry: every argument check, then the block.  Returns an empty
// string, or what is wrong.
static inline std::string jaco_lqr_resolve(const JacoLqrOpts* o, int n, const JacoLqrProb* p, const JacoLqrOutp* out, JacoLqrArgs* Q) {
  if (!o || !p || !out) return "the options, the problem and the outputs are required";
  if (o->nknots < 1 || o->nknots > JLQR_MAX_KNOTS) return "nknots " + std::to_string(o->nknots) + " outside [1, " + std::to_string(JLQR_MAX_KNOTS) + "]";
  if (o->nx < 1 || o->nx > JLQR_MAX_NX) return "nx " + std::to_string(o->nx) + " outside [1, " + std::to_string(JLQR_MAX_NX) + "]";
  if (o->nu < 1 || o->nu > JLQR_MAX_NU) return "nu " + std::to_string(o->nu) + " outside [1, " + std::to_string(JLQR_MAX_NU) + "]";
  if (n < 0) return "n " + std::to_string(n) + " is negative";
  if (p->nprob < 1) return "nprob " + std::to_string(p->nprob) + ": at least one problem is required";
  if (!p->prob_idx && n > p->nprob) return "n " + std::to_string(n) + " solves of " + std::to_string(p->nprob) + " problems without a problem index";
  if (!p->A || !p->B || !p->lxx || !p->luu || !p->Vxx) return "A, B, lxx, luu and the terminal Vxx are required";
  if (!out->gain && !out->kff && !out->dV && !out->Vxx0 && !out->Vx0) return "at least one of the outputs gain, kff, dV, Vxx0 and Vx0 is required";
  if ((o->shared_knots | o->shared_probs) & ~(unsigned)JLQR_ALL) return "a shared-axis mask has a bit outside the seven named";
  *Q = JacoLqrArgs{};
  Q->o = *o;
  Q->rows = o->nu;
  if (o->rows_out != 0) {
    if (o->rows_out < o->nu || o->rows_out > JLQR_MAX_ROWS)
      return "rows_out " + std::to_string(o->rows_out) + " outside [nu = " + std::to_string(o->nu) + ", " + std::to_string(JLQR_MAX_ROWS) + "]";
    for (int a = 0; a < o->nu; a++) {
      if (o->row[a] < 0 || o->row[a] >= o->rows_out) return "row " + std::to_string(o->row[a]) + " outside [0, " + std::to_string(o->rows_out) + ")";
      for (int b = 0; b < a; b++) if (o->row[b] == o->row[a]) return "row " + std::to_string(o->row[a]) + " is listed twice";
    }
    Q->rows = o->rows_out;
  } else {
    for (int a = 0; a < o->nu; a++) Q->o.row[a] = a;
  }
  for (int a = o->nu; a < JLQR_MAX_NU; a++) Q->o.row[a] = 0;
  Q->p = *p;
  Q->out = *out;
  Q->n = n;
  return std::string();
}

// (kernarg_view of physics_kernel.h, which this header must do without: the block is read through the kernel-argument segment, so
// that a per-lane index into row[] is a load, not a private copy of the block)
#ifdef JACO_EMULATED
JDEV const JacoLqrArgs* lqr_args_view(const JacoLqrArgs& Q) { return &Q; }
#else
JDEV const JacoLqrArgs* lqr_args_view(const JacoLqrArgs&) {
  typedef const JacoLqrArgs __attribute__((address_space(4))) * KP;
  KP p = (KP)__builtin_amdgcn_kernarg_segment_ptr();
  return (const JacoLqrArgs*)p;
}
#endif

#define JLQR_LDX 36   // padded row lengths at the maxima: nx, nu, nx + 1 rounded up to multiples of 4
#define JLQR_LDU 20
#define JLQR_LDA 40
struct JacoLqrLDS {
  alignas(16) float Vxx[JLQR_MAX_NX * JLQR_LDX];
  alignas(16) float A[JLQR_MAX_NX * JLQR_LDX];
  alignas(16) float W[JLQR_MAX_NX * JLQR_LDX];    // Vxx A; then G = Quu (K | k) + (Qux | Qu), rows of lda
  alignas(16) float B[JLQR_MAX_NX * JLQR_LDU];    // B; then (K | k), rows of lda (18 x 40 = 36 x 20 words)
  alignas(16) float Y[JLQR_MAX_NX * JLQR_LDU];    // Vxx B
  alignas(16) float Qa[JLQR_MAX_NU * JLQR_LDA];   // (Qux | Qu)
  alignas(16) float Quu[JLQR_MAX_NU * JLQR_LDU];
  alignas(16) float L[JLQR_MAX_NU * JLQR_LDU];    // the Cholesky factor of Quu + mu I, lower triangle
  float Vx[JLQR_MAX_NX], Qx[JLQR_MAX_NX], dinv[JLQR_LDU];
};
static_assert(JLQR_MAX_NU * JLQR_LDA == JLQR_MAX_NX * JLQR_LDU && JLQR_MAX_NU * JLQR_LDA <= JLQR_MAX_NX * JLQR_LDX, "the overlays of (K | k) on B and of G on W");
static_assert(sizeof(JacoLqrLDS) <= 32000, "five workgroups per CU: 25 LDS granules of 1 280 bytes");

typedef float jlqr_f4 __attribute__((vector_size(16)));
// Every inner loop below is a chain of fmas on LDS operands with a run-time trip count.  At five workgroups per CU a SIMD holds one or
// two waves, so nothing hides an LDS round trip but the loop's own loads: the loops are unrolled this far (the order of the sums does
// not change), so that this many iterations' operands are in flight at once.
#ifndef JLQR_UNROLL
#define JLQR_UNROLL 4
#endif

// C(i, j) = sum_k X(i, k) Y(k, j) for i < n, j < m, handed to done(i, j, value) by the lane that formed it.  X(i, k) is X[i xi + k xk]
// (either a matrix or its transpose), Y(k, j) is Y[k ldy + j] with ldy a multiple of 4 and at least m rounded up to one: a lane forms a
// 2 x 4 tile, its columns past m from the padding (formed, never handed over).  k ascends: one fixed order of summation.  add: a compact
// [n][ldadd] array in global memory whose entry is added to the sum (nullptr: 0.0f is), loaded BEFORE the k loop so that its memory
// latency passes under the loop -- loaded where it is used, each of a knot's five passes with a cost array exposed one round trip.
template <class Done>
JDEV void lqr_gemm(const float* X, int xi, int xk, const float* Y, int ldy, int n, int m, int kk, int lane, const float* add, int ldadd, Done done) {
  const int tj = (m + 3) >> 2, nt = ((n + 1) >> 1) * tj;
#pragma nounroll
  for (int t0 = 0; t0 < nt; t0 += JACO_WAVE) {
    const bool on = t0 + lane < nt;
    const int t = on ? t0 + lane : 0;
    const int bi = t / tj, i0 = 2 * bi, j0 = 4 * (t - bi * tj);
    const int i1 = i0 + 1 < n ? i0 + 1 : i0;
    const float *x0 = X + i0 * xi, *x1 = X + i1 * xi, *y = Y + j0;
    float c0[4] = {0.f, 0.f, 0.f, 0.f}, c1[4] = {0.f, 0.f, 0.f, 0.f}, z0[4] = {0.f, 0.f, 0.f, 0.f}, z1[4] = {0.f, 0.f, 0.f, 0.f};
    if (add && on) {
#pragma unroll
      for (int c = 0; c < 4; c++)
        if (j0 + c < m) {
          z0[c] = add[i0 * ldadd + j0 + c];
          if (i0 + 1 < n) z1[c] = add[(i0 + 1) * ldadd + j0 + c];
        }
    }
#pragma unroll JLQR_UNROLL
    for (int k = 0; k < kk; k++) {
      const float a0 = x0[k * xk], a1 = x1[k * xk];
      const jlqr_f4 b = *(const jlqr_f4*)(y + k * ldy);
#pragma unroll
      for (int c = 0; c < 4; c++) { c0[c] = fmaf(a0, b[c], c0[c]); c1[c] = fmaf(a1, b[c], c1[c]); }
    }
    if (on) {
#pragma unroll
      for (int c = 0; c < 4; c++)
        if (j0 + c < m) {
          done(i0, j0 + c, c0[c] + z0[c]);
          if (i0 + 1 < n) done(i0 + 1, j0 + c, c1[c] + z1[c]);
        }
    }
  }
}

// Element e = lane + 64 r of a compact [rows][w] array as (i, j), stepped from r to r + 1 without a division.
struct LqrWalk {
  int i, j, qi, qj, w;
  __device__ __forceinline__ LqrWalk(int lane, int w_) : i(lane / w_), j(lane - (lane / w_) * w_), qi(JACO_WAVE / w_), qj(JACO_WAVE - (JACO_WAVE / w_) * w_), w(w_) {}
  __device__ __forceinline__ void next() {
    i += qi; j += qj;
    if (j >= w) { j -= w; i++; }
  }
};
#define JLQR_REGS_A ((JLQR_MAX_NX * JLQR_MAX_NX + JACO_WAVE - 1) / JACO_WAVE)   // 21
#define JLQR_REGS_B ((JLQR_MAX_NX * JLQR_MAX_NU + JACO_WAVE - 1) / JACO_WAVE)   // 11

JDEV bool lqr_finite(float v) { return fabsf(v) <= 3.4028234e38f; }   // (false for NaN)

JDEV void run_lqr(const JacoLqrArgs& Q_, JacoLqrLDS& s, int i, int lane) {
  const JacoLqrArgs* Q = lqr_args_view(Q_);
  const int T = Q->o.nknots, nx = Q->o.nx, nu = Q->o.nu, rows = Q->rows;
  const int p = wave_uniform_i(Q->p.prob_idx ? Q->p.prob_idx[i] : i);
  if (p < 0 || p >= Q->p.nprob) {   // (neither a fault nor silence)
    if (lane == 0 && Q->out.status) Q->out.status[i] = JLQR_BAD_INDEX;
    return;
  }
  const int ldx = (nx + 3) & ~3, ldu = (nu + 3) & ~3, lda = (nx + 4) & ~3, nxx = nx * nx, nxu = nx * nu;
  const unsigned sk = Q->o.shared_knots, sp = Q->o.shared_probs;
  const LqrWalk wx0(lane, nx), wu0(lane, nu);   // (the two divisions once, not per knot)
  // where an array's block of `words` for (problem p, knot t) starts, its dropped axes taken out
  auto at = [&](const float* base, unsigned bit, int t, int words) -> const float* {
    const size_t knots = (sk & bit) ? 1 : (size_t)T;
    return base + ((sp & bit) ? 0 : (size_t)p * knots * words) + ((sk & bit) ? 0 : (size_t)t * words);
  };
  const float mu = Q->p.mu ? Q->p.mu[i] : 0.f;
  float* const Ka = s.B;   // (K | k), rows of lda
  float* const G = s.W;    // Quu (K | k) + (Qux | Qu), rows of lda

  // the terminal cost-to-go
  {
    const float* V = Q->p.Vxx + ((sp & JLQR_VXX) ? 0 : (size_t)p * nxx);
    LqrWalk w = wx0;
    for (int e = lane; e < nxx; e += JACO_WAVE, w.next()) s.Vxx[w.i * ldx + w.j] = V[e];
    if (lane < nx) s.Vx[lane] = Q->p.Vx ? Q->p.Vx[((sp & JLQR_VX) ? 0 : (size_t)p * nx) + lane] : 0.f;
  }
  // the last knot's A and B into registers
  float pa[JLQR_REGS_A], pb[JLQR_REGS_B];
  auto fetch = [&](int t) {
    const float* A = Q->p.A + ((size_t)p * T + t) * nxx;
    const float* B = Q->p.B + ((size_t)p * T + t) * nxu;
#pragma unroll
    for (int r = 0; r < JLQR_REGS_A; r++) pa[r] = lane + JACO_WAVE * r < nxx ? A[lane + JACO_WAVE * r] : 0.f;
#pragma unroll
    for (int r = 0; r < JLQR_REGS_B; r++) pb[r] = lane + JACO_WAVE * r < nxu ? B[lane + JACO_WAVE * r] : 0.f;
  };
  fetch(T - 1);
  float dV1 = 0.f, dV2 = 0.f;
  unsigned status = 0u;
  wave_sync();

#pragma nounroll
  for (int t = T - 1; t >= 0; t--) {
    // ---- this knot's A and B from the registers to LDS, the next knot's on their way
    {
      LqrWalk wa = wx0, wb = wu0;
#pragma unroll
      for (int r = 0; r < JLQR_REGS_A; r++, wa.next())
        if (lane + JACO_WAVE * r < nxx) s.A[wa.i * ldx + wa.j] = pa[r];
#pragma unroll
      for (int r = 0; r < JLQR_REGS_B; r++, wb.next())
        if (lane + JACO_WAVE * r < nxu) s.B[wb.i * ldu + wb.j] = pb[r];
    }
    wave_sync();
    if (t > 0) fetch(t - 1);

    // ---- W = Vxx A, Y = Vxx B, Qx = lx + A'Vx, Qu = lu + B'Vx
    lqr_gemm(s.Vxx, ldx, 1, s.A, ldx, nx, nx, nx, lane, nullptr, 0, [&](int r, int c, float v) { s.W[r * ldx + c] = v; });
    lqr_gemm(s.Vxx, ldx, 1, s.B, ldu, nx, nu, nx, lane, nullptr, 0, [&](int r, int c, float v) { s.Y[r * ldu + c] = v; });
    {
      const float* lx = Q->p.lx ? at(Q->p.lx, JLQR_LX, t, nx) : nullptr;
      const float* lu = Q->p.lu ? at(Q->p.lu, JLQR_LU, t, nu) : nullptr;
      const float gx = (lx && lane < nx) ? lx[lane] : 0.f, gu = (lu && lane < nu) ? lu[lane] : 0.f;
      const int jx = lane < nx ? lane : 0, ju = lane < nu ? lane : 0;
      float ax = 0.f, au = 0.f;
#pragma unroll JLQR_UNROLL
      for (int k = 0; k < nx; k++) {
        const float v = s.Vx[k];
        ax = fmaf(s.A[k * ldx + jx], v, ax);
        au = fmaf(s.B[k * ldu + ju], v, au);
      }
      if (lane < nx) s.Qx[lane] = ax + gx;
      if (lane < nu) s.Qa[lane * lda + nx] = au + gu;
    }
    wave_sync();

    // ---- Qxx = lxx + A'W (over Vxx), Qux = lux + B'W, Quu = luu + B'Y
    {
      const float* lxx = at(Q->p.lxx, JLQR_LXX, t, nxx);
      const float* luu = at(Q->p.luu, JLQR_LUU, t, nu * nu);
      const float* lux = Q->p.lux ? at(Q->p.lux, JLQR_LUX, t, nxu) : nullptr;
      lqr_gemm(s.A, 1, ldx, s.W, ldx, nx, nx, nx, lane, lxx, nx, [&](int r, int c, float v) { s.Vxx[r * ldx + c] = v; });
      lqr_gemm(s.B, 1, ldu, s.W, ldx, nu, nx, nx, lane, lux, nx, [&](int r, int c, float v) { s.Qa[r * lda + c] = v; });
      lqr_gemm(s.B, 1, ldu, s.Y, ldu, nu, nu, nx, lane, luu, nu, [&](int r, int c, float v) { s.Quu[r * ldu + c] = v; });
    }
    wave_sync();

    // ---- L L' = Quu + mu I, column by column: lane r forms its row's entry of column c from the columns before
    bool bad = false;
#pragma nounroll
    for (int c = 0; c < nu; c++) {
      const int r = (lane >= c && lane < nu) ? lane : c;
      float v = s.Quu[r * ldu + c] + (r == c ? mu : 0.f);
#pragma unroll JLQR_UNROLL
      for (int k = 0; k < c; k++) v = fmaf(-s.L[r * ldu + k], s.L[c * ldu + k], v);
      const float d = wave_bcast(v, c);
      if (!(d > 0.f) || !lqr_finite(d)) { bad = true; break; }   // (d is wave-uniform)
      const float root = sqrtf(d), inv = 1.0f / root;
      if (lane >= c && lane < nu) s.L[lane * ldu + c] = lane == c ? root : v * inv;
      if (lane == c) s.dinv[c] = inv;
      wave_sync();
    }
    if (bad) { status = JLQR_NOT_PD | (unsigned)t; break; }

    // ---- (K | k) = -(L L')^-1 (Qux | Qu): lane c owns column c, forward then backward, in place in its column of Ka
    if (lane <= nx) {
#pragma nounroll
      for (int r = 0; r < nu; r++) {
        float v = -s.Qa[r * lda + lane];
#pragma unroll JLQR_UNROLL
        for (int k = 0; k < r; k++) v = fmaf(-s.L[r * ldu + k], Ka[k * lda + lane], v);
        Ka[r * lda + lane] = v * s.dinv[r];
      }
#pragma nounroll
      for (int r = nu - 1; r >= 0; r--) {
        float v = Ka[r * lda + lane];
#pragma unroll JLQR_UNROLL
        for (int k = r + 1; k < nu; k++) v = fmaf(-s.L[k * ldu + r], Ka[k * lda + lane], v);
        Ka[r * lda + lane] = v * s.dinv[r];
      }
    }
    wave_sync();

    // ---- G = Quu (K | k) + (Qux | Qu); the expected cost change's two terms
    lqr_gemm(s.Quu, ldu, 1, Ka, lda, nu, nx + 1, nu, lane, nullptr, 0, [&](int r, int c, float v) { G[r * lda + c] = v + s.Qa[r * lda + c]; });
    float t1, t2;
    {
      const int a = lane < nu ? lane : 0;
      float m = 0.f;
#pragma unroll JLQR_UNROLL
      for (int c = 0; c < nu; c++) m = fmaf(s.Quu[a * ldu + c], Ka[c * lda + nx], m);
      const float kf = Ka[a * lda + nx];
      wave_sum2(lane < nu ? kf * s.Qa[a * lda + nx] : 0.f, lane < nu ? kf * m : 0.f, &t1, &t2);
    }
    wave_sync();

    // ---- Vxx = Qxx + K'G + Qux'K, Vx = Qx + K'G_k + Qux'k
    lqr_gemm(Ka, 1, lda, G, lda, nx, nx, nu, lane, nullptr, 0, [&](int r, int c, float v) { s.Vxx[r * ldx + c] += v; });
    lqr_gemm(s.Qa, 1, lda, Ka, lda, nx, nx, nu, lane, nullptr, 0, [&](int r, int c, float v) { s.Vxx[r * ldx + c] += v; });
    bool fin = true;
    if (lane < nx) {
      float a = 0.f, b = 0.f;
#pragma unroll JLQR_UNROLL
      for (int k = 0; k < nu; k++) {
        a = fmaf(Ka[k * lda + lane], G[k * lda + nx], a);
        b = fmaf(s.Qa[k * lda + lane], Ka[k * lda + nx], b);
      }
      const float v = (s.Qx[lane] + a) + b;
      s.Vx[lane] = v;
      fin = lqr_finite(v);
    }
    wave_sync();
    // ---- Vxx = 1/2 (Vxx + Vxx'): the lane that holds (r, c) with r <= c writes both; everything checked for finiteness on the way
    {
      LqrWalk w = wx0;
      for (int e = lane; e < nxx; e += JACO_WAVE, w.next())
        if (w.i <= w.j) {
          const float v = 0.5f * (s.Vxx[w.i * ldx + w.j] + s.Vxx[w.j * ldx + w.i]);
          s.Vxx[w.i * ldx + w.j] = v;
          s.Vxx[w.j * ldx + w.i] = v;
          fin = fin && lqr_finite(v);
        }
    }
    float kr[JLQR_REGS_B];   // K of this knot, as the lane will write it
    float kfv = 0.f;
    {
      LqrWalk w = wx0;
#pragma unroll
      for (int r = 0; r < JLQR_REGS_B; r++, w.next()) {
        kr[r] = lane + JACO_WAVE * r < nxu ? Ka[w.i * lda + w.j] : 0.f;
        fin = fin && lqr_finite(kr[r]);
      }
      if (lane < nu) kfv = Ka[lane * lda + nx];
      fin = fin && lqr_finite(kfv) && lqr_finite(t1) && lqr_finite(t2);
    }
    if (wave_ballot(!fin) != 0ull) { status = JLQR_NOT_PD | (unsigned)t; break; }
    dV1 += t1;
    dV2 = fmaf(0.5f, t2, dV2);
    // ---- the knot's rows: control a goes to row row[a]
    {
      const size_t knot = ((size_t)i * T + t) * rows;
      if (Q->out.gain) {
        LqrWalk w = wx0;
#pragma unroll
        for (int r = 0; r < JLQR_REGS_B; r++, w.next())
          if (lane + JACO_WAVE * r < nxu) Q->out.gain[(knot + Q->o.row[w.i]) * nx + w.j] = kr[r];
      }
      if (Q->out.kff && lane < nu) Q->out.kff[knot + Q->o.row[lane]] = kfv;
    }
    wave_sync();
  }

  if (status == 0u) {
    if (Q->out.dV && lane < 2) Q->out.dV[(size_t)i * 2 + lane] = lane == 0 ? dV1 : dV2;
    if (Q->out.Vxx0) {
      LqrWalk w = wx0;
      for (int e = lane; e < nxx; e += JACO_WAVE, w.next()) Q->out.Vxx0[(size_t)i * nxx + e] = s.Vxx[w.i * ldx + w.j];
    }
    if (Q->out.Vx0 && lane < nx) Q->out.Vx0[(size_t)i * nx + lane] = s.Vx[lane];
  }
  if (lane == 0 && Q->out.status) Q->out.status[i] = status;
}

#if JACO_TU_HAS(17)
__global__ __launch_bounds__(64) void jaco_lqr_kernel(JacoLqrArgs Q) {
  __shared__ JacoLqrLDS s;
  JEMU_POISON(s);
  const int i = (int)blockIdx.x;
  if (i >= Q.n) return;
  run_lqr(Q, s, i, (int)threadIdx.x);
}
#endif

#ifndef JACO_EMULATED
void jaco_launch_lqr(unsigned grid, hipStream_t st, const JacoLqrArgs& Q);
#if defined(JACO_TU) && JACO_TU == 17
void jaco_launch_lqr(unsigned grid, hipStream_t st, const JacoLqrArgs& Q) { hipLaunchKernelGGL(jaco_lqr_kernel, dim3(grid), dim3(64), 0, st, Q); }
#endif
#endif
