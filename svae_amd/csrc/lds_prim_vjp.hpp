// lds_prim_vjp.hpp -- the reference's three reverse-mode LDS primitives, one kernel each, n <= 15 (fp64, gfx950).
//
//   filter VJP    natural_filter_grad            svae/lds/cython_lds_inference.pyx:92-145
//                 (_natural_lognorm_grad, _natural_condition_diag_grad, _natural_predict_grad: cython_gaussian_grads.pxd:17-206)
//   smoother VJP  natural_smoother_general_grad  cython_lds_inference.pyx:236-306 (+ _compute_stats_grad :212-234)
//                 (_rts_backward_step, _rts_backward_step_grad, _rts_{1,2,3}_grad, _info_to_mean_grad: .pxd:208-430)
//   sampler VJP   natural_sample_backward_grad   cython_lds_inference.pyx:357-409
//                 (_natural_sample_grad, _natural_condition_on_grad: .pxd:456-530)
//
// Unlike lds_vjp_kernel.hpp, which differentiates this library's own forward recursion from the records of an E-step
// call, these kernels differentiate the reference's recursions AS FUNCTIONS OF THE FORWARD MESSAGES
// (J_pred, h_pred, J_filt, h_filt) and the pair parameters: every per-step factor the reference keeps as an
// `intermediate` (the Cholesky factors L, v, v2, temp, the smoother's Js/hs/moments, the sampler's J, h) is rebuilt from
// the messages, so a call needs nothing from an earlier launch.  Every pivot is factored (Cholesky) and solved with its
// factor, as the reference does: no explicit inverse is multiplied into J12 (accuracy cond * eps).
//
// Layout: the row tile of dpp.hpp -- one 16-lane DPP row per sequence, lane c holds COLUMN c of every small matrix
// (register i = M[i][c]); vectors are held uniformly in every lane of the row.  Element M[i][k] of another lane is a
// row_newbcast operand: inline-asm v_fmac_f64_dpp / v_mov_b64_dpp statements that carry their own wait states
// (dpp.hpp mac_bc<K, NEG, true>, bcast_fenced<K>; volatile, so the compiler neither hoists nor keeps N^2 broadcast
// values live); sums over lanes are DPP permutations (group_sum<16>).  Matrices are held in the reference's internal scaling (J = precision, J12 -> -J12) and index order
// (its Fortran arrays: the natural (n,n) arrays come in transposed where the reference transposes them).  Transposes go
// through a per-row LDS tile of 16 x 17 doubles; only lanes that own a column of the source write it (tile-store rule,
// DESIGN section 4), so no lane writes outside its own column of its own row's tile.
#pragma once
#include <hip/hip_runtime.h>
#include "dpp.hpp"

namespace svae {

struct PrimArgs {
  int B, T, S;
  long pair_t_stride, pair_seq_stride;     // doubles between steps / sequences of J11, J12, J22 (0: shared)
  const double *J11, *J12, *J22;           // natural pair parameters
  const double *Jp, *hp, *Jf, *hf;         // forward messages (B,T,n,n) / (B,T,n), natural scaling
  // filter VJP
  const double *gJp, *ghp, *gJf, *ghf, *g_lognorm;
  double *g_node_J, *g_node_h, *g_node_logZ;
  // smoother VJP: cotangents of the statistics (each may be NULL), workspace
  const double *g_E_init, *g_E_pair, *g_dxx, *g_x;
  int g_pair_per_step;
  double* ws;
  // sampler VJP
  const double *g_samples, *eps, *samples;
  // message cotangents (smoother and sampler VJPs)
  double *oJp, *ohp, *oJf, *ohf;
  int* info;                               // bit 0 <- a pivot was not positive definite (may be NULL)
};

constexpr int PRIM_TILE = 16 * 17;           // per-row transposition tile (doubles)
constexpr int PRIM_ROWS = 4;                 // sequences per 64-lane block

// smoother VJP workspace per sequence-step: Js, Sigma = Cov[x_t], ExnxT (n x n each), hs, E[x_t] (n each)
__host__ __device__ constexpr long prim_smoother_step_doubles(int n) { return 3L * n * n + 2L * n; }

namespace prim {

template <int N>
__device__ __forceinline__ double pick(const double (&v)[N], int c) {     // v[c] in lane c (0 beyond N)
  double r = 0.0;
  static_for<0, N>([&](auto k) { r = (c == k) ? v[k] : r; });
  return r;
}

// out[s] (lane j) = in[j] (lane s): transpose of an R-row, `cols`-column tile; zeros beyond (R, cols)
template <int R, int RO>
__device__ __forceinline__ void transpose(double* tile, int c, int cols, const double (&in)[R], double (&out)[RO]) {
  __syncthreads();
  if (c < cols) {
    static_for<0, R>([&](auto i) { tile[i * 17 + c] = in[i]; });
  }
  __syncthreads();
  static_for<0, RO>([&](auto s) { out[s] = (c < R && s < cols) ? tile[c * 17 + s] : 0.0; });
}

// load an (N,N) row-major block p as M (lane c = column), scaled; TR: the block's transpose
template <int N, bool TR>
__device__ __forceinline__ void ld(double (&M)[N], const double* p, int c, double scale) {
  static_for<0, N>([&](auto i) { M[i] = (c < N) ? scale * (TR ? p[c * N + i] : p[i * N + c]) : 0.0; });
}
template <int N, bool TR>
__device__ __forceinline__ void ld_add(double (&M)[N], const double* p, int c, double scale) {
  static_for<0, N>([&](auto i) { if (c < N) M[i] += scale * (TR ? p[c * N + i] : p[i * N + c]); });
}
template <int N, bool TR>
__device__ __forceinline__ void st(double* p, const double (&M)[N], int c, double scale) {
  if (c < N) static_for<0, N>([&](auto i) { (TR ? p[c * N + i] : p[i * N + c]) = scale * M[i]; });
}
template <int N>
__device__ __forceinline__ void ldv(double (&v)[N], const double* p, double scale) {
  static_for<0, N>([&](auto i) { v[i] = scale * p[i]; });
}
template <int N>
__device__ __forceinline__ void stv(double* p, const double (&v)[N], int c, double scale) {
  if (c < N) p[c] = scale * pick(v, c);
}

// Cholesky A = L L' (A symmetric, overwritten).  Lc: L (lane c = column), rd = 1/L_ii.
template <int N>
__device__ __forceinline__ void chol(double (&A)[N], double (&Lc)[N], double (&rd)[N], int c, bool& bad) {
  static_for<0, N>([&](auto j) {
    const double d = bcast_fenced<j>(A[j]);
    bad |= !(d > 0.0);                                         // not positive definite (reference: LAPACK info, ignored)
    const double r = rsqrt_nr(d);
    rd[j] = r;
    const double lcj = (c >= j) ? A[j] * r : 0.0;        // L[c][j]: A is symmetric, A[c][j] = A[j][c]
    static_for<0, N>([&](auto i) { Lc[i] = (c == j) ? ((i >= j) ? A[i] * r : 0.0) : Lc[i]; });
    static_for<j + 1, N>([&](auto i) { mac_bc<i, true, true>(A[i], lcj, lcj); });
  });
}

// X <- L^-1 X  (forward substitution; X a matrix in the lane layout or a uniform vector)
template <int N>
__device__ __forceinline__ void trsv_l(const double (&Lc)[N], const double (&rd)[N], double (&X)[N]) {
  static_for<0, N>([&](auto i) {
    double s = X[i];
    static_for<0, i>([&](auto k) { mac_bc<k, true, true>(s, Lc[i], X[k]); });
    X[i] = s * rd[i];
  });
}
// X <- L^-T X  (back substitution)
template <int N>
__device__ __forceinline__ void trsv_lt(const double (&Lc)[N], const double (&rd)[N], double (&X)[N]) {
  static_for<0, N>([&](auto ii) {
    constexpr int i = N - 1 - ii;
    double s = X[i];
    static_for<i + 1, N>([&](auto k) { mac_bc<i, true, true>(s, Lc[k], X[k]); });
    X[i] = s * rd[i];
  });
}

// C += a * A B   (KN = inner dimension: lanes of A's rows / rows of B)
template <int N, int KN, int NB>
__device__ __forceinline__ void mm_ab(double (&C)[N], const double (&A)[N], const double (&B)[NB], double a) {
  static_for<0, N>([&](auto i) {
    double s = 0.0;
    static_for<0, KN>([&](auto k) { mac_bc<k, false, true>(s, A[i], B[k]); });
    C[i] = __builtin_fma(a, s, C[i]);
  });
}
// C += a * A' B   (A: KN x N in the lane layout)
template <int N, int KN, int NA, int NB>
__device__ __forceinline__ void mm_atb(double (&C)[N], const double (&A)[NA], const double (&B)[NB], double a) {
  static_for<0, N>([&](auto i) {
    double s = 0.0;
    static_for<0, KN>([&](auto k) { mac_bc<i, false, true>(s, A[k], B[k]); });
    C[i] = __builtin_fma(a, s, C[i]);
  });
}
// y = A x, y = A' x  (x, y uniform vectors)
template <int N>
__device__ __forceinline__ void mv(double (&y)[N], const double (&A)[N], const double (&x)[N], double a, bool acc) {
  static_for<0, N>([&](auto i) {
    double s = 0.0;
    static_for<0, N>([&](auto k) { mac_bc<k, false, true>(s, A[i], x[k]); });
    y[i] = acc ? __builtin_fma(a, s, y[i]) : a * s;
  });
}
template <int N>
__device__ __forceinline__ void mtv(double (&y)[N], const double (&A)[N], const double (&x)[N], double a, bool acc) {
  static_for<0, N>([&](auto i) {
    double s = 0.0;
    static_for<0, N>([&](auto k) { mac_bc<i, false, true>(s, A[k], x[k]); });
    y[i] = acc ? __builtin_fma(a, s, y[i]) : a * s;
  });
}

// G <- lower(G) + lower(a * X Y')   with Y' given as YT (lane layout of Y', KN rows)
template <int N, int KN, int NX, int NY>
__device__ __forceinline__ void acc_lower_abt(double (&G)[N], const double (&X)[NX], const double (&YT)[NY], double a,
                                              int c) {
  static_for<0, N>([&](auto i) {
    double s = 0.0;
    static_for<0, KN>([&](auto k) { mac_bc<k, false, true>(s, X[i], YT[k]); });
    if (i >= c) G[i] = __builtin_fma(a, s, G[i]);
  });
}

// _cholesky_grad (svae/cython_linalg_grads.pxd:10-26): G holds the lower-triangular cotangent of L; on return the
// symmetric cotangent of A = L L' (off-diagonal halves, the reference's final `symmetrize`).
template <int N>
__device__ __forceinline__ void chol_grad(double (&G)[N], const double (&Lc)[N], const double (&rd)[N], double* tile,
                                          int c) {
  double LT[N];                                                 // lane c: row c of L
  transpose<N, N>(tile, c, N, Lc, LT);
  static_for<0, N>([&](auto i) { if (i < c) G[i] = 0.0; });
  G[N - 1] = (c == N - 1) ? G[N - 1] * (0.5 * rd[N - 1]) : G[N - 1];
  static_for<0, N - 1>([&](auto kk) {
    constexpr int k = N - 2 - kk;
    double Lk[N];
    static_for<k + 1, N>([&](auto i) { Lk[i] = bcast_fenced<k>(Lc[i]); });
    double wB = 0.0;                                            // lane c > k: sum_{j > c} G[j][c] L[j][k]
    static_for<k + 1, N>([&](auto j) { if (j > c) wB = __builtin_fma(G[j], Lk[j], wB); });
    double dot = 0.0;
    static_for<k + 1, N>([&](auto i) {
      const double z = (c > k && c <= i) ? G[i] * LT[k] : 0.0; // sum_{k < j <= i} G[i][j] L[j][k]
      const double y = group_sum<16>(z) + bcast_fenced<i>(wB);         // (sym(G[k+1:,k+1:]) L[k+1:,k])_i
      const double gd = bcast_fenced<i>(G[i]);
      const double nv = (G[i] - y - gd * Lk[i]) * rd[k];
      dot = __builtin_fma(nv, Lk[i], dot);
      G[i] = (c == k) ? nv : G[i];
    });
    G[k] = (c == k) ? (G[k] - dot) * (0.5 * rd[k]) : G[k];
  });
  double Gt[N];
  transpose<N, N>(tile, c, N, G, Gt);
  static_for<0, N>([&](auto i) { G[i] = (i > c) ? 0.5 * G[i] : ((i < c) ? 0.5 * Gt[i] : G[i]); });
}

template <int N>
__device__ __forceinline__ const double* pair_block(const double* base, const PrimArgs& a, int b, int t) {
  return base + (long)b * a.pair_seq_stride + (long)t * a.pair_t_stride;
}

}  // namespace prim

// ---------------------------------------------------------------------------------------------------------------- filter
// natural_filter_grad: t = T-1 .. 0.  Running state: the cotangent of (J_pred,t, h_pred,t) as the filtered message's
// adds to it.  Per step the predict factor L = chol(J_filt,t-1 + J11), v = L^-1 h_filt,t-1, v2 = L^-T v,
// temp = L^-1 J12 is rebuilt from the messages.
template <int N>
__global__ void __launch_bounds__(64) prim_filter_vjp_kernel(const PrimArgs a) {
  using namespace prim;
  __shared__ double tiles[PRIM_ROWS * PRIM_TILE];
  const int c = threadIdx.x & 15, row = threadIdx.x >> 4;
  double* tile = tiles + row * PRIM_TILE;
  const int b0 = blockIdx.x * PRIM_ROWS + row;
  const bool live = b0 < a.B;
  const int b = live ? b0 : a.B - 1;                          // dead rows shadow the last sequence, write nothing
  const int T = a.T;
  const long m = (long)b * T;
  bool bad = false;
  const double g = a.g_lognorm[b];
  double GJ[N], gh[N];                                        // cotangent of the filtered message of step t
  double L[N], rd[N], A[N], v[N];
  // t = T-1: _natural_lognorm_grad on chol(J_filt,T-1)
  ld<N, true>(GJ, a.gJf + (m + T - 1) * N * N, c, -0.5);
  ldv<N>(gh, a.ghf + (m + T - 1) * N, 1.0);
  {
    ld<N, true>(A, a.Jf + (m + T - 1) * N * N, c, -2.0);
    chol<N>(A, L, rd, c, bad);
    ldv<N>(v, a.hf + (m + T - 1) * N, 1.0);
    trsv_l<N>(L, rd, v);
    double w[N], G[N];
    static_for<0, N>([&](auto i) { w[i] = g * v[i]; G[i] = (i == c) ? -g * rd[i] : 0.0; });
    trsv_lt<N>(L, rd, w);                                     // L^-T g_v
    static_for<0, N>([&](auto i) { if (i >= c) G[i] -= w[i] * pick(v, c); });
    chol_grad<N>(G, L, rd, tile, c);
    static_for<0, N>([&](auto i) { GJ[i] += G[i]; gh[i] += w[i]; });
  }
  for (int t = T - 1; t >= 0; --t) {
    // _natural_condition_diag_grad: node cotangents of step t, and the prediction's
    double d = 0.0;
    static_for<0, N>([&](auto i) { d = (c == i) ? GJ[i] : d; });
    if (live && c < N) {
      a.g_node_J[(m + t) * N + c] = -2.0 * d;
      a.g_node_h[(m + t) * N + c] = pick(gh, c);
    }
    if (live && c == 0) a.g_node_logZ[m + t] = g;
    if (t == 0) break;
    // the prediction's cotangent (J_pred,t; h_pred,t): input + the filtered message's
    ld_add<N, true>(GJ, a.gJp + (m + t) * N * N, c, -0.5);
    static_for<0, N>([&](auto i) { gh[i] += a.ghp[(m + t) * N + i]; });
    // _natural_predict_grad at step t-1
    const double* J11 = prim::pair_block<N>(a.J11, a, b, t - 1);
    const double* J12 = prim::pair_block<N>(a.J12, a, b, t - 1);
    ld<N, true>(A, a.Jf + (m + t - 1) * N * N, c, -2.0);
    ld_add<N, false>(A, J11, c, -2.0);
    chol<N>(A, L, rd, c, bad);
    ldv<N>(v, a.hf + (m + t - 1) * N, 1.0);
    trsv_l<N>(L, rd, v);
    double v2[N];
    static_for<0, N>([&](auto i) { v2[i] = v[i]; });
    trsv_lt<N>(L, rd, v2);
    double J12m[N], tmp[N];
    ld<N, false>(J12m, J12, c, -1.0);
    static_for<0, N>([&](auto i) { tmp[i] = J12m[i]; });
    trsv_l<N>(L, rd, tmp);                                    // temp = L^-1 J12
    double S[N], St[N];                                       // sym(g_J_pred)
    transpose<N, N>(tile, c, N, GJ, St);
    static_for<0, N>([&](auto i) { S[i] = 0.5 * (GJ[i] + St[i]); });
    double X[N];                                              // X = L^-T (-2 temp sym(gJp))
    static_for<0, N>([&](auto i) { X[i] = 0.0; });
    mm_ab<N, N, N>(X, tmp, S, -2.0);
    trsv_lt<N>(L, rd, X);
    double tT[N];
    transpose<N, N>(tile, c, N, tmp, tT);
    double G[N];
    static_for<0, N>([&](auto i) { G[i] = 0.0; });
    acc_lower_abt<N, N>(G, X, tT, -1.0, c);                   // lower(-X temp')
    double u[N];
    mv<N>(u, J12m, gh, -1.0, false);                          // -J12 g_h_pred
    trsv_l<N>(L, rd, u);
    const double vc = pick(v, c);
    static_for<0, N>([&](auto i) {
      if (i >= c) G[i] -= v2[i] * pick(u, c);
      if (i == c) G[i] -= g * rd[i];
    });
    double w[N];
    static_for<0, N>([&](auto i) { w[i] = u[i] + g * v[i]; });
    trsv_lt<N>(L, rd, w);
    static_for<0, N>([&](auto i) { if (i >= c) G[i] -= w[i] * vc; });
    chol_grad<N>(G, L, rd, tile, c);
    // the filtered message of step t-1: input + what the prediction passes back
    ld<N, true>(GJ, a.gJf + (m + t - 1) * N * N, c, -0.5);
    static_for<0, N>([&](auto i) { GJ[i] += G[i]; gh[i] = a.ghf[(m + t - 1) * N + i] + w[i]; });
  }
  if (bad && live && a.info) atomicOr(a.info, 1);
}

// -------------------------------------------------------------------------------------------------------------- smoother
// natural_smoother_general_grad.  Phase 1 (t = T-1 .. 0): the reference's RTS recursion on the messages
// (_rts_backward_step), writing Js, Sigma, ExnxT, hs, E[x] per step to the workspace.  Phase 2 (t = 0 .. T-1): the
// adjoint (_rts_backward_step_grad); the step factor L = chol(Js,t+1 - J_pred,t+1 + J22), temp = L^-1 J12',
// temp_n = L^-1 (hs,t+1 - h_pred,t+1) is rebuilt from the workspace and the messages.
template <int N>
__global__ void __launch_bounds__(64) prim_smoother_vjp_kernel(const PrimArgs a) {
  using namespace prim;
  __shared__ double tiles[PRIM_ROWS * PRIM_TILE];
  const int c = threadIdx.x & 15, row = threadIdx.x >> 4;
  double* tile = tiles + row * PRIM_TILE;
  const int b0 = blockIdx.x * PRIM_ROWS + row;
  const bool live = b0 < a.B;
  const int b = live ? b0 : a.B - 1;
  const int T = a.T;
  const long m = (long)b * T;
  bool bad = false;
  constexpr long NN = (long)N * N, SD = prim_smoother_step_doubles(N);
  double* ws = a.ws + m * SD;                     // [t][Js | Sigma | ExnxT | hs | Ex]
  auto wJs = [&](int t) { return ws + t * SD; };
  auto wSig = [&](int t) { return ws + t * SD + NN; };
  auto wX = [&](int t) { return ws + t * SD + 2 * NN; };
  auto whs = [&](int t) { return ws + t * SD + 3 * NN; };
  auto wEx = [&](int t) { return ws + t * SD + 3 * NN + N; };
  double L[N], rd[N], A[N];

  // ---- phase 1
  double Js[N], hs[N], Ex[N], Sig[N];
  // _info_to_mean: Sig = Js^-1 (lower triangle mirrored to the upper, as dpotri + copy_lower_to_upper), Ex = Sig hs
  auto info_to_mean = [&]() __attribute__((always_inline)) {
    static_for<0, N>([&](auto i) { A[i] = Js[i]; Sig[i] = (i == c) ? 1.0 : 0.0; Ex[i] = hs[i]; });
    chol<N>(A, L, rd, c, bad);
    trsv_l<N>(L, rd, Sig);
    trsv_lt<N>(L, rd, Sig);
    double St[N];
    transpose<N, N>(tile, c, N, Sig, St);
    static_for<0, N>([&](auto i) { if (i < c) Sig[i] = St[i]; });
    trsv_l<N>(L, rd, Ex);
    trsv_lt<N>(L, rd, Ex);
  };
  // the workspace keeps E[x x'] = Sig + Ex Ex' (the reference's ExxT); the adjoint recomputes Sig from it
  auto st_exxt = [&](double* p) __attribute__((always_inline)) {
    const double exc = pick(Ex, c);
    double X[N];
    static_for<0, N>([&](auto i) { X[i] = __builtin_fma(Ex[i], exc, Sig[i]); });
    st<N, false>(p, X, c, 1.0);
  };
  ld<N, true>(Js, a.Jf + (m + T - 1) * NN, c, -2.0);
  ldv<N>(hs, a.hf + (m + T - 1) * N, 1.0);
  info_to_mean();
  if (live) { st<N, false>(wJs(T - 1), Js, c, 1.0); st_exxt(wSig(T - 1));
              stv<N>(whs(T - 1), hs, c, 1.0); stv<N>(wEx(T - 1), Ex, c, 1.0); }
  for (int t = T - 1; t > 0; --t) {
    const double* J11 = pair_block<N>(a.J11, a, b, t - 1);
    const double* J12 = pair_block<N>(a.J12, a, b, t - 1);
    const double* J22 = pair_block<N>(a.J22, a, b, t - 1);
    double mun[N];
    static_for<0, N>([&](auto i) { mun[i] = Ex[i]; A[i] = Js[i]; });
    ld_add<N, true>(A, a.Jp + (m + t) * NN, c, 2.0);            // Jns - Jnp + J22
    ld_add<N, false>(A, J22, c, -2.0);
    chol<N>(A, L, rd, c, bad);
    double tmp[N], J12T[N];
    ld<N, true>(J12T, J12, c, -1.0);
    static_for<0, N>([&](auto i) { tmp[i] = J12T[i]; });
    trsv_l<N>(L, rd, tmp);                                       // temp = L^-1 J12'
    double tn[N];
    static_for<0, N>([&](auto i) { tn[i] = hs[i] - a.hp[(m + t) * N + i]; });
    trsv_l<N>(L, rd, tn);
    ld<N, true>(Js, a.Jf + (m + t - 1) * NN, c, -2.0);           // Js = Jf + J11 - temp' temp
    ld_add<N, false>(Js, J11, c, -2.0);
    mm_atb<N, N>(Js, tmp, tmp, -1.0);
    ldv<N>(hs, a.hf + (m + t - 1) * N, 1.0);                     // hs = hf - temp' temp_n
    mtv<N>(hs, tmp, tn, -1.0, true);
    double Lsave[N], rdsave[N];
    static_for<0, N>([&](auto i) { Lsave[i] = L[i]; rdsave[i] = rd[i]; });
    info_to_mean();
    double X[N];                                                 // ExnxT = -L^-T L^-1 (J12' Sigma) + mun Ex'
    static_for<0, N>([&](auto i) { X[i] = 0.0; });
    mm_ab<N, N, N>(X, J12T, Sig, -1.0);
    trsv_l<N>(Lsave, rdsave, X);
    trsv_lt<N>(Lsave, rdsave, X);
    const double exc = pick(Ex, c);
    static_for<0, N>([&](auto i) { X[i] = __builtin_fma(mun[i], exc, X[i]); });
    if (live) { st<N, false>(wJs(t - 1), Js, c, 1.0); st_exxt(wSig(t - 1));
                st<N, false>(wX(t - 1), X, c, 1.0); stv<N>(whs(t - 1), hs, c, 1.0); stv<N>(wEx(t - 1), Ex, c, 1.0); }
  }
  if (bad && live && a.info) atomicOr(a.info, 1);
}

template <int N>
__global__ void __launch_bounds__(64) prim_smoother_vjp2_kernel(const PrimArgs a) {
  using namespace prim;
  __shared__ double tiles[PRIM_ROWS * PRIM_TILE];
  const int c = threadIdx.x & 15, row = threadIdx.x >> 4;
  double* tile = tiles + row * PRIM_TILE;
  const int b0 = blockIdx.x * PRIM_ROWS + row;
  const bool live = b0 < a.B;
  const int b = live ? b0 : a.B - 1;
  const int T = a.T;
  const long m = (long)b * T;
  bool bad = false;
  constexpr long NN = (long)N * N, SD = prim_smoother_step_doubles(N);
  const double* ws = a.ws + m * SD;
  auto wJs = [&](int t) { return ws + t * SD; };
  auto wSig = [&](int t) { return ws + t * SD + NN; };
  auto wX = [&](int t) { return ws + t * SD + 2 * NN; };
  auto whs = [&](int t) { return ws + t * SD + 3 * NN; };
  auto wEx = [&](int t) { return ws + t * SD + 3 * NN + N; };
  double L[N], rd[N], A[N], hs[N], Ex[N], Sig[N];
  double gJs[N], ghs[N], gEx[N];                                  // running cotangents of Js_t, hs_t, E[x_t]
  static_for<0, N>([&](auto i) { gJs[i] = 0.0; ghs[i] = 0.0; gEx[i] = 0.0; });
  auto ld_sigma = [&](int t) __attribute__((always_inline)) {   // Sigma = ExxT - Ex Ex' (_rts_2_grad); Ex loaded
    ld<N, false>(Sig, wSig(t), c, 1.0);
    const double exc = pick(Ex, c);
    static_for<0, N>([&](auto i) { Sig[i] = __builtin_fma(-Ex[i], exc, Sig[i]); });
  };
  auto load_stats_grad = [&](int t, double (&GS)[N]) __attribute__((always_inline)) {            // _compute_stats_grad: g_ExxT_t, g_Ex_t
    static_for<0, N>([&](auto i) { GS[i] = 0.0; });
    if (a.g_dxx) static_for<0, N>([&](auto i) { if (i == c) GS[i] = a.g_dxx[(m + t) * N + i]; });
    if (a.g_x) static_for<0, N>([&](auto i) { gEx[i] += a.g_x[(m + t) * N + i]; });
    if (t == 0 && a.g_E_init) {
      const double* gi = a.g_E_init + (long)b * (NN + N);
      ld_add<N, false>(GS, gi, c, 1.0);
      static_for<0, N>([&](auto i) { gEx[i] += gi[NN + i]; });
    }
    if (a.g_E_pair) {
      const long sb = a.g_pair_per_step ? (long)b * (T - 1) * 3 * NN : (long)b * 3 * NN;
      if (t < T - 1) ld_add<N, false>(GS, a.g_E_pair + sb + (a.g_pair_per_step ? (long)t * 3 * NN : 0), c, 1.0);
      if (t > 0) ld_add<N, false>(GS, a.g_E_pair + sb + (a.g_pair_per_step ? (long)(t - 1) * 3 * NN : 0) + 2 * NN, c, 1.0);
    }
  };
  // _info_to_mean_grad(g_mu = gEx, g_Sigma = GS) into (GJ, gh): mutates GS as the reference does
  auto info_to_mean_grad = [&](double (&GS)[N], double (&GJ)[N], double (&gh)[N]) __attribute__((always_inline)) {
    const double hc = pick(hs, c);
    static_for<0, N>([&](auto i) { GS[i] = __builtin_fma(gEx[i], hc, GS[i]); });
    mtv<N>(gh, Sig, gEx, 1.0, true);
    double Q[N];
    static_for<0, N>([&](auto i) { Q[i] = 0.0; });
    mm_atb<N, N>(Q, Sig, GS, -1.0);                              // -Sigma' g_Sigma
    mm_ab<N, N, N>(GJ, Q, Sig, 1.0);                             // g_J += (-Sigma' g_Sigma) Sigma'  (Sigma symmetric)
  };
  for (int t = 0; t < T - 1; ++t) {
    double GS[N];
    load_stats_grad(t, GS);
    ldv<N>(Ex, wEx(t), 1.0);
    double mun[N], hsn[N];
    ldv<N>(mun, wEx(t + 1), 1.0);
    const double* J12 = pair_block<N>(a.J12, a, b, t);
    const double* J22 = pair_block<N>(a.J22, a, b, t);
    ld<N, false>(A, wJs(t + 1), c, 1.0);
    ld_add<N, true>(A, a.Jp + (m + t + 1) * NN, c, 2.0);
    ld_add<N, false>(A, J22, c, -2.0);
    chol<N>(A, L, rd, c, bad);
    double gL[N];
    static_for<0, N>([&](auto i) { gL[i] = 0.0; });
    // _rts_3_grad
    double gmun[N];
    {
      mv<N>(gEx, GS, Ex, 1.0, true);
      mtv<N>(gEx, GS, Ex, 1.0, true);
      double GX[N];
      if (a.g_E_pair) {
        const long sb = a.g_pair_per_step ? (long)b * (T - 1) * 3 * NN + (long)t * 3 * NN : (long)b * 3 * NN;
        ld<N, true>(GX, a.g_E_pair + sb + NN, c, 1.0);
      } else {
        static_for<0, N>([&](auto i) { GX[i] = 0.0; });
      }
      mv<N>(gmun, GX, Ex, 1.0, false);
      mtv<N>(gEx, GX, mun, 1.0, true);
      double S21[N];
      ld<N, false>(S21, wX(t), c, 1.0);
      const double exc = pick(Ex, c);
      static_for<0, N>([&](auto i) { S21[i] = __builtin_fma(-mun[i], exc, S21[i]); });
      double inter[N];                                           // L' Sigma21
      static_for<0, N>([&](auto i) { inter[i] = 0.0; });
      mm_atb<N, N>(inter, L, S21, 1.0);
      double X[N], XT[N];
      static_for<0, N>([&](auto i) { X[i] = GX[i]; });
      trsv_l<N>(L, rd, X);                                       // L^-1 g
      transpose<N, N>(tile, c, N, X, XT);
      acc_lower_abt<N, N>(gL, S21, XT, -1.0, c);                 // lower(-Sigma21 X')
      trsv_lt<N>(L, rd, X);                                      // Y = L^-T X
      double iT[N];
      transpose<N, N>(tile, c, N, inter, iT);
      acc_lower_abt<N, N>(gL, X, iT, -1.0, c);                   // lower(-Y inter')
      double J12m[N];
      ld<N, false>(J12m, J12, c, -1.0);
      mm_ab<N, N, N>(GS, J12m, X, -1.0);                         // g_ExxT -= J12 Y
    }
    // _rts_2_grad
    ld_sigma(t);
    ldv<N>(hs, whs(t), 1.0);
    info_to_mean_grad(GS, gJs, ghs);
    // _rts_1_grad
    double tmp[N];
    ld<N, true>(tmp, J12, c, -1.0);
    trsv_l<N>(L, rd, tmp);                                       // temp = L^-1 J12'
    double tn[N];
    ldv<N>(hsn, whs(t + 1), 1.0);
    static_for<0, N>([&](auto i) { tn[i] = hsn[i] - a.hp[(m + t + 1) * N + i]; });
    trsv_l<N>(L, rd, tn);
    double av[N];
    mv<N>(av, tmp, ghs, -1.0, false);                            // -temp g_hs
    double T2[N];
    const double ghc = pick(ghs, c);
    static_for<0, N>([&](auto i) { T2[i] = -tn[i] * ghc; });
    trsv_lt<N>(L, rd, av);                                       // b = L^-T a
    const double tnc = pick(tn, c);
    static_for<0, N>([&](auto i) { if (i >= c) gL[i] = __builtin_fma(-av[i], tnc, gL[i]); });
    double Sy[N];
    transpose<N, N>(tile, c, N, gJs, Sy);
    static_for<0, N>([&](auto i) { Sy[i] = 0.5 * (gJs[i] + Sy[i]); });
    mm_ab<N, N, N>(T2, tmp, Sy, -2.0);
    trsv_lt<N>(L, rd, T2);
    double tT[N];
    transpose<N, N>(tile, c, N, tmp, tT);
    acc_lower_abt<N, N>(gL, T2, tT, -1.0, c);
    chol_grad<N>(gL, L, rd, tile, c);
    if (live) {
      st<N, false>(a.oJf + (m + t) * NN, gJs, c, -2.0);
      stv<N>(a.ohf + (m + t) * N, ghs, c, 1.0);
      st<N, false>(a.oJp + (m + t + 1) * NN, gL, c, 2.0);
      stv<N>(a.ohp + (m + t + 1) * N, av, c, -1.0);
    }
    static_for<0, N>([&](auto i) { gJs[i] = gL[i]; ghs[i] = av[i]; gEx[i] = gmun[i]; });
  }
  {  // t = T-1
    double GS[N];
    load_stats_grad(T - 1, GS);
    ldv<N>(hs, whs(T - 1), 1.0); ldv<N>(Ex, wEx(T - 1), 1.0);
    ld_sigma(T - 1);
    mv<N>(gEx, GS, Ex, 1.0, true);
    mtv<N>(gEx, GS, Ex, 1.0, true);
    double GJ[N], gh[N];
    static_for<0, N>([&](auto i) { GJ[i] = gJs[i]; gh[i] = ghs[i]; });
    info_to_mean_grad(GS, GJ, gh);
    if (live) {
      st<N, false>(a.oJf + (m + T - 1) * NN, GJ, c, -2.0);
      stv<N>(a.ohf + (m + T - 1) * N, gh, c, 1.0);
      double z[N];
      static_for<0, N>([&](auto i) { z[i] = 0.0; });
      st<N, false>(a.oJp + m * NN, z, c, 1.0);
      stv<N>(a.ohp + m * N, z, c, 1.0);
    }
  }
  if (bad && live && a.info) atomicOr(a.info, 1);
}

// --------------------------------------------------------------------------------------------------------------- sampler
// natural_sample_backward_grad, t = 0 .. T-1.  Lanes hold the S <= 16 samples of the (n, S) blocks.  Step factor
// L = chol(J_filt,t + J11) (t < T-1; J_filt,T-1 at the last step), h_t = h_filt,t - J12 x_t+1.
template <int N>
__global__ void __launch_bounds__(64) prim_sample_vjp_kernel(const PrimArgs a) {
  using namespace prim;
  __shared__ double tiles[PRIM_ROWS * PRIM_TILE];
  const int c = threadIdx.x & 15, row = threadIdx.x >> 4;
  double* tile = tiles + row * PRIM_TILE;
  const int b0 = blockIdx.x * PRIM_ROWS + row;
  const bool live = b0 < a.B;
  const int b = live ? b0 : a.B - 1;
  const int T = a.T, S = a.S;
  const long m = (long)b * T;
  bool bad = false;
  constexpr long NN = (long)N * N;
  const bool sl = c < S;
  auto ld_ns = [&](double (&X)[N], const double* p) __attribute__((always_inline)) {             // (S, n) block -> lanes = samples
    static_for<0, N>([&](auto i) { X[i] = sl ? p[(long)c * N + i] : 0.0; });
  };
  double gx[N];                                                   // cotangent of x_t (the carried part)
  static_for<0, N>([&](auto i) { gx[i] = 0.0; });
  double L[N], rd[N], A[N];
  for (int t = 0; t < T; ++t) {
    const long st_off = (m + t) * (long)S * N;
    double G[N];
    ld_ns(G, a.g_samples + st_off);
    static_for<0, N>([&](auto i) { G[i] += gx[i]; });
    ld<N, true>(A, a.Jf + (m + t) * NN, c, -2.0);
    double H[N];
    static_for<0, N>([&](auto i) { H[i] = sl ? a.hf[(m + t) * N + i] : 0.0; });
    double J12m[N];
    if (t < T - 1) {
      ld_add<N, false>(A, pair_block<N>(a.J11, a, b, t), c, -2.0);
      ld<N, false>(J12m, pair_block<N>(a.J12, a, b, t), c, -1.0);
      double Xn[N];
      ld_ns(Xn, a.samples + st_off + (long)S * N);
      // h = h_filt - J12 x_t+1  (J12m = -J12_nat: the internal J12; _natural_condition_on)
      double P[N];
      static_for<0, N>([&](auto i) { P[i] = 0.0; });
      mm_ab<N, N, N>(P, J12m, Xn, 1.0);
      static_for<0, N>([&](auto i) { if (sl) H[i] -= P[i]; });
    }
    chol<N>(A, L, rd, c, bad);
    trsv_l<N>(L, rd, H);                                          // inter = L^-1 h
    double MU[N];
    static_for<0, N>([&](auto i) { MU[i] = H[i]; });
    trsv_lt<N>(L, rd, MU);                                        // mu = L^-T L^-1 h
    double E[N];
    ld_ns(E, a.eps + st_off);
    trsv_lt<N>(L, rd, E);                                         // zero-mean part L^-T eps
    static_for<0, N>([&](auto i) { MU[i] += E[i]; });
    double X[N];
    static_for<0, N>([&](auto i) { X[i] = G[i]; });
    trsv_l<N>(L, rd, X);                                          // L^-1 g
    double XT[16], HT[16];
    transpose<N, 16>(tile, c, S, X, XT);                          // (n,S) -> lane j holds row j
    double gL[N];
    static_for<0, N>([&](auto i) { gL[i] = 0.0; });
    // lower(-(mu + zm) X'): products over the S samples (lanes of MU / rows of XT)
    static_for<0, N>([&](auto i) {
      double s = 0.0;
      static_for<0, 16>([&](auto k) { mac_bc<k, false, true>(s, MU[i], XT[k]); });
      if (i >= c) gL[i] -= s;
    });
    trsv_lt<N>(L, rd, X);                                         // Y = L^-T L^-1 g = g_h
    transpose<N, 16>(tile, c, S, H, HT);
    static_for<0, N>([&](auto i) {                                // lower(-Y inter')
      double s = 0.0;
      static_for<0, 16>([&](auto k) { mac_bc<k, false, true>(s, X[i], HT[k]); });
      if (i >= c) gL[i] -= s;
    });
    chol_grad<N>(gL, L, rd, tile, c);
    double ghf[N];
    static_for<0, N>([&](auto i) { ghf[i] = group_sum<16>(sl ? X[i] : 0.0); });
    if (live) {
      st<N, true>(a.oJf + (m + t) * NN, gL, c, -2.0);
      stv<N>(a.ohf + (m + t) * N, ghf, c, 1.0);
      double z[N];
      static_for<0, N>([&](auto i) { z[i] = 0.0; });
      st<N, false>(a.oJp + (m + t) * NN, z, c, 1.0);
      stv<N>(a.ohp + (m + t) * N, z, c, 1.0);
    }
    if (t < T - 1) {                                              // _natural_condition_on_grad: g_x_t+1 -= J12' g_h
      static_for<0, N>([&](auto i) { gx[i] = 0.0; });
      mm_atb<N, N>(gx, J12m, X, -1.0);
      static_for<0, N>([&](auto i) { if (!sl) gx[i] = 0.0; });
    }
  }
  if (bad && live && a.info) atomicOr(a.info, 1);
}

template <int N>
int launch_prim(int which, const PrimArgs& a, hipStream_t stream) {
  const dim3 grid((a.B + PRIM_ROWS - 1) / PRIM_ROWS), block(64);
  if (which == 0) hipLaunchKernelGGL(prim_filter_vjp_kernel<N>, grid, block, 0, stream, a);
  else if (which == 1) {
    hipLaunchKernelGGL(prim_smoother_vjp_kernel<N>, grid, block, 0, stream, a);
    hipLaunchKernelGGL(prim_smoother_vjp2_kernel<N>, grid, block, 0, stream, a);
  }
  else hipLaunchKernelGGL(prim_sample_vjp_kernel<N>, grid, block, 0, stream, a);
  return hipGetLastError() == hipSuccess ? 0 : -1000;
}

}  // namespace svae
