// gmm_wide.hip -- the GMM-SVAE local step for latent dimensions up to 16 on MI355X (gfx950, fp64): the per-sweep
// fixed point of gmm.py:90-110 with its final pass and global statistics, the sampler of gaussian.py:27-33, the
// adjoint of the final pass + sampler (the one derived in the header of gmm_train.hip) and the global step
// (dirichlet / niw expectedstats and the prior KL of gmm.py:54-58).  Same contracts as the N <= 8 entries of
// gmm_meanfield.hip (svae_gmm_mw_*) and gmm_train.hip; every entry here accepts 1 <= N <= 16.
//
// Layout: ONE 16-lane DPP row per point (or per NIW component), four per wavefront.  Lane i owns row i of the point's
// matrices -- J (reduced in place to its inverse by Gauss-Jordan without pivoting, i.e. the LDL' elimination: the
// pivots are the d_j of J = Lt D Lt'), Sigma, E[x x'], the unit-lower factor Lt (row i and column i) -- plus h_i and
// mu_i; lanes i >= N hold zero rows and contribute nothing.  Every cross-lane operand is a row broadcast of lane j
// (bcast<j>, row_newbcast) or a row sum (row_sum16); an element that lane i needs from "its own column" of a broadcast
// row is picked by a compile-time select chain, so every register array is indexed by constants (no scratch).  The K
// responsibilities and label potentials of a point are spread over its row: k = 16 q + lane, q < 4 (K <= 64).
// The global potentials G_k are read straight from global memory (row i of block k by lane i: the four rows of a
// wavefront and every wavefront read the same 17 words, an L2/L1 broadcast); K = 64 blocks at N = 16 are 166 KB, more
// than the 160 KB of LDS of a CU, so there is no staged table here.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <type_traits>

#include "../../include/svae_hip.h"
#include "dpp.hpp"
#include "special_fn.hpp"

namespace svae {
namespace gwide {

constexpr int WBLOCK = 256;                 // 16 points (rows) per workgroup
constexpr int WROWS = WBLOCK / 16;
constexpr int WMAX_K = 64;

// log(x 2^eadd), x > 0 normal (the arithmetic of gmm_meanfield.hip's gmm_log2e)
__device__ __forceinline__ double wide_log2e(double x, int eadd) {
  int e = __builtin_amdgcn_frexp_exp(x) + eadd;
  double m = __builtin_amdgcn_frexp_mant(x);
  const bool lo = m < 0.70710678118654752440;
  m = lo ? 2.0 * m : m;
  e = lo ? e - 1 : e;
  const double f = m - 1.0;
  const double s = f * rcp_nr(2.0 + f);
  const double z = s * s;
  double p = 1.0 / 23.0;
  p = __builtin_fma(p, z, 1.0 / 21.0);
  p = __builtin_fma(p, z, 1.0 / 19.0);
  p = __builtin_fma(p, z, 1.0 / 17.0);
  p = __builtin_fma(p, z, 1.0 / 15.0);
  p = __builtin_fma(p, z, 1.0 / 13.0);
  p = __builtin_fma(p, z, 1.0 / 11.0);
  p = __builtin_fma(p, z, 1.0 / 9.0);
  p = __builtin_fma(p, z, 1.0 / 7.0);
  p = __builtin_fma(p, z, 1.0 / 5.0);
  p = __builtin_fma(p, z, 1.0 / 3.0);
  const double t = (s * z) * p;
  const double de = (double)e;
  return __builtin_fma(de, 6.93147180369123816490e-01,
                       __builtin_fma(2.0, s, __builtin_fma(2.0, t, de * 1.90821492927058770002e-10)));
}
__device__ __forceinline__ double wide_log(double x) { return wide_log2e(x, 0); }

// a[i] for a lane-dependent i (a select chain: the array stays in registers)
template <int M>
__device__ __forceinline__ double pick(const double (&a)[M], int i) {
  double v = 0.0;
#pragma unroll
  for (int c = 0; c < M; ++c) v = (c == i) ? a[c] : v;
  return v;
}

__device__ __forceinline__ double row_max16(double x) {
  x = fmax(x, __shfl_xor(x, 1, 16));
  x = fmax(x, __shfl_xor(x, 2, 16));
  x = fmax(x, __shfl_xor(x, 4, 16));
  x = fmax(x, __shfl_xor(x, 8, 16));
  return x;
}

// Row-held factorisation.  On entry lane i holds row i of the SPD matrix J in W (zero rows for i >= N).  Gauss-Jordan
// without pivoting: on return X = row i of J^-1, d[j] = the pivots (every lane), and with WANT_L: Lr = row i of the
// strict part of the unit-lower Lt (J = Lt D Lt'), Lc[m] = Lt_mi for m > i (column i).  Below a pivot Gauss-Jordan
// does exactly the LU elimination, so W_i[j] at step j is L_ij d_j and the pivot row j is d_j Lt_{., j}.
template <int N, bool WANT_L>
__device__ __forceinline__ void row_factor(const int i, double (&W)[N], double (&X)[N], double (&d)[N],
                                           double (&Lr)[N], double (&Lc)[N]) {
#pragma unroll
  for (int c = 0; c < N; ++c) { X[c] = (c == i) ? 1.0 : 0.0; Lr[c] = 0.0; Lc[c] = 0.0; }
  static_for<0, N>([&](auto J_) {
    constexpr int j = decltype(J_)::value;
    double pw[N], px[N];
#pragma unroll
    for (int c = j; c < N; ++c) pw[c] = bcast<j>(W[c]);
#pragma unroll
    for (int c = 0; c <= j; ++c) px[c] = bcast<j>(X[c]);
    const double dj = pw[j];
    d[j] = dj;
    const double r = rcp_nr(dj);
    const bool me = (i == j);
    const double f = me ? 0.0 : W[j] * r;
    if constexpr (WANT_L) {
      Lr[j] = (i > j) ? f : 0.0;
#pragma unroll
      for (int c = j + 1; c < N; ++c) Lc[c] = me ? pw[c] * r : Lc[c];
    }
#pragma unroll
    for (int c = j + 1; c < N; ++c) W[c] = me ? W[c] * r : __builtin_fma(-f, pw[c], W[c]);
    W[j] = me ? 1.0 : 0.0;
#pragma unroll
    for (int c = 0; c <= j; ++c) X[c] = me ? X[c] * r : __builtin_fma(-f, px[c], X[c]);
  });
}

// An empty statement that "rewrites" x: the row broadcasts of x that follow stay behind it (hipcc would otherwise hoist
// all N^2 broadcasts of a loop-invariant row-held matrix at once, far past the register file)
template <int M>
__device__ __forceinline__ void pin(double (&x)[M]) {
#pragma unroll
  for (int c = 0; c < M; ++c) asm volatile("" : "+v"(x[c]));
}

// y = X v for row-held X (lane i: row i) and a row-distributed vector v (lane c: v_c) -> lane i: y_i
template <int N>
__device__ __forceinline__ double row_matvec(const double (&X)[N], double v) {
  double y = 0.0;
  static_for<0, N>([&](auto C_) {
    constexpr int c = decltype(C_)::value;
    y = __builtin_fma(X[c], bcast<c>(v), y);
  });
  return y;
}

// n = chol(J)^-T e = Lt^-T D^-1/2 e for a row-distributed e: back substitution on the columns Lc
template <int N>
__device__ __forceinline__ double row_noise(const double (&Lc)[N], double dis_i, double e_i) {
  double n = e_i * dis_i;
  static_for<0, N>([&](auto M_) {
    constexpr int m = N - 1 - decltype(M_)::value;
    const double nm = bcast<m>(n);
    n = __builtin_fma(-Lc[m], nm, n);          // Lc[m] = 0 for m <= i
  });
  return n;
}

__device__ __forceinline__ double wave_sum64(double v) {
#pragma unroll
  for (int m = 1; m < 64; m <<= 1) v += __shfl_xor(v, m, 64);
  return v;
}

// workgroup total in a fixed order: wavefront butterflies, then ((w0 + w1) + w2) + w3 (every thread returns it)
__device__ __forceinline__ double block_sum(double v, double* red) {
  constexpr int W = WBLOCK / 64;
  v = wave_sum64(v);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  double out = red[0];
#pragma unroll
  for (int w = 1; w < W; ++w) out += red[w];
  return out;
}

struct WideArgs {
  int T, K, max_iter, sweep, mode;    // mode 0: fixed-point sweep `sweep`; 1: final pass
  double tol;
  const double* __restrict__ label_global;
  const double* __restrict__ gaussian_globals;
  const double* __restrict__ node_J;
  const double* __restrict__ node_h;
  const double* __restrict__ label_init;
  double* label_stats;
  double* label_fixed;
  double* gaussian_stats;
  double* label_natparam;
  double* gaussian_natparam;
  double* dirichlet_stats;
  double* niw_stats;
  double* kl;
  int32_t* iters;
  int32_t* assign;
  int32_t* info;
  double* kl_hist;
  double* partials;
  double* spart;
  int32_t* counters;
};

// One point of one sweep (or of the final pass) on the caller's 16-lane row -> the point's KL term (every lane).
// Arithmetic of gmm_point (gmm_meanfield.hip): eta = node + sum_k r_k G_k, Gaussian expected statistics, label
// potentials l_k = <s, G_k>, softmax, KL = <node, s> - logZ(eta) + <r', l> - logsumexp (+ the linear correction term
// of gmm.py:99-102 inside the fixed point).
template <int N>
__device__ __forceinline__ double wide_point(const WideArgs& a, const int t, const int i, const double* rin,
                                             const bool final_pass) {
  constexpr int D = N + 2;
  const int K = a.K;
  const bool act = i < N;
  const int ir = act ? i : 0;
  // ---- eta [gmm.py:113-114]
  double A[N], h = 0.0, cN = 0.0, dN = 0.0;
#pragma unroll
  for (int c = 0; c < N; ++c) A[c] = 0.0;
  for (int k = 0; k < K; ++k) {
    const double rk = rin[k];
    const double* G = a.gaussian_globals + (long)k * D * D;
#pragma unroll
    for (int c = 0; c < N; ++c) A[c] = __builtin_fma(rk, G[ir * D + c], A[c]);
    h = __builtin_fma(rk, G[ir * D + N], h);
    cN = __builtin_fma(rk, G[N * D + N], cN);
    dN = __builtin_fma(rk, G[(N + 1) * D + N + 1], dN);
  }
  const double nJ = act ? a.node_J[(long)t * N + i] : 0.0;
  const double nh = act ? a.node_h[(long)t * N + i] : 0.0;
#pragma unroll
  for (int c = 0; c < N; ++c) A[c] = act ? (c == i ? A[c] + nJ : A[c]) : 0.0;
  h = act ? h + nh : 0.0;
  // ---- Gaussian expected statistics [gaussian.py:11-25]
  double W[N], X[N], d[N], Lr[N], Lc[N];
#pragma unroll
  for (int c = 0; c < N; ++c) W[c] = -2.0 * A[c];
  row_factor<N, false>(i, W, X, d, Lr, Lc);
  bool ok = true;
  // prod_j d_j = detm 2^dete (mantissas in [1/2, 1), exponents summed: pivots of 1e+-20 at N = 16 leave the fp64 range
  // as a plain product; the same bits as the plain product wherever that is a normal number)
  double detm = 1.0;
  int dete = 0;
#pragma unroll
  for (int j = 0; j < N; ++j) {
    ok = ok && (d[j] > 0.0);
    detm *= __builtin_amdgcn_frexp_mant(d[j]);
    dete += __builtin_amdgcn_frexp_exp(d[j]);
  }
  const double mu = row_matvec<N>(X, h);
  double E[N];                                   // row i of E[x x'] = Sigma + mu mu'
  static_for<0, N>([&](auto C_) {
    constexpr int c = decltype(C_)::value;
    E[c] = __builtin_fma(mu, bcast<c>(mu), X[c]);
  });
  const double logZ = 0.5 * row_sum16(h * mu) - 0.5 * wide_log2e(detm, dete) + (cN + dN);
  double klt = row_sum16(act ? __builtin_fma(nJ, pick(E, i), nh * mu) : 0.0) - logZ;   // <node, s> - logZ [gmm.py:116]
  // ---- label update [gmm.py:119-124]: lane (k mod 16) keeps l_k in slot k / 16
  double lsl[4] = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    for (int kk = 0; kk < 16; ++kk) {
      const int k = 16 * q + kk;
      if (k >= K) break;
      const double* G = a.gaussian_globals + (long)k * D * D;
      double p = 0.0;
      if (act) {
#pragma unroll
        for (int c = 0; c < N; ++c) p = __builtin_fma(E[c], G[ir * D + c], p);
        p = __builtin_fma(mu, G[ir * D + N], p);
      }
      const double l = row_sum16(p) + (G[N * D + N] + G[(N + 1) * D + N + 1]) + a.label_global[k];
      lsl[q] = (i == kk) ? l : lsl[q];
    }
  }
  double mx = -1.0 / 0.0;
#pragma unroll
  for (int q = 0; q < 4; ++q) mx = (16 * q + i < K && lsl[q] > mx) ? lsl[q] : mx;
  mx = row_max16(mx);
  double ex[4], sep = 0.0;
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    ex[q] = (16 * q + i < K) ? exp_nonpos(lsl[q] - mx) : 0.0;
    sep += ex[q];
  }
  const double se = row_sum16(sep);
  const double lse = mx + wide_log(se);
  const double inv = rcp_nr(se);
  double labp = 0.0, linp = 0.0, bestv = -1.0;
  int best = 0x7fffffff;
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const int k = 16 * q + i;
    if (k < K) {
      const double l = lsl[q] - a.label_global[k];
      const double rnew = ex[q] * inv;
      const double rold = rin[k];
      labp = __builtin_fma(rnew, l, labp);
      linp = __builtin_fma(rold - rnew, l, linp);
      if (rnew > bestv) { bestv = rnew; best = k; }
      if (final_pass) {
        if (a.label_fixed) a.label_fixed[(long)t * K + k] = rold;
        a.label_natparam[(long)t * K + k] = lsl[q];
      }
      ex[q] = rnew;
    }
  }
  // (all of the row's reads of rin are above this line: the stores below may overwrite it in place)
#pragma unroll
  for (int q = 0; q < 4; ++q) if (16 * q + i < K) a.label_stats[(long)t * K + 16 * q + i] = ex[q];
  // argmax, ties to the lowest k (the order of gmm_point's ascending scan)
#pragma unroll
  for (int m = 1; m < 16; m <<= 1) {
    const double ov = __shfl_xor(bestv, m, 16);
    const int ob = __shfl_xor(best, m, 16);
    if (ov > bestv || (ov == bestv && ob < best)) { bestv = ov; best = ob; }
  }
  klt += row_sum16(labp) - lse;
  // status word, as gmm_point's: a non-positive pivot, or a KL term that is not finite (NaN / infinite node potentials)
  if ((!ok || !(fabs(klt) < 1.0 / 0.0)) && i == 0) {
    int old = *(volatile int32_t*)a.info;
    while (old == 0 || old > t + 1) {
      const int seen = atomicCAS(a.info, old, t + 1);
      if (seen == old) break;
      old = seen;
    }
  }
  if (!final_pass) klt += row_sum16(linp);
  if (final_pass) {
    if (i == 0) a.assign[t] = best;
    double* gs = a.gaussian_stats + (long)t * D * D;
    double* gn = a.gaussian_natparam + (long)t * D * D;
    for (int row = i; row < D; row += 16) {
#pragma unroll
      for (int c = 0; c < D; ++c) {
        double sv = 0.0, nv = 0.0;
        if (row < N) {
          if (c < N) { sv = E[c < N ? c : 0]; nv = A[c < N ? c : 0]; }
          else if (c == N) { sv = mu; nv = h; }
        } else if (row == c) {
          sv = 1.0;
          nv = row == N ? cN : dN;
        }
        gs[row * D + c] = sv;
        gn[row * D + c] = nv;
      }
    }
  }
  return klt;
}

// first sweep index j < upto with |kl_hist[j] - kl_hist[j-1]| < tol (kl_hist[-1] = inf), or -1
__device__ __forceinline__ int converged_at(const double* kl_hist, int upto, double tol) {
  double prev = 1.0 / 0.0;
  for (int j = 0; j < upto; ++j) {
    const double kl = kl_hist[j];
    if (fabs(kl - prev) < tol) return j;
    prev = kl;
  }
  return -1;
}

// One sweep (mode 0) or the final pass (mode 1) over all points: each workgroup reduces its points' KL terms in a fixed
// order into partials[wg]; the last workgroup to arrive sums the partials in index order (bit-reproducible).
template <int N>
__global__ __launch_bounds__(WBLOCK) void wide_sweep_kernel(const WideArgs a) {
  __shared__ double red[WBLOCK / 64];
  __shared__ int sh_flag;
  const int tid = threadIdx.x, i = tid & 15;
  const int conv = converged_at(a.kl_hist, a.sweep, a.tol);
  if (a.mode == 0 && conv >= 0) return;                           // fixed point already reached
  const bool final_pass = a.mode == 1;
  const bool from_init = final_pass ? (a.max_iter == 0) : (a.sweep == 0);
  double klpart = 0.0;
  for (int t = blockIdx.x * WROWS + (tid >> 4); t < a.T; t += gridDim.x * WROWS) {
    const double* rin = (from_init ? a.label_init : a.label_stats) + (long)t * a.K;
    const double kt = wide_point<N>(a, t, i, rin, final_pass);
    klpart += (i == 0) ? kt : 0.0;
  }
  const double wgsum = block_sum(klpart, red);
  if (tid == 0) {
    a.partials[blockIdx.x] = wgsum;
    __threadfence();
    const int ticket = atomicAdd(&a.counters[final_pass ? a.max_iter + 1 : a.sweep], 1);
    sh_flag = (ticket == (int)gridDim.x - 1);
  }
  __syncthreads();
  if (!sh_flag) return;
  __threadfence();
  if (tid >= 64) return;
  double v = 0.0;
  for (int j = tid; j < (int)gridDim.x; j += 64) v += a.partials[j];
  const double total = wave_sum64(v);
  if (tid == 0) {
    if (final_pass) {
      a.kl[0] = total;
      a.iters[0] = conv >= 0 ? conv + 1 : a.max_iter;
    } else {
      a.kl_hist[a.sweep] = total;
    }
  }
}

// dirichlet_stats = sum_t r_t, niw_stats_k = sum_t r_tk stats_t: per-workgroup slices, the last workgroup sums the
// partials in index order
__global__ __launch_bounds__(WBLOCK) void wide_stats_kernel(const WideArgs a, int D, int32_t* counter) {
  __shared__ int sh_flag;
  const int K = a.K, T = a.T, NO = K * (1 + D * D);
  const int per = (T + gridDim.x - 1) / gridDim.x;
  const int t0 = blockIdx.x * per, t1 = min(T, t0 + per);
  for (int j = threadIdx.x; j < NO; j += WBLOCK) {
    double s = 0.0;
    if (j < K) {
      for (int t = t0; t < t1; ++t) s += a.label_stats[(long)t * K + j];
    } else {
      const int k = (j - K) / (D * D), e = (j - K) % (D * D);
      for (int t = t0; t < t1; ++t)
        s = __builtin_fma(a.label_stats[(long)t * K + k], a.gaussian_stats[(long)t * D * D + e], s);
    }
    a.spart[(long)blockIdx.x * NO + j] = s;
  }
  __threadfence();
  __syncthreads();
  if (threadIdx.x == 0) sh_flag = (atomicAdd(counter, 1) == (int)gridDim.x - 1);
  __syncthreads();
  if (!sh_flag) return;
  __threadfence();
  for (int j = threadIdx.x; j < NO; j += WBLOCK) {
    double s = 0.0;
    for (int w = 0; w < (int)gridDim.x; ++w) s += a.spart[(long)w * NO + j];
    if (j < K) a.dirichlet_stats[j] = s; else a.niw_stats[j - K] = s;
  }
}

// ---- sampler and local VJP ------------------------------------------------------------------------------------------
// the factor of a point's (N+2)x(N+2) dense-packed natural parameter: W = -2 A, h
template <int N>
__device__ __forceinline__ void load_factor(const double* gn, int i, double (&X)[N], double (&d)[N], double (&Lr)[N],
                                            double (&Lc)[N], double& h, double& mu) {
  constexpr int D = N + 2;
  const bool act = i < N;
  double W[N];
#pragma unroll
  for (int c = 0; c < N; ++c) W[c] = act ? -2.0 * gn[i * D + c] : 0.0;
  h = act ? gn[i * D + N] : 0.0;
  row_factor<N, true>(i, W, X, d, Lr, Lc);
  mu = row_matvec<N>(X, h);
}

template <int N>
__global__ __launch_bounds__(WBLOCK) void wide_sample_kernel(int T, int S, const double* __restrict__ natparam,
                                                             const double* __restrict__ eps,
                                                             double* __restrict__ samples) {
  constexpr int D = N + 2;
  const int i = threadIdx.x & 15;
  const int t = blockIdx.x * WROWS + (threadIdx.x >> 4);
  if (t >= T) return;                            // (a whole row at a time)
  double X[N], d[N], Lr[N], Lc[N], h, mu;
  load_factor<N>(natparam + (long)t * D * D, i, X, d, Lr, Lc, h, mu);
  const bool act = i < N;
  const double dis = act ? 1.0 / sqrt(pick(d, i)) : 0.0;
  for (int s = 0; s < S; ++s) {
    const double e = act ? eps[((long)t * S + s) * N + i] : 0.0;
    const double n = row_noise<N>(Lc, dis, e);
    if (act) samples[((long)t * S + s) * N + i] = mu + n;
  }
}

// The adjoint of gmm_train.hip's header, row by row:
//   mu_bar = gk (gb + (GA + GA') mu) + sum_s x_bar_s,  h_bar = Sigma mu_bar,
//   J_bar_ii = -[gk (Sigma GA Sigma)_ii + h_bar_i mu_i] + (L^-T Phi(L' L_bar) L^-1)_ii,
//   L_bar = -tril(sum_s n_s z_s'), z_s = L^-1 x_bar_s, L = Lt D^1/2;  g_node_J = -2 J_bar_ii, g_node_h = h_bar.
// Two launches: wide_local_vjp_kernel writes everything but the Cholesky path of the noise, wide_chol_vjp_kernel
// (samples with a cotangent only) adds that term to g_node_J -- in one kernel the two halves' row-held matrices
// exceed the register file at N >= 15.
template <int N>
__global__ __launch_bounds__(WBLOCK) void wide_local_vjp_kernel(
    int T, int K, int S, const double* __restrict__ label_global, const double* __restrict__ gaussian_globals,
    const double* __restrict__ node_J, const double* __restrict__ node_h, const double* __restrict__ natparam,
    const double* __restrict__ label_natparam, const double* __restrict__ g_kl,
    const double* __restrict__ g_samples, double* __restrict__ g_node_J, double* __restrict__ g_node_h) {
  constexpr int D = N + 2;
  const int i = threadIdx.x & 15;
  const int t = blockIdx.x * WROWS + (threadIdx.x >> 4);
  if (t >= T) return;
  const bool act = i < N;
  const int ir = act ? i : 0;
  double X[N], d[N], Lr[N], Lc[N], h, mu;
  load_factor<N>(natparam + (long)t * D * D, i, X, d, Lr, Lc, h, mu);
  const double gk = g_kl ? g_kl[0] : 0.0;
  // ---- cotangent of the statistics: gk (node + sum_k w_k G_k), row i ----
  double GA[N], gb;
  const double nJ = act ? node_J[(long)t * N + i] : 0.0;
#pragma unroll
  for (int c = 0; c < N; ++c) GA[c] = (c == i) ? nJ : 0.0;
  gb = act ? node_h[(long)t * N + i] : 0.0;
  if (gk != 0.0) {
    const double* np_ = label_natparam + (long)t * K;
    double mx = -1.0 / 0.0;
    for (int k = 0; k < K; ++k) mx = np_[k] > mx ? np_[k] : mx;
    double se = 0.0, lbar = 0.0;
    for (int k = 0; k < K; ++k) {
      const double e = exp(np_[k] - mx);
      se += e;
      lbar = __builtin_fma(e, np_[k] - label_global[k], lbar);
    }
    const double inv = 1.0 / se;
    lbar *= inv;
    for (int k = 0; k < K; ++k) {
      const double l = np_[k] - label_global[k];
      const double w = act ? exp(np_[k] - mx) * inv * (l - lbar) : 0.0;
      const double* G = gaussian_globals + (long)k * D * D;
#pragma unroll
      for (int c = 0; c < N; ++c) GA[c] = __builtin_fma(w, G[ir * D + c], GA[c]);
      gb = __builtin_fma(w, G[ir * D + N], gb);
    }
  }
  // mu_bar_i = gk (gb_i + (GA mu)_i + (GA' mu)_i) + sum_s x_bar_s,i
  double s = gb + row_matvec<N>(GA, mu);
  static_for<0, N>([&](auto C_) {
    constexpr int c = decltype(C_)::value;
    const double col = row_sum16(GA[c] * mu);    // (GA' mu)_c
    s += (c == i) ? col : 0.0;
  });
  double mub = gk * s;
  if (g_samples)
    for (int s_ = 0; s_ < S; ++s_) mub += act ? g_samples[((long)t * S + s_) * N + i] : 0.0;
  // (Sigma GA Sigma)_ii = sum_a Sigma_ai (GA Sigma)_ai: R = GA Sigma row-held, then column sums of Sigma .* R
  double acc = 0.0;
  {
    double R[N];
#pragma unroll
    for (int c = 0; c < N; ++c) R[c] = 0.0;
    static_for<0, N>([&](auto B_) {
      constexpr int b = decltype(B_)::value;
      pin(X);
#pragma unroll
      for (int c = 0; c < N; ++c) R[c] = __builtin_fma(GA[b], bcast<b>(X[c]), R[c]);
    });
#pragma unroll
    for (int c = 0; c < N; ++c) {
      const double col = row_sum16(X[c] * R[c]);
      acc += (c == i) ? col : 0.0;
    }
  }
  const double hb = row_matvec<N>(X, mub);
  const double Jb = -(gk * acc + hb * mu);
  if (act) {
    g_node_J[(long)t * N + i] = -2.0 * Jb;
    g_node_h[(long)t * N + i] = hb;
  }
}

template <int N>
__global__ __launch_bounds__(WBLOCK) void wide_chol_vjp_kernel(int T, int S, const double* __restrict__ natparam,
                                                               const double* __restrict__ eps,
                                                               const double* __restrict__ g_samples,
                                                               double* __restrict__ g_node_J) {
  constexpr int D = N + 2;
  const int i = threadIdx.x & 15;
  const int t = blockIdx.x * WROWS + (threadIdx.x >> 4);
  if (t >= T) return;
  const bool act = i < N;
  double X[N], d[N], Lr[N], Lc[N], h, mu;
  load_factor<N>(natparam + (long)t * D * D, i, X, d, Lr, Lc, h, mu);
  const double dis = act ? 1.0 / sqrt(pick(d, i)) : 0.0;
  double Lb[N];                                   // row i of L_bar (c <= i)
#pragma unroll
  for (int c = 0; c < N; ++c) Lb[c] = 0.0;
  for (int s_ = 0; s_ < S; ++s_) {
    const double e = act ? eps[((long)t * S + s_) * N + i] : 0.0;
    const double xb = act ? g_samples[((long)t * S + s_) * N + i] : 0.0;
    const double n = row_noise<N>(Lc, dis, e);
    double z = xb;                               // z = D^-1/2 Lt^-1 x_bar: forward substitution on the rows Lr
    static_for<0, N>([&](auto M_) {
      constexpr int m = decltype(M_)::value;
      z = __builtin_fma(-Lr[m], bcast<m>(z), z);   // Lr[m] = 0 for m >= i
    });
    z *= dis;
    static_for<0, N>([&](auto C_) {
      constexpr int c = decltype(C_)::value;
      const double zc = bcast<c>(z);
      Lb[c] = (c <= i) ? __builtin_fma(-n, zc, Lb[c]) : Lb[c];
    });
  }
  // Ph = Phi(L' L_bar): row i = sqrt(d_i) (Lb_i + sum_{m > i} Lt_mi Lb_m), lower part, diagonal halved
  double Y[N];
#pragma unroll
  for (int c = 0; c < N; ++c) Y[c] = Lb[c];
  static_for<0, N>([&](auto M_) {
    constexpr int m = decltype(M_)::value;
    pin(Lb);
#pragma unroll
    for (int c = 0; c <= m; ++c) Y[c] = __builtin_fma(Lc[m], bcast<m>(Lb[c]), Y[c]);   // Lc[m] = 0 for m <= i
  });
  const double sq = act ? sqrt(pick(d, i)) : 0.0;
#pragma unroll
  for (int c = 0; c < N; ++c) Y[c] = (c < i) ? Y[c] * sq : ((c == i) ? 0.5 * Y[c] * sq : 0.0);
  // Y <- L^-T Ph: L' Y = Ph, L' = D^1/2 Lt': Y_i = dis_i Ph_i - sum_{k > i} Lt_ki Y_k (back substitution)
#pragma unroll
  for (int c = 0; c < N; ++c) Y[c] *= dis;
  static_for<0, N>([&](auto K_) {
    constexpr int k = N - 1 - decltype(K_)::value;
#pragma unroll
    for (int c = 0; c < N; ++c) Y[c] = __builtin_fma(-Lc[k], bcast<k>(Y[c]), Y[c]);   // Lc[k] = 0 for k <= i
  });
  // P_ii = sum_a Y_ia (L^-1)_ai, L^-1 = D^-1/2 Li, Li = Lt^-1 row-held by forward substitution on the rows Lr; row a
  // of Li is final when step a broadcasts it, so its element i is consumed there
  double Li[N];
#pragma unroll
  for (int c = 0; c < N; ++c) Li[c] = (c == i) ? 1.0 : 0.0;
  double P = 0.0;
  static_for<0, N>([&](auto M_) {
    constexpr int m = decltype(M_)::value;
    double lmi = 0.0;                             // Li_{m, i}
#pragma unroll
    for (int c = 0; c <= m; ++c) {
      const double v = bcast<m>(Li[c]);
      lmi = (c == i) ? v : lmi;
      Li[c] = __builtin_fma(-Lr[m], v, Li[c]);    // Lr[m] = 0 for m >= i
    }
    P = __builtin_fma(Y[m], rsqrt_nr(d[m]) * lmi, P);
  });
  if (act) g_node_J[(long)t * N + i] += -2.0 * P;
}

// ---- global step: one row per NIW component ---------------------------------------------------------------------------
// NIW natural parameter (dense (N+2)x(N+2)) -> row i of S^-1 (X), m_i, kappa, nu, log|S|, ok
template <int N>
__device__ __forceinline__ void niw_row_standard(const double* nat, int i, double (&X)[N], double& m, double& kappa,
                                                 double& nu, double& logdet, bool& ok) {
  constexpr int D = N + 2;
  const bool act = i < N;
  kappa = nat[N * D + N];
  nu = nat[(N + 1) * D + N + 1];
  const double bi = act ? nat[i * D + N] : 0.0;
  m = bi / kappa;
  double W[N], d[N], Lr[N], Lc[N];
#pragma unroll
  for (int c = 0; c < N; ++c) {
    const double bc = nat[c * D + N], mc = bc / kappa;
    W[c] = act ? niw_scale_entry(nat[i * D + c], bi, mc, niw_mean_residual(bc, mc, kappa)) : 0.0;
  }
  row_factor<N, false>(i, W, X, d, Lr, Lc);
  ok = (kappa > 0.0) && (nu > (double)(N - 1));      // (NaN / meaningless maps with every pivot positive otherwise)
  logdet = 0.0;
#pragma unroll
  for (int j = 0; j < N; ++j) { ok = ok && (d[j] > 0.0); logdet += log(d[j]); }
}

template <int N>
__device__ __forceinline__ double niw_logZ_row(double nu, double kappa, double logdet) {
  double mg = 0.25 * N * (N - 1) * 1.1447298858494001741;       // log(pi)
#pragma unroll
  for (int j = 0; j < N; ++j) mg += lgamma(0.5 * nu - 0.5 * j);
  return 0.5 * N * nu * 0.6931471805599453094 + mg - 0.5 * nu * logdet - 0.5 * N * log(kappa);
}

// one component on the caller's row -> its contraction term and its logZ differences (prior KL: the Dirichlet log-gamma
// term and the NIW log-normalisers apart) in contr / lz_dir / lz
template <int N>
__device__ __forceinline__ void wide_global_one(const int k, const int i, const double asum,
                                                const double* __restrict__ dir_nat, const double* __restrict__ niw_nat,
                                                const double* __restrict__ prior_dir,
                                                const double* __restrict__ prior_niw,
                                                double* __restrict__ label_global,
                                                double* __restrict__ gaussian_globals, const bool want_kl,
                                                double& es_dir, double& contr, double& lz_dir, double& lz, bool& bad) {
  constexpr int D = N + 2;
  const bool act = i < N;
  // ---- Dirichlet factor (dirichlet.py:5-7) ----
  const double alpha = dir_nat[k] + 1.0;
  es_dir = digamma_pos(alpha) - digamma_pos(asum);
  if (i == 0) label_global[k] = es_dir;
  // ---- NIW factor (niw.py:15-25) ----
  const double* nat = niw_nat + (long)k * D * D;
  double EJ[N], m, kappa, nu, logdet;
  bool ok;
  {
    double X[N];
    niw_row_standard<N>(nat, i, X, m, kappa, nu, logdet, ok);
    static_for<0, N>([&](auto A_) {               // nu sym(S^-1) + 1e-8 I, row i
      constexpr int a_ = decltype(A_)::value;
      double xt = 0.0;                            // (S^-1)_{a, i}
#pragma unroll
      for (int c = 0; c < N; ++c) {
        const double v = bcast<a_>(X[c]);
        xt = (c == i) ? v : xt;
      }
      EJ[a_] = nu * (0.5 * (X[a_] + xt)) + ((a_ == i) ? 1e-8 : 0.0);
    });
  }
  const double Eh = row_matvec<N>(EJ, m);
  const double E_hJh = (double)N / kappa + row_sum16(act ? m * Eh : 0.0);
  double dg = 0.0;
#pragma unroll
  for (int j = 0; j < N; ++j) dg += digamma_pos(0.5 * (nu - j));
  const double E_logdet = dg + N * 0.6931471805599453094 - logdet;
  double* G = gaussian_globals + (long)k * D * D;
  for (int row = i; row < D; row += 16) {
#pragma unroll
    for (int c = 0; c < D; ++c) {
      double v = 0.0;
      if (row < N) {
        if (c < N) v = -0.5 * EJ[c < N ? c : 0];
        else if (c == N) v = Eh;
      } else if (row == N && c == N) {
        v = -0.5 * E_hJh;
      } else if (row == N + 1 && c == N + 1) {
        v = 0.5 * E_logdet;
      }
      G[row * D + c] = v;
    }
  }
  bad = !(ok && alpha > 0.0);
  if (!want_kl) return;
  // ---- prior KL terms (gmm.py:54-58): <eta_q - eta_p, E_q t>, logZ(q) - logZ(p) ----
  const double* pn = prior_niw + (long)k * D * D;
  double pm, pkappa, pnu, plogdet;
  bool pok;
  {
    double PX[N];
    niw_row_standard<N>(pn, i, PX, pm, pkappa, pnu, plogdet, pok);
  }
  double part = 0.0;
  if (act) {
#pragma unroll
    for (int c = 0; c < N; ++c) part = __builtin_fma(nat[i * D + c] - pn[i * D + c], -0.5 * EJ[c], part);
    part = __builtin_fma(nat[i * D + N] - pn[i * D + N], Eh, part);
  }
  contr = row_sum16(part);
  contr = __builtin_fma(dir_nat[k] - prior_dir[k], es_dir, contr);
  contr = __builtin_fma(nat[N * D + N] - pn[N * D + N], -0.5 * E_hJh, contr);
  contr = __builtin_fma(nat[(N + 1) * D + N + 1] - pn[(N + 1) * D + N + 1], 0.5 * E_logdet, contr);
  const double palpha = prior_dir[k] + 1.0;
  lz_dir = lgamma(alpha) - lgamma(palpha);
  lz = niw_logZ_row<N>(nu, kappa, logdet) - niw_logZ_row<N>(pnu, pkappa, plogdet);
  bad = bad || !(pok && palpha > 0.0);
}

// One workgroup of 16 rows; row r takes the components r, r + 16, .. < K.  The sums over components run in index
// order through LDS.
template <int N>
__global__ __launch_bounds__(WBLOCK) void wide_global_step_kernel(int K, const double* __restrict__ dir_nat,
                                                                  const double* __restrict__ niw_nat,
                                                                  const double* __restrict__ prior_dir,
                                                                  const double* __restrict__ prior_niw,
                                                                  double* __restrict__ label_global,
                                                                  double* __restrict__ gaussian_globals,
                                                                  double* __restrict__ kl, int32_t* __restrict__ info) {
  __shared__ double sh_contr[WMAX_K], sh_lz[WMAX_K], sh_lzd[WMAX_K], sh_es0;
  __shared__ int sh_bad;
  const int i = threadIdx.x & 15, r = threadIdx.x >> 4;
  if (threadIdx.x == 0) sh_bad = 0;
  __syncthreads();
  double asum = 0.0;
  for (int j = 0; j < K; ++j) asum += dir_nat[j] + 1.0;
  for (int k = r; k < K; k += WROWS) {
    double es = 0.0, contr = 0.0, lzd = 0.0, lz = 0.0;
    bool bad = false;
    wide_global_one<N>(k, i, asum, dir_nat, niw_nat, prior_dir, prior_niw, label_global, gaussian_globals,
                       kl != nullptr, es, contr, lzd, lz, bad);
    if (i == 0) {
      sh_contr[k] = contr;
      sh_lz[k] = lz;
      sh_lzd[k] = lzd;
      if (k == 0) sh_es0 = es;
      if (bad) atomicOr(&sh_bad, 1);
    }
  }
  __syncthreads();
  if (threadIdx.x != 0) return;
  if (sh_bad) atomicMax(info, 1);
  if (!kl) return;
  double psum = 0.0;
  for (int j = 0; j < K; ++j) psum += prior_dir[j] + 1.0;
  // -(logZ(q) - logZ(p)), the Dirichlet part on its own: sum_k lgamma(alpha_k) and lgamma(sum_k alpha_k) cancel, and an NIW
  // term added to lgamma(1e8) = 1.7e9 first would lose its digits below 2e-7 (svae_gmm_global_step_f64 does the same)
  double c = 0.0, lzd = 0.0, lzn = 0.0;
  for (int j = 0; j < K; ++j) { c += sh_contr[j]; lzd += sh_lzd[j]; lzn += sh_lz[j]; }
  const double mlz = ((lgamma(asum) - lgamma(psum)) - lzd) - lzn;
  kl[0] = c + mlz;
  // kl[1]: the value the reference AS SHIPPED returns (svae_gmm_global_step_f64): the contraction's first term only
  kl[1] = (dir_nat[0] - prior_dir[0]) * sh_es0 + mlz;
}

template <typename Fn>
static int wide_dispatch(int N, Fn&& fn) {
  switch (N) {
    case 1: return fn(std::integral_constant<int, 1>{});
    case 2: return fn(std::integral_constant<int, 2>{});
    case 3: return fn(std::integral_constant<int, 3>{});
    case 4: return fn(std::integral_constant<int, 4>{});
    case 5: return fn(std::integral_constant<int, 5>{});
    case 6: return fn(std::integral_constant<int, 6>{});
    case 7: return fn(std::integral_constant<int, 7>{});
    case 8: return fn(std::integral_constant<int, 8>{});
    case 9: return fn(std::integral_constant<int, 9>{});
    case 10: return fn(std::integral_constant<int, 10>{});
    case 11: return fn(std::integral_constant<int, 11>{});
    case 12: return fn(std::integral_constant<int, 12>{});
    case 13: return fn(std::integral_constant<int, 13>{});
    case 14: return fn(std::integral_constant<int, 14>{});
    case 15: return fn(std::integral_constant<int, 15>{});
    case 16: return fn(std::integral_constant<int, 16>{});
  }
  return -2;
}

static int sweep_grid(int T) {
  const int g = (T + WROWS - 1) / WROWS;
  return g < 1 ? 1 : (g > 2048 ? 2048 : g);
}
static int stats_grid(int T) {
  const int g = (T + 15) / 16;
  return g < 1 ? 1 : (g > 1024 ? 1024 : g);
}
// workspace: kl_hist (max_iter + 1, rounded up to even) | partials (sweep grid) | statistics partials | counters
static size_t ws_doubles(int T, int N, int K, int max_iter) {
  const int D = N + 2;
  return (size_t)((max_iter + 2) & ~1) + (size_t)((sweep_grid(T) + 1) & ~1) + (size_t)stats_grid(T) * K * (1 + D * D);
}

}  // namespace gwide
}  // namespace svae

extern "C" size_t svae_gmm_wide_mw_workspace_bytes(int T, int N, int K, int max_iter) {
  if (T < 0 || N < 1 || N > 16 || K < 1 || K > 64 || max_iter < 0) return 0;
  return svae::gwide::ws_doubles(T, N, K, max_iter) * sizeof(double) + (size_t)(max_iter + 3) * sizeof(int32_t);
}

extern "C" int svae_gmm_wide_mw_begin(int T, int N, int K, int max_iter, void* workspace, size_t ws_bytes,
                                      void* stream) {
  if (T < 0) return -1;
  if (N < 1 || N > 16) return -2;
  if (K < 1 || K > 64) return -3;
  if (max_iter < 0) return -4;
  const size_t need = svae_gmm_wide_mw_workspace_bytes(T, N, K, max_iter);
  if (!workspace || ws_bytes < need) return -5;
  if (hipMemsetAsync(workspace, 0, need, (hipStream_t)stream) != hipSuccess) return -1000;
  return 0;
}

extern "C" int svae_gmm_wide_mw_step_f64(int phase, int sweep, int T, int N, int K,
                                         const double* label_global, const double* gaussian_globals,
                                         const double* node_J, const double* node_h,
                                         const double* label_init, double tol, int max_iter,
                                         double* label_stats, double* label_fixed, double* gaussian_stats,
                                         double* label_natparam, double* gaussian_natparam,
                                         double* dirichlet_stats, double* niw_stats,
                                         double* kl, int32_t* iters, int32_t* assign, int32_t* info,
                                         void* workspace, size_t ws_bytes, void* stream) {
  if (phase < 0 || phase > 2) return -1;
  if (phase == 0 && (sweep < 0 || sweep >= max_iter)) return -2;
  if (T < 0) return -3;
  if (N < 1 || N > 16) return -4;
  if (K < 1 || K > 64) return -5;
  if (!label_global) return -6;
  if (!gaussian_globals) return -7;
  if (T > 0 && (!node_J || !node_h || !label_init)) return -8;
  if (!(tol >= 0.0)) return -11;
  if (max_iter < 0) return -12;
  if (T > 0 && (!label_stats || !gaussian_stats || !label_natparam || !gaussian_natparam)) return -13;
  if (!dirichlet_stats || !niw_stats || !kl || !iters) return -18;
  if (T > 0 && !assign) return -22;
  if (!info) return -23;
  if (!workspace || ws_bytes < svae_gmm_wide_mw_workspace_bytes(T, N, K, max_iter)) return -24;
  namespace w = svae::gwide;
  w::WideArgs a;
  a.T = T; a.K = K; a.max_iter = max_iter; a.tol = tol;
  a.label_global = label_global; a.gaussian_globals = gaussian_globals;
  a.node_J = node_J; a.node_h = node_h; a.label_init = label_init;
  a.label_stats = label_stats; a.label_fixed = label_fixed; a.gaussian_stats = gaussian_stats;
  a.label_natparam = label_natparam; a.gaussian_natparam = gaussian_natparam;
  a.dirichlet_stats = dirichlet_stats; a.niw_stats = niw_stats;
  a.kl = kl; a.iters = iters; a.assign = assign; a.info = info;
  a.kl_hist = (double*)workspace;
  a.partials = a.kl_hist + ((max_iter + 2) & ~1);
  a.spart = a.partials + ((w::sweep_grid(T) + 1) & ~1);
  a.counters = (int32_t*)(a.spart + (size_t)w::stats_grid(T) * K * (1 + (N + 2) * (N + 2)));
  hipStream_t s = (hipStream_t)stream;
  if (phase == 2) {
    a.sweep = max_iter; a.mode = 2;
    hipLaunchKernelGGL(w::wide_stats_kernel, dim3(w::stats_grid(T)), dim3(w::WBLOCK), 0, s, a, N + 2,
                       a.counters + max_iter + 2);
    return hipGetLastError() == hipSuccess ? 0 : -1000;
  }
  a.mode = phase;
  a.sweep = phase == 0 ? sweep : max_iter;
  return w::wide_dispatch(N, [&](auto n) -> int {
    hipLaunchKernelGGL((w::wide_sweep_kernel<decltype(n)::value>), dim3(w::sweep_grid(T)), dim3(w::WBLOCK), 0, s, a);
    return hipGetLastError() == hipSuccess ? 0 : -1000;
  });
}

extern "C" int svae_gmm_wide_sample_f64(int T, int N, int S, const double* gaussian_natparam, const double* eps,
                                        double* samples, void* stream) {
  if (T < 0) return -1;
  if (N < 1 || N > 16) return -2;
  if (S < 0) return -3;
  if (T > 0 && !gaussian_natparam) return -4;
  if (T > 0 && S > 0 && (!eps || !samples)) return -5;
  if (T == 0 || S == 0) return 0;
  namespace w = svae::gwide;
  hipStream_t s = (hipStream_t)stream;
  return w::wide_dispatch(N, [&](auto n) -> int {
    hipLaunchKernelGGL((w::wide_sample_kernel<decltype(n)::value>), dim3((T + w::WROWS - 1) / w::WROWS),
                       dim3(w::WBLOCK), 0, s, T, S, gaussian_natparam, eps, samples);
    return hipGetLastError() == hipSuccess ? 0 : -1000;
  });
}

extern "C" int svae_gmm_wide_local_vjp_f64(int T, int N, int K, int S, const double* label_global,
                                           const double* gaussian_globals, const double* node_J, const double* node_h,
                                           const double* gaussian_natparam, const double* label_natparam,
                                           const double* g_kl, const double* eps, const double* g_samples,
                                           double* g_node_J, double* g_node_h, void* stream) {
  if (T < 0) return -1;
  if (N < 1 || N > 16) return -2;
  if (K < 1 || K > 64) return -3;
  if (S < 0) return -4;
  if (!label_global) return -5;
  if (!gaussian_globals) return -6;
  if (T > 0 && (!node_J || !node_h)) return -7;
  if (T > 0 && (!gaussian_natparam || !label_natparam)) return -9;
  if (g_samples && S > 0 && !eps) return -12;
  if (T > 0 && (!g_node_J || !g_node_h)) return -14;
  if (T == 0) return 0;
  namespace w = svae::gwide;
  hipStream_t s = (hipStream_t)stream;
  const double* gs = (S > 0) ? g_samples : nullptr;
  return w::wide_dispatch(N, [&](auto n) -> int {
    constexpr int NN = decltype(n)::value;
    const dim3 grid((T + w::WROWS - 1) / w::WROWS);
    hipLaunchKernelGGL((w::wide_local_vjp_kernel<NN>), grid, dim3(w::WBLOCK), 0, s, T, K, S, label_global,
                       gaussian_globals, node_J, node_h, gaussian_natparam, label_natparam, g_kl, gs, g_node_J,
                       g_node_h);
    if (hipGetLastError() != hipSuccess) return -1000;
    if (gs)
      hipLaunchKernelGGL((w::wide_chol_vjp_kernel<NN>), grid, dim3(w::WBLOCK), 0, s, T, S, gaussian_natparam, eps, gs,
                         g_node_J);
    return hipGetLastError() == hipSuccess ? 0 : -1000;
  });
}

extern "C" int svae_gmm_wide_global_step_f64(int K, int N, const double* dirichlet_natparam,
                                             const double* niw_natparam, const double* prior_dirichlet,
                                             const double* prior_niw, double* label_global, double* gaussian_globals,
                                             double* kl, int32_t* info, void* stream) {
  if (K < 1 || K > 64) return -1;
  if (N < 1 || N > 16) return -2;
  if (!dirichlet_natparam) return -3;
  if (!niw_natparam) return -4;
  if (kl && (!prior_dirichlet || !prior_niw)) return -5;
  if (!label_global) return -7;
  if (!gaussian_globals) return -8;
  if (!info) return -10;
  namespace w = svae::gwide;
  hipStream_t s = (hipStream_t)stream;
  return w::wide_dispatch(N, [&](auto n) -> int {
    hipLaunchKernelGGL((w::wide_global_step_kernel<decltype(n)::value>), dim3(1), dim3(w::WBLOCK), 0, s, K,
                       dirichlet_natparam, niw_natparam, prior_dirichlet, prior_niw, label_global, gaussian_globals,
                       kl, info);
    return hipGetLastError() == hipSuccess ? 0 : -1000;
  });
}
