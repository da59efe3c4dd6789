// hmm_estep_perstep.hip -- batched HMM E-step with PER-STEP transition potentials for MI355X (gfx950), K <= 64:
// svae_hmm_perstep_estep_f64 / svae_hmm_perstep_workspace_bytes (include/svae_hip.h).
//
//   log p(z) ∝ init[z_0] + sum_{t<L-1} pair[t][z_t][z_{t+1}] + sum_{t<L} node[t][z_t],   pair (T-1,K,K) or (B,T-1,K,K)
//
// ONE ROUTE, log space throughout.  With a fixed matrix the scaled kernels (hmm_estep.hip, hmm_estep_wide.hip) pay the K^2
// exponentials once per sequence; with P_t new at every step a scaled step pays them too (exp(P_t - max P_t)), which is
// exactly the exponential count of a log-sum-exp step -- so the scaled recursion would save nothing but the K logarithms,
// and would need the range criterion, the REDO flags and a second launch behind it.  Here every step is
//   forward :  la_{t+1}[k] = node_{t+1}[k] + logsumexp_j(la_t[j] + P_t[j][k])
//   backward:  lb_t[j]     = logsumexp_k(P_t[j][k] + w_{t+1}[k]),   w_{t+1} = node_{t+1} + lb_{t+1},  lb_{L-1} = 0
//   gamma_t[j] = exp(la_t[j] + lb_t[j] - logZ),   logZ = logsumexp_k la_{L-1}[k]
//   xi_t[j][k] = e_jk gamma_t[j] / s_j,   e_jk = exp(P_t[j][k] + w_{t+1}[k] - m_j),  s_j = sum_k e_jk  (m_j the row's maximum)
// so the pair marginals reuse the backward step's own exponentials: 2 K^2 exp per step in all, and every row of xi_t sums to
// gamma_t[j] by construction.  An offset common to one P_t moves la, lb and logZ alike and cancels; a -inf entry is a term
// exp(-inf) = 0; an all -inf row or column gives -inf (never inf - inf: the shift of an empty maximum is 0).
//
// Mapping: a group of G = 8, 16, 32 or 64 lanes per sequence (the smallest G >= K), lane = state, 64 / G sequences per
// workgroup of W wavefronts: W = 1 for K <= 16; W = 4 for K > 16, where one SIMD's exp issue bounds the step -- every
// wavefront holds the same groups and takes a quarter of each reduction (of j forward, of k backward), the four partial
// (maximum, sum) pairs meet in LDS and every wavefront combines them alike, sum_w s_w exp(m_w - M), so all W hold the
// same la, lb and gamma and the first stores them.  Per group in LDS: a K x KS tile (KS = K | 1, an odd row stride: column reads by lane = k and
// row reads by lane = j are both free of bank conflicts), the broadcast vector (la_t, then w_{t+1}), and per wavefront
// the partial pairs and the row factors gamma_t[j] / s_j exp(m_w - m_j) of its quarter of the columns.
//   forward  lane k reads column k of P_t straight from memory (consecutive lanes, consecutive addresses) and keeps
//            la_t[j] + P_t[j][k] in its tile column between the maximum pass and the exponential pass.
//   backward the group copies P_t into the tile (coalesced), lane j reduces row j, overwrites it with e_jk, and after the
//            barrier lane k writes column k of xi_t = tile[j][k] * (gamma_t[j] / s_j): full-width coalesced stores.  With
//            E_trans == NULL the tile is not written back and that pass is skipped; the other outputs do not change a bit.
// Workspace: la_t, (B,T,K) doubles, written by the forward sweep (first wavefront) and read back behind workgroup barriers.
// Lengths: L = lengths[b] clamped to [1,T]; a workgroup loops to the longest of its sequences with the shorter ones
// predicated off (no load, no store, registers frozen), so no sequence's arithmetic depends on a neighbour's length.
// E_states[b, L:] and E_trans[b, L-1:] are stored as 0.0; nothing at node steps >= L or pair steps >= L-1 is loaded.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "../../include/svae_hip.h"

namespace svae {

// a separate type: the uniform kernels' HmmArgs and the ragged HmmRaggedArgs (hmm_args.hpp) stay what they are
struct HmmPerstepArgs {
  int B, T, K;
  long pair_stride;                        // doubles between sequences' (T-1,K,K) blocks (0 = shared)
  const double* __restrict__ init_params;  // (K)
  const double* __restrict__ pair_params;  // (T-1,K,K) or (B,T-1,K,K)
  const double* __restrict__ node_params;  // (B,T,K)
  const int32_t* __restrict__ lengths;     // (B) or nullptr
  double* __restrict__ logZ;               // (B)
  double* __restrict__ E_init;             // (B,K)
  double* __restrict__ E_trans;            // (B,T-1,K,K) or nullptr
  double* __restrict__ E_states;           // (B,T,K)
  int32_t* __restrict__ info;              // status word (nullptr only with lengths == nullptr)
  double* __restrict__ ws;                 // (B,T,K) log alpha
};

constexpr int hmm_perstep_group(int K) { return K <= 8 ? 8 : K <= 16 ? 16 : K <= 32 ? 32 : 64; }
constexpr int hmm_perstep_waves(int K) { return K <= 16 ? 1 : 4; }
// per group: tile, vector, and per wavefront the row factors and the partial (maximum, sum) pairs
constexpr int hmm_perstep_lds_doubles(int K, int W) { return K * (K | 1) + K + 3 * W * K; }

template <int G, int W>
__global__ __launch_bounds__(64 * W) void hmm_perstep_kernel(const HmmPerstepArgs a) {
  extern __shared__ double smem[];
  const int K = a.K, T = a.T, KS = K | 1;
  const int wv = threadIdx.x >> 6, tl = threadIdx.x & 63;
  const int lane = tl & (G - 1), grp = tl / G;
  const long b = (long)blockIdx.x * (64 / G) + grp;
  const bool valid = b < a.B;                    // an idle group shadows the last sequence for one step and stores nothing
  const long bb = valid ? b : a.B - 1;
  const bool live = lane < K;
  const bool first = wv == 0;                    // the wavefront that stores what all W hold alike
  const bool want = a.E_trans != nullptr;
  double* tile = smem + (long)grp * hmm_perstep_lds_doubles(K, W);
  double* vec = tile + K * KS;
  double* cs = vec + K;                          // [W][K] row factors, per quarter of the columns
  double* pm = cs + W * K;                       // [W][K] partial maxima
  double* psm = pm + W * K;                      // [W][K] partial sums, each relative to its own maximum
  const int Q = (K + W - 1) / W;                 // this wavefront's share of every reduction: indices q0 .. q1-1
  const int q0 = min(wv * Q, K), q1 = min(q0 + Q, K);

  int L = T;
  if (a.lengths) {
    const int l = a.lengths[bb];
    if ((l < 1 || l > T) && valid && first && lane == 0) atomicOr(a.info, 1);
    L = min(max(l, 1), T);
  }
  if (!valid) L = 1;
  int Lmax = L;                                  // the workgroup's trip count (every wavefront holds the same groups)
  for (int o = G; o < 64; o <<= 1) Lmax = max(Lmax, __shfl_xor(Lmax, o));

  const long KK = (long)K * K;
  const double* node = a.node_params + bb * T * K;
  const double* pair = a.pair_params + bb * a.pair_stride;
  double* la = a.ws + bb * T * K;
  double* Es = a.E_states + bb * T * K;
  const double NINF = -INFINITY;

  // the W partial (maximum, sum) pairs of index `lane` -> (M, S): sum_w s_w exp(m_w - M); an empty or all -inf share is 0
  auto combine = [&](double& M, double& S) {
    M = NINF;
#pragma unroll
    for (int w = 0; w < W; ++w) M = fmax(M, pm[w * K + lane]);
    const double Ms = M == NINF ? 0.0 : M;
    S = 0.0;
#pragma unroll
    for (int w = 0; w < W; ++w) S += psm[w * K + lane] * exp(pm[w * K + lane] - Ms);
    return Ms;
  };

  double pmax = NINF, psum = 0.0;                // W = 1: the one share's (maximum, sum) stays in registers
  // ---- forward: la_t -----------------------------------------------------------------------------------------------------
  double al = NINF;
  if (live) {
    al = a.init_params[lane] + node[lane];
    if (valid && first) la[lane] = al;
  }
  for (int t = 0; t + 1 < Lmax; ++t) {
    const bool act = live && t + 1 < L;
    if (live && first) vec[lane] = al;
    __syncthreads();
    if (act) {
      const double* P = pair + t * KK + lane;
      double* col = tile + lane;
      double m = NINF;
#pragma unroll 4
      for (int j = q0; j < q1; ++j) {
        const double v = vec[j] + P[(long)j * K];
        col[j * KS] = v;
        m = fmax(m, v);
      }
      const double ms = m == NINF ? 0.0 : m;
      double s = 0.0;
#pragma unroll 4
      for (int j = q0; j < q1; ++j) s += exp(col[j * KS] - ms);
      if constexpr (W > 1) {
        pm[wv * K + lane] = m;
        psm[wv * K + lane] = s;
      } else {
        pmax = m;
        psum = s;
      }
    }
    if constexpr (W > 1) __syncthreads();
    if (act) {
      double M = pmax, S = psum;
      if constexpr (W > 1) combine(M, S);
      al = M + log(S) + node[(long)(t + 1) * K + lane];
      if (valid && first) la[(long)(t + 1) * K + lane] = al;
    }
  }

  // ---- logZ = logsumexp_k la_{L-1}[k]: every lane adds the same terms in the same order -------------------------------------
  __syncthreads();
  if (live && first) vec[lane] = al;
  __syncthreads();
  double lz;
  {
    double m = NINF;
    for (int k = 0; k < K; ++k) m = fmax(m, vec[k]);
    const double ms = m == NINF ? 0.0 : m;
    double s = 0.0;
    for (int k = 0; k < K; ++k) s += exp(vec[k] - ms);
    lz = m + log(s);
  }
  if (valid && first && lane == 0) a.logZ[b] = lz;
  __syncthreads();

  // ---- backward: lb_t, gamma_t, xi_t ---------------------------------------------------------------------------------------
  double wb = NINF;                              // w_{t+1}[lane] = node_{t+1} + lb_{t+1}
  if (live) {
    const double g = exp(al - lz);               // t = L - 1: lb = 0
    wb = node[(long)(L - 1) * K + lane];
    if (valid && first) {
      Es[(long)(L - 1) * K + lane] = g;
      if (L == 1) a.E_init[b * K + lane] = g;
    }
  }
  double* Et = want ? a.E_trans + bb * (T - 1) * KK : nullptr;
  for (int t = Lmax - 2; t >= 0; --t) {
    const bool act = live && t + 1 < L;
    if (act) {
      if (first) vec[lane] = wb;
      const double* P = pair + t * KK + lane;
      double* col = tile + lane;
#pragma unroll 4
      for (int j = q0; j < q1; ++j) col[j * KS] = P[(long)j * K];
    }
    __syncthreads();
    if (act) {                                   // row `lane`, columns q0 .. q1-1
      double* row = tile + lane * KS;
      double m = NINF;
#pragma unroll 4
      for (int k = q0; k < q1; ++k) m = fmax(m, row[k] + vec[k]);
      const double ms = m == NINF ? 0.0 : m;
      double s = 0.0;
      if (want) {
#pragma unroll 4
        for (int k = q0; k < q1; ++k) {
          const double e = exp(row[k] + vec[k] - ms);
          s += e;
          row[k] = e;
        }
      } else {
#pragma unroll 4
        for (int k = q0; k < q1; ++k) s += exp(row[k] + vec[k] - ms);
      }
      if constexpr (W > 1) {
        pm[wv * K + lane] = m;
        psm[wv * K + lane] = s;
      } else {
        pmax = m;
        psum = s;
      }
    }
    if constexpr (W > 1) __syncthreads();
    if (act) {
      double M = pmax, S = psum, shift = 1.0;
      if constexpr (W > 1) {
        const double Ms = combine(M, S);
        shift = exp(pm[wv * K + lane] - Ms);
      }
      const double lb = M + log(S);
      const double g = exp(la[(long)t * K + lane] + lb - lz);
      // this wavefront's columns of row `lane` hold e relative to its own maximum: xi = e (gamma / S) exp(m_w - M)
      cs[wv * K + lane] = S > 0.0 ? g / S * shift : 0.0;
      wb = node[(long)t * K + lane] + lb;
      if (valid && first) {
        Es[(long)t * K + lane] = g;
        if (t == 0) a.E_init[b * K + lane] = g;
      }
    }
    __syncthreads();
    if (want && act && valid) {                  // column `lane`, rows q0 .. q1-1
      const double* f = cs + (lane / Q) * K;     // the factors of the share column `lane` was reduced in
      double* X = Et + t * KK + lane;
      const double* col = tile + lane;
#pragma unroll 4
      for (int j = q0; j < q1; ++j) X[(long)j * K] = col[j * KS] * f[j];
    }
    __syncthreads();
  }

  // ---- the padded tails: exactly 0.0 ----------------------------------------------------------------------------------------
  if (valid && L < T) {
    if (live && first)
      for (int t = L; t < T; ++t) Es[(long)t * K + lane] = 0.0;
    if (want)
      for (long i = (L - 1) * KK + wv * G + lane; i < (T - 1) * KK; i += G * W) Et[i] = 0.0;
  }
}

template <int G, int W>
static void launch_perstep(const HmmPerstepArgs& a, hipStream_t s) {
  constexpr int SPB = 64 / G;
  const size_t lds = (size_t)SPB * hmm_perstep_lds_doubles(a.K, W) * sizeof(double);
  hipLaunchKernelGGL((hmm_perstep_kernel<G, W>), dim3((unsigned)((a.B + SPB - 1) / SPB)), dim3(64 * W), lds, s, a);
}

}  // namespace svae

extern "C" size_t svae_hmm_perstep_workspace_bytes(int B, int T, int K) {
  if (B <= 0 || T <= 0 || K < 1 || K > SVAE_HMM_MAX_K) return 0;
  const size_t bytes = (size_t)B * T * K * sizeof(double);
  return (bytes + 127) & ~(size_t)127;
}

extern "C" int svae_hmm_perstep_estep_f64(int B, int T, int K, int pair_batched,
                                          const double* init_params, const double* pair_params,
                                          const double* node_params, const int32_t* lengths,
                                          double* logZ, double* E_init, double* E_trans, double* E_states,
                                          int32_t* info, void* workspace, size_t ws_bytes, void* stream) {
  if (B < 0) return -1;
  if (T < 1) return -2;
  if (K < 1 || K > SVAE_HMM_MAX_K) return -3;
  if (pair_batched != 0 && pair_batched != 1) return -4;
  if (!init_params) return -5;
  if (!pair_params && T > 1) return -6;
  if (B == 0) return 0;
  if (!node_params) return -7;
  if (!logZ) return -8;
  if (!E_init) return -9;
  if (!E_states) return -10;
  if (lengths && !info) return -11;
  if (!workspace) return -12;
  if (ws_bytes < svae_hmm_perstep_workspace_bytes(B, T, K)) return -13;
  if (((uintptr_t)workspace & 15) != 0) return -14;
  svae::HmmPerstepArgs a;
  a.B = B; a.T = T; a.K = K; a.pair_stride = pair_batched ? (long)(T - 1) * K * K : 0;
  a.init_params = init_params; a.pair_params = pair_params; a.node_params = node_params; a.lengths = lengths;
  a.logZ = logZ; a.E_init = E_init; a.E_trans = E_trans; a.E_states = E_states; a.info = info;
  a.ws = (double*)workspace;
  hipStream_t s = (hipStream_t)stream;
  switch (svae::hmm_perstep_group(K)) {
    case 8: svae::launch_perstep<8, 1>(a, s); break;
    case 16: svae::launch_perstep<16, 1>(a, s); break;
    case 32: svae::launch_perstep<32, 4>(a, s); break;
    default: svae::launch_perstep<64, 4>(a, s); break;
  }
  return hipGetLastError() == hipSuccess ? 0 : -1000;
}
