// hmm_perstep_kernel.hpp -- the kernel template of the HMM recursions with PER-STEP transition potentials (see
// hmm_estep_perstep.hip for the definition of the arithmetic, the mapping and the workspace), shared by
//   hmm_estep_perstep.hip    FILTER = false: the E-step (4 kernels: groups of 8, 16, 32 and 64 lanes)
//   hmm_sample_perstep.hip   FILTER = true:  the forward sweep alone -- la_t into the workspace, the logZ store (logZ may
//                            be NULL there) and return: the filter of posterior sampling (the same 4 groups)
// Every FILTER difference is an `if constexpr`: the E-step's instantiations compile to what they were.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "hmm_units.hpp"    // hmm_perstep_group, hmm_perstep_waves (hmm_args.hpp) and the entry points' host helpers

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

// per group: tile, vector, and per wavefront the row factors and the partial (maximum, sum) pairs
constexpr int hmm_perstep_lds_doubles(int K, int W) { return K * (K | 1) + K + 3 * W * K; }

template <int G, int W, bool FILTER = false>
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
  if constexpr (FILTER) {                        // the sampler's filter: la_t is in the workspace; logZ is optional there
    if (valid && first && lane == 0 && a.logZ) a.logZ[b] = lz;
    return;
  } else {
    if (valid && first && lane == 0) a.logZ[b] = lz;
  }
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

}  // namespace svae
