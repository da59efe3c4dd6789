// hmm_perstep_vjp_kernel.hpp -- the kernel template of the reverse-mode derivative of the HMM E-step with PER-STEP
// transition potentials (hmm_estep_perstep_vjp.hip states the arithmetic, the mapping and the workspace).  A template of
// its own: hmm_perstep_kernel.hpp and its instantiations stay what they are.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "hmm_units.hpp"    // hmm_perstep_group, hmm_perstep_waves (hmm_args.hpp) and the entry points' host helpers

namespace svae {

struct HmmPerstepVjpArgs {
  int B, T, K;
  long pair_stride;                        // doubles between sequences' (T-1,K,K) blocks of pair_params (0 = shared)
  const double* __restrict__ init_params;  // (K)
  const double* __restrict__ pair_params;  // (T-1,K,K) or (B,T-1,K,K)
  const double* __restrict__ node_params;  // (B,T,K)
  const int32_t* __restrict__ lengths;     // (B) or nullptr
  const double* __restrict__ g_logZ;       // (B) or nullptr
  const double* __restrict__ g_init;       // (B,K) or nullptr
  const double* __restrict__ g_trans;      // (B,T-1,K,K) or nullptr
  const double* __restrict__ g_states;     // (B,T,K) or nullptr
  double* __restrict__ d_init;             // (B,K)
  double* __restrict__ d_pair;             // (B,T-1,K,K) or nullptr
  double* __restrict__ d_node;             // (B,T,K)
  int32_t* __restrict__ info;              // status word (nullptr only with lengths == nullptr)
  double* __restrict__ ws;                 // (B,T,2K): [la_t | r_t]
};

// per group: the e tile and the V tile, the two broadcast vectors, and per wavefront the row factors and the partial
// (maximum, sum, weighted sum) triples
constexpr int hmm_perstep_vjp_lds_doubles(int K, int W) { return 2 * K * (K | 1) + 2 * K + 4 * W * K; }

// LDS is sized at compile time for the widest K of the group width (K = G); the tiles' row stride is the run-time K | 1
template <int G, int W>
__global__ __launch_bounds__(64 * W) void hmm_perstep_vjp_kernel(const HmmPerstepVjpArgs a) {
  constexpr int PER_GROUP = hmm_perstep_vjp_lds_doubles(G, W);
  __shared__ double smem[(64 / G) * PER_GROUP];
  const int K = a.K, T = a.T, KS = K | 1;
  const int wv = threadIdx.x >> 6, tl = threadIdx.x & 63;
  const int lane = tl & (G - 1), grp = tl / G;
  const long b = (long)blockIdx.x * (64 / G) + grp;
  const bool valid = b < a.B;                    // an idle group shadows the last sequence for one step and stores nothing
  const long bb = valid ? b : a.B - 1;
  const bool live = lane < K;
  const bool first = wv == 0;                    // the wavefront that stores what all W hold alike
  const bool hasV = a.g_trans != nullptr;
  const bool hasW = a.g_states != nullptr;
  const bool store = a.d_pair != nullptr;
  double* tile = smem + grp * PER_GROUP;         // K x KS: la_t + P_t forward; P_t, then e_jk backward
  double* vtile = tile + K * KS;                 // K x KS: V_t (backward)
  double* vec = vtile + K * KS;                  // la_t forward; node_{t+1} + lb_{t+1} backward
  double* vec2 = vec + K;                        // r_t forward; y_{t+1}, then c + r_t backward
  double* cs = vec2 + K;                         // [W][K] row factors, per quarter of the columns
  double* pm = cs + W * K;                       // [W][K] partial maxima
  double* psm = pm + W * K;                      // [W][K] partial sums, each relative to its own maximum
  double* pws = psm + W * K;                     // [W][K] partial weighted sums, likewise
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
  const double* gV = hasV ? a.g_trans + bb * (T - 1) * KK : nullptr;
  const double* gW = hasW ? a.g_states + bb * T * K : nullptr;
  double* rec = a.ws + bb * T * 2 * K;
  double* dn = a.d_node + bb * T * K;
  const double NINF = -INFINITY;

  // the W partial triples of index `lane` -> (M, S, A): sum_w (s_w, a_w) exp(m_w - M); an empty or all -inf share is 0
  auto combine = [&](double& M, double& S, double& A) {
    M = NINF;
#pragma unroll
    for (int w = 0; w < W; ++w) M = fmax(M, pm[w * K + lane]);
    const double Ms = M == NINF ? 0.0 : M;
    S = 0.0;
    A = 0.0;
#pragma unroll
    for (int w = 0; w < W; ++w) {
      const double f = exp(pm[w * K + lane] - Ms);
      S += psm[w * K + lane] * f;
      A += pws[w * K + lane] * f;
    }
    return Ms;
  };

  double pmax = NINF, psum = 0.0, pwsum = 0.0;   // W = 1: the one share's triple stays in registers
  // ---- forward: la_t, r_t ----------------------------------------------------------------------------------------------------
  double al = NINF, r = 0.0;
  if (live) {
    al = a.init_params[lane] + node[lane];
    r = (a.g_init ? a.g_init[bb * K + lane] : 0.0) + (hasW ? gW[lane] : 0.0);
    if (valid && first) {
      rec[lane] = al;
      rec[K + lane] = r;
    }
  }
  for (int t = 0; t + 1 < Lmax; ++t) {
    const bool act = live && t + 1 < L;
    if (live && first) {
      vec[lane] = al;
      vec2[lane] = r;
    }
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
      double s = 0.0, ws = 0.0;
      if (hasV) {
        const double* V = gV + t * KK + lane;
#pragma unroll 4
        for (int j = q0; j < q1; ++j) {
          const double e = exp(col[j * KS] - ms);
          s += e;
          ws += e * (vec2[j] + V[(long)j * K]);
        }
      } else {
#pragma unroll 4
        for (int j = q0; j < q1; ++j) {
          const double e = exp(col[j * KS] - ms);
          s += e;
          ws += e * vec2[j];
        }
      }
      if constexpr (W > 1) {
        pm[wv * K + lane] = m;
        psm[wv * K + lane] = s;
        pws[wv * K + lane] = ws;
      } else {
        pmax = m;
        psum = s;
        pwsum = ws;
      }
    }
    if constexpr (W > 1) __syncthreads();
    if (act) {
      double M = pmax, S = psum, A = pwsum;
      if constexpr (W > 1) combine(M, S, A);
      al = M + log(S) + node[(long)(t + 1) * K + lane];
      r = (S > 0.0 ? A / S : 0.0) + (hasW ? gW[(long)(t + 1) * K + lane] : 0.0);
      if (valid && first) {
        rec[(long)(t + 1) * 2 * K + lane] = al;
        rec[(long)(t + 1) * 2 * K + K + lane] = r;
      }
    }
  }

  // ---- logZ, E[phi]: every lane adds the same terms in the same order --------------------------------------------------------
  __syncthreads();
  if (live && first) {
    vec[lane] = al;
    vec2[lane] = r;
  }
  __syncthreads();
  double lz, c;
  {
    double m = NINF;
    for (int k = 0; k < K; ++k) m = fmax(m, vec[k]);
    const double ms = m == NINF ? 0.0 : m;
    double s = 0.0;
    for (int k = 0; k < K; ++k) s += exp(vec[k] - ms);
    lz = m + log(s);
    double ephi = 0.0;
    for (int k = 0; k < K; ++k) ephi += exp(vec[k] - lz) * vec2[k];
    c = (a.g_logZ ? a.g_logZ[bb] : 0.0) - ephi;
  }
  __syncthreads();

  // ---- backward: lb_t, s_t, gamma_t; d_node, d_pair --------------------------------------------------------------------------
  double wb = NINF, yb = 0.0;                    // node_{t+1} + lb_{t+1} and y_{t+1} = W[t+1] + s_{t+1} of state `lane`
  if (live) {
    const double g = exp(al - lz);               // t = L - 1: lb = 0, s = 0
    const double d = g * (c + r);
    wb = node[(long)(L - 1) * K + lane];
    yb = hasW ? gW[(long)(L - 1) * K + lane] : 0.0;
    if (valid && first) {
      dn[(long)(L - 1) * K + lane] = d;
      if (L == 1) a.d_init[b * K + lane] = d;
    }
  }
  double* dp = store ? a.d_pair + bb * (T - 1) * KK : nullptr;
  for (int t = Lmax - 2; t >= 0; --t) {
    const bool act = live && t + 1 < L;
    if (act) {
      if (first) {
        vec[lane] = wb;
        vec2[lane] = yb;
      }
      const double* P = pair + t * KK + lane;
      double* col = tile + lane;
#pragma unroll 4
      for (int j = q0; j < q1; ++j) col[j * KS] = P[(long)j * K];
      if (hasV) {
        const double* V = gV + t * KK + lane;
        double* vcol = vtile + lane;
#pragma unroll 4
        for (int j = q0; j < q1; ++j) vcol[j * KS] = V[(long)j * K];
      }
    }
    __syncthreads();
    if (act) {                                   // row `lane`, columns q0 .. q1-1
      double* row = tile + lane * KS;
      const double* vrow = vtile + lane * KS;
      double m = NINF;
#pragma unroll 4
      for (int k = q0; k < q1; ++k) m = fmax(m, row[k] + vec[k]);
      const double ms = m == NINF ? 0.0 : m;
      double s = 0.0, ws = 0.0;
      if (hasV) {
#pragma unroll 4
        for (int k = q0; k < q1; ++k) {
          const double e = exp(row[k] + vec[k] - ms);
          s += e;
          ws += e * (vrow[k] + vec2[k]);
          if (store) row[k] = e;
        }
      } else {
#pragma unroll 4
        for (int k = q0; k < q1; ++k) {
          const double e = exp(row[k] + vec[k] - ms);
          s += e;
          ws += e * vec2[k];
          if (store) row[k] = e;
        }
      }
      if constexpr (W > 1) {
        pm[wv * K + lane] = m;
        psm[wv * K + lane] = s;
        pws[wv * K + lane] = ws;
      } else {
        pmax = m;
        psum = s;
        pwsum = ws;
      }
    }
    if constexpr (W > 1) __syncthreads();
    const double yold = yb;                      // y_{t+1}[lane]: the store pass's column term
    if (act) {
      double M = pmax, S = psum, A = pwsum, shift = 1.0;
      if constexpr (W > 1) {
        const double Ms = combine(M, S, A);
        shift = exp(pm[wv * K + lane] - Ms);
      }
      const double lb = M + log(S);
      const double st = S > 0.0 ? A / S : 0.0;
      const double g = exp(rec[(long)t * 2 * K + lane] + lb - lz);
      const double cr = c + rec[(long)t * 2 * K + K + lane];
      const double d = g * (cr + st);
      // this wavefront's columns of row `lane` hold e relative to its own maximum: gamma q = e (gamma / S) exp(m_w - M)
      cs[wv * K + lane] = S > 0.0 ? g / S * shift : 0.0;
      if (first) vec2[lane] = cr;                // every reader of y_{t+1} is behind the barrier above (W = 1: this wavefront)
      wb = node[(long)t * K + lane] + lb;
      yb = (hasW ? gW[(long)t * K + lane] : 0.0) + st;
      if (valid && first) {
        dn[(long)t * K + lane] = d;
        if (t == 0) a.d_init[b * K + lane] = d;
      }
    }
    __syncthreads();
    if (store && act && valid) {                 // column `lane`, rows q0 .. q1-1
      const double* f = cs + (lane / Q) * K;     // the factors of the share column `lane` was reduced in
      double* X = dp + t * KK + lane;
      const double* col = tile + lane;
      if (hasV) {
        const double* vcol = vtile + lane;
#pragma unroll 4
        for (int j = q0; j < q1; ++j) X[(long)j * K] = col[j * KS] * f[j] * (vec2[j] + vcol[j * KS] + yold);
      } else {
#pragma unroll 4
        for (int j = q0; j < q1; ++j) X[(long)j * K] = col[j * KS] * f[j] * (vec2[j] + yold);
      }
    }
    __syncthreads();
  }

  // ---- the padded tails: exactly 0.0 ----------------------------------------------------------------------------------------
  if (valid && L < T) {
    if (live && first)
      for (int t = L; t < T; ++t) dn[(long)t * K + lane] = 0.0;
    if (store)
      for (long i = (L - 1) * KK + wv * G + lane; i < (T - 1) * KK; i += G * W) dp[i] = 0.0;
  }
}

}  // namespace svae
