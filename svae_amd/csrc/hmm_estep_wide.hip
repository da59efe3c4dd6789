// hmm_estep_wide.hip -- batched HMM E-step for 17 <= K <= 64 discrete states on MI355X (gfx950): round 6, lifting the
// K <= 16 limit of hmm_estep.hip (one 16-lane DPP row per sequence) for the state counts the reference's SLDS was used
// with (its compiled kernels take any K: svae/hmm/cython_hmm_inference.pyx:93-166).
//
// What it replaces (reference = mattjj/svae, /root/reference), as hmm_estep.hip:
//   hmm_logZ        svae/hmm/cython_hmm_inference.pyx:93-121   (forward pass)
//   hmm_logZ_grad   svae/hmm/cython_hmm_inference.pyx:126-166  (at g = 1 the E-step: E[z_0], sum_t E[z_t z_{t+1}'], E[z_t])
//
// Mapping: ONE WAVEFRONT PER SEQUENCE, lane j = discrete state j (KP = 32 or 64 padded states; padding carries zero
// mass).  The transition matrix lives in registers -- its column j in the forward pass (KP doubles per lane), its row i
// in the backward pass (the two phases do not overlap) --, the vector that multiplies it (alpha^_t, then e o beta^ / c)
// is published through a KP-double LDS line and read back as wave-uniform (broadcast) loads: a step is KP multiply-adds
// per lane, the backward one 2 KP (the products P[i][j] w[j] also feed the K x K transition counts, KP accumulators per
// lane).  Scaled recursions as hmm_estep.hip: node log-potentials shifted by their maximum and exponentiated once per
// lane, alpha^ renormalised to sum 1 per step, log Z = sum of the log scales.
// Dynamic range (hmm_args.hpp, HMM_LOW): a sequence is trusted while every live component of every step's unnormalised
// message (alpha^_{t-1} P) o e_t stays >= 1e-250 and every normaliser above 1e-200 -- a component a scaled step flushes
// is never rebuilt, whatever the normaliser says.  Any other sequence (a state forbidden by a -1e4 or -inf potential
// counts) is flagged and REDONE IN LOG SPACE, all of it -- the reference's own arithmetic, K log-sum-exps of KP terms
// per step, by that count roughly 10x a scaled sequence's time (LOGSPACE instantiation, second launch: workgroups of unflagged sequences
// leave at once).  hmm_estep_rowlog_kernel (the body at KP = 16, ROW) is that second launch for the DPP-row kernels of hmm_estep.hip:
// their record stride and flag word, and the SLDS sweep's fused node potentials rebuilt from the LDS contractions.
// Bound: LDS broadcast reads + fp64 issue of one wavefront per sequence; the kernel is the general-K path, not a
// tuned one: K = 64, T = 500, 2048 sequences measured in DESIGN.md.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/svae_hip.h"
#include <type_traits>

#include "dpp.hpp"
#include "hmm_args.hpp"

namespace svae {

__device__ __forceinline__ double wave_sum64(double x) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) x += __shfl_xor(x, o, 64);
  return x;
}
__device__ __forceinline__ double wave_max64(double x) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) x = fmax(x, __shfl_xor(x, o, 64));
  return x;
}

// publish one double per lane, then read all KP back as wave-uniform loads
template <int KP>
__device__ __forceinline__ void publish(double* line, int lane, double x) {
  __builtin_amdgcn_wave_barrier();
  line[lane] = x;
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// RAG (svae_hmm_ragged_estep_f64): the sequence's own length TL = lengths[b] (clamped to [1, T]; one wavefront per
// sequence, so it is wave-uniform) bounds every loop; records and outputs keep stride T, nothing stored at t >= TL is
// read, and the scaled launch zeroes E_states from TL on.  The uniform instantiations have TL = T.
template <int KP, bool LOGSPACE, bool RAG, bool ROW>
__device__ __forceinline__ void hmm_estep_wide_body(const std::conditional_t<RAG, HmmRaggedArgs, HmmArgs>& a) {
  static_assert(!ROW || (LOGSPACE && KP == 16), "ROW: the log-space pass behind the DPP-row kernels");
  constexpr int REC = ROW ? HMM_WS : hmm_wide_rec(KP);
  constexpr int FLAG = ROW ? HMM_REDO : KP + 1;          // the sequence's REDO flag (first record)
  constexpr double NEG_BIG = -1.0e300;
  __shared__ double line[64];
  const int lane = threadIdx.x;
  const int K = a.K, T = a.T;
  const int braw = a.seq_index ? a.seq_index[blockIdx.x] : (int)blockIdx.x;
  if (braw < 0) return;                       // (indexed launches: unused slot)
  const long b = braw;
  const bool st = lane < K;
  const int cc = st ? lane : 0;
  double* wsb = a.ws + b * T * REC;
  int TL = T;
  if constexpr (RAG) {
    const int l = a.lengths[b];
    TL = l < 1 ? 1 : (l > T ? T : l);
    if constexpr (!LOGSPACE) {
      if ((l < 1 || l > T) && lane == 0) atomicOr(a.info, 1);
      double* tail = a.E_states + b * T * K;
      for (long q = (long)TL * K + lane; q < (long)T * K; q += 64) tail[q] = 0.0;
    }
  }
  if constexpr (LOGSPACE) {
    if (wsb[FLAG] == 0.0) return;             // not flagged by the scaled pass
  }
  const double* pp = a.pair_params + b * a.pair_stride;
  const double* nd = a.node_params ? a.node_params + (b * T) * K : nullptr;
  // node potential of step t in this lane's state.  ROW without node_params: the fused potentials of the SLDS sweep, in
  // the arithmetic of hmm_estep.hip (node[0] = <E x0 x0', J_c> + <E x0, h_c> + cinit_c; node[t] = pc[t-1][0] + pc[t][1] + lz_c)
  auto node_at = [&](int t) -> double {
    if constexpr (ROW) {
      if (!nd) {
        if (t > 0) {
          const double* pc = a.pair_contr + (b * T) * 2 * K + cc;
          return (pc[(long)(t - 1) * 2 * K] + pc[(long)t * 2 * K + K]) + a.lz[cc];
        }
        const int n = a.n;
        const double* ei = a.lds_E_init + b * (n * n + n);
        const double* Jc = a.init_J + (long)cc * n * n;
        const double* hc = a.init_h + (long)cc * n;
        double s0 = 0.0;
        for (int q = 0; q < n * n; ++q) s0 = __builtin_fma(ei[q], Jc[q], s0);
        double s1 = 0.0;
        for (int q = 0; q < n; ++q) s1 = __builtin_fma(ei[n * n + q], hc[q], s1);
        return (s0 + s1) + a.cinit[cc];
      }
    }
    return nd[(long)t * K + cc];
  };

  // ---- forward pass: column `lane` of the transition matrix in registers ------------------------------------------
  double pmax = NEG_BIG;
  double Pc[KP];
#pragma unroll
  for (int i = 0; i < KP; ++i) {
    const double v = pp[(i < K ? i : 0) * K + cc];
    Pc[i] = (st && i < K) ? v : NEG_BIG;
    pmax = fmax(pmax, Pc[i]);
  }
  pmax = wave_max64(pmax);
  if constexpr (!LOGSPACE) {
#pragma unroll
    for (int i = 0; i < KP; ++i) Pc[i] = (st && i < K) ? exp(Pc[i] - pmax) : 0.0;
  }
  double logZ = 0.0, al;                      // al: alpha^_t[lane] (scaled) or log alpha_t[lane] (log space)
  bool flagged = false;                       // (per lane until the forward pass ends)
  {
    const double x = st ? a.init_params[cc] + node_at(0) : NEG_BIG;
    if constexpr (LOGSPACE) {
      al = x;
    } else {
      const double m = wave_max64(x);
      const double u = st ? exp(x - m) : 0.0;
      const double s = wave_sum64(u);
      flagged = st && !(u >= HMM_LOW);
      al = u / s;
      logZ = m + ::log(s);
      if (lane == 0) wsb[KP] = s;
    }
    if (lane < KP) wsb[lane] = al;
  }
  for (int t = 1; t < TL; ++t) {
    const double x = st ? node_at(t) : NEG_BIG;
    publish<KP>(line, lane, al);
    if constexpr (LOGSPACE) {
      double m = NEG_BIG;
#pragma unroll
      for (int i = 0; i < KP; ++i) m = fmax(m, line[i] + Pc[i]);      // (>= NEG_BIG: every term -inf gives 0, not NaN)
      double s = 0.0;
#pragma unroll
      for (int i = 0; i < KP; ++i) s += exp(line[i] + Pc[i] - m);
      al = st ? m + ::log(s) + x : NEG_BIG;
    } else {
      const double m = wave_max64(x);
      const double e = st ? exp(x - m) : 0.0;
      double v0 = 0.0, v1 = 0.0;
#pragma unroll
      for (int i = 0; i < KP; i += 2) {
        v0 = __builtin_fma(line[i], Pc[i], v0);
        v1 = __builtin_fma(line[i + 1], Pc[i + 1], v1);
      }
      const double u = (v0 + v1) * e;
      const double c = wave_sum64(u);
      flagged = flagged || (st && !(u >= HMM_LOW)) || !(c > HMM_WIDE_TINY);
      al = u / c;
      logZ += ::log(c) + m + pmax;
      if (lane == 0) wsb[(long)t * REC + KP] = c;
    }
    if (lane < KP) wsb[(long)t * REC + lane] = al;
  }
  if constexpr (LOGSPACE) {
    const double m = wave_max64(al);
    logZ = m + ::log(wave_sum64(st ? exp(al - m) : 0.0));
  } else {
    flagged = __any(flagged);
    if (lane == 0) wsb[FLAG] = flagged ? 1.0 : 0.0;
    if (flagged) return;                                       // (wave-uniform) the log-space launch takes it
  }
  if (lane == 0) a.logZ[b] = logZ;

  // ---- backward pass: row `lane` of the transition matrix in registers; transition counts row `lane` ---------------
  double Pr[KP], acc[KP];
#pragma unroll
  for (int j = 0; j < KP; ++j) {
    const double v = pp[cc * K + (j < K ? j : 0)];
    if constexpr (LOGSPACE) Pr[j] = (st && j < K) ? v : NEG_BIG;
    else Pr[j] = (st && j < K) ? exp(v - pmax) : 0.0;
    acc[j] = 0.0;
  }
  double bt = LOGSPACE ? 0.0 : (st ? 1.0 : 0.0);              // beta^_{T-1} = 1  (log beta = 0)
  {
    // (log space: log Z of thousands of nats carries 1e-12 of rounding into exp(. - logZ) -- every step's marginals and
    //  transition terms are scaled by the reciprocal of the marginals' own sum)
    double g = al;
    if constexpr (LOGSPACE) {
      g = st ? exp(al - logZ) : 0.0;
      g /= wave_sum64(g);
    }
    if (st) a.E_states[(b * T + (TL - 1)) * K + lane] = g;
    if (TL == 1 && st) a.E_init[b * K + lane] = g;
  }
  for (int t = TL - 2; t >= 0; --t) {
    const double x = st ? node_at(t + 1) : NEG_BIG;
    const double alt = wsb[(long)t * REC + (lane < KP ? lane : 0)];
    double g;
    if constexpr (LOGSPACE) {
      publish<KP>(line, lane, st ? x + bt : NEG_BIG);          // log (e o beta)_{t+1}
      double m = NEG_BIG;
#pragma unroll
      for (int j = 0; j < KP; ++j) m = fmax(m, Pr[j] + line[j]);
      double s = 0.0;
#pragma unroll
      for (int j = 0; j < KP; ++j) s += exp(Pr[j] + line[j] - m);
      bt = st ? m + ::log(s) : NEG_BIG;
      g = st ? exp(alt + bt - logZ) : 0.0;
      const double rs = 1.0 / wave_sum64(g);
      g *= rs;
      const double base = alt - logZ;                          // xi_t[lane][j] = exp(log alpha_t + log P + log(e beta) - logZ)
#pragma unroll
      for (int j = 0; j < KP; ++j) acc[j] += st ? exp(base + (Pr[j] + line[j])) * rs : 0.0;
    } else {
      const double m = wave_max64(x);
      const double e = st ? exp(x - m) : 0.0;
      const double c = wsb[(long)(t + 1) * REC + KP];
      publish<KP>(line, lane, e * bt / c);                     // w_{t+1}
      double s0 = 0.0, s1 = 0.0;
#pragma unroll
      for (int j = 0; j < KP; j += 2) {
        const double p0 = Pr[j] * line[j], p1 = Pr[j + 1] * line[j + 1];
        s0 += p0; s1 += p1;
        acc[j] = __builtin_fma(alt, p0, acc[j]);
        acc[j + 1] = __builtin_fma(alt, p1, acc[j + 1]);
      }
      bt = s0 + s1;
      g = alt * bt;
    }
    if (st) a.E_states[(b * T + t) * K + lane] = g;
    if (t == 0 && st) a.E_init[b * K + lane] = g;
  }
  if (st) {
#pragma unroll
    for (int j = 0; j < KP; ++j) if (j < K) a.E_trans[(b * K + lane) * K + j] = acc[j];
  }
}

template <int KP, bool LOGSPACE, bool RAG = false>
__global__ __launch_bounds__(64) void hmm_estep_wide_kernel(const std::conditional_t<RAG, HmmRaggedArgs, HmmArgs> a) {
  hmm_estep_wide_body<KP, LOGSPACE, RAG, false>(a);
}

// the log-space pass behind the DPP-row kernels of hmm_estep.hip (K <= 16): the body above at KP = 16 with their records
template <bool RAG>
__global__ __launch_bounds__(64) void hmm_estep_rowlog_kernel(const std::conditional_t<RAG, HmmRaggedArgs, HmmArgs> a) {
  hmm_estep_wide_body<16, true, RAG, true>(a);
}

}  // namespace svae

extern "C" int svae_hmm_wide_launch(const svae::HmmArgs* a, void* stream) {
  hipStream_t s = (hipStream_t)stream;
  dim3 grid(a->B), block(64);
  if (a->K <= 32) {
    hipLaunchKernelGGL((svae::hmm_estep_wide_kernel<32, false>), grid, block, 0, s, *a);
    hipLaunchKernelGGL((svae::hmm_estep_wide_kernel<32, true>), grid, block, 0, s, *a);
  } else {
    hipLaunchKernelGGL((svae::hmm_estep_wide_kernel<64, false>), grid, block, 0, s, *a);
    hipLaunchKernelGGL((svae::hmm_estep_wide_kernel<64, true>), grid, block, 0, s, *a);
  }
  return hipGetLastError() == hipSuccess ? 0 : -1000;
}

// the log-space pass behind the DPP-row kernels (K <= 16, hmm_estep.hip): one wavefront per slot, at work only where the
// scaled pass raised the sequence's REDO flag
extern "C" int svae_hmm_row_logspace_launch(const svae::HmmArgs* a, void* stream) {
  hipLaunchKernelGGL((svae::hmm_estep_rowlog_kernel<false>), dim3(a->B), dim3(64), 0, (hipStream_t)stream, *a);
  return hipGetLastError() == hipSuccess ? 0 : -1000;
}

extern "C" int svae_hmm_row_logspace_ragged_launch(const svae::HmmRaggedArgs* a, void* stream) {
  hipLaunchKernelGGL((svae::hmm_estep_rowlog_kernel<true>), dim3(a->B), dim3(64), 0, (hipStream_t)stream, *a);
  return hipGetLastError() == hipSuccess ? 0 : -1000;
}

extern "C" int svae_hmm_wide_ragged_launch(const svae::HmmRaggedArgs* a, void* stream) {
  hipStream_t s = (hipStream_t)stream;
  dim3 grid(a->B), block(64);
  if (a->K <= 32) {
    hipLaunchKernelGGL((svae::hmm_estep_wide_kernel<32, false, true>), grid, block, 0, s, *a);
    hipLaunchKernelGGL((svae::hmm_estep_wide_kernel<32, true, true>), grid, block, 0, s, *a);
  } else {
    hipLaunchKernelGGL((svae::hmm_estep_wide_kernel<64, false, true>), grid, block, 0, s, *a);
    hipLaunchKernelGGL((svae::hmm_estep_wide_kernel<64, true, true>), grid, block, 0, s, *a);
  }
  return hipGetLastError() == hipSuccess ? 0 : -1000;
}
