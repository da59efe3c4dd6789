// hmm_sample_log.hip -- the LOG-SPACE filter launch of HMM posterior sampling for MI355X (gfx950): the second of the three
// launches of svae_hmm_sample_f64 / svae_hmm_ragged_sample_f64 (include/svae_hip.h), between the scaled filter and the
// draw of hmm_sample.hip / hmm_sample_ragged.hip.  It recomputes, all of each, the sequences the scaled filter flagged
// as outside its range (hmm_args.hpp, HMM_LOW: a live component of an unnormalised message below 1e-250 of the step's
// scale, or a normaliser below 1e-200) -- the counterpart of hmm_estep_wide_kernel<KP, LOGSPACE> for the E-step and of
// hmm_vjp_wide_kernel<KP, LOGSPACE> for its derivative.
//
// Mapping: ONE WAVEFRONT PER SEQUENCE, lane = state, KP = 16 / 32 / 64 padded states (KP = 16 stands behind the DPP-row
// kernels: their record stride).  A workgroup whose sequence is not flagged -- its step-0 record's first entry is not
// below 0 (hmm_sample_kernel.hpp: the flagged scaled filter leaves -1 in every live lane there) -- leaves at once.
// Arithmetic (the reference's: K log-sum-exps of KP terms per step, column `lane` of the LOG transition matrix in
// registers, the previous step's vector through a 64-double LDS line read back as broadcast loads):
//   x_0[k] = init[k] + node_0[k];   x_t[k] = logsumexp_j(la_{t-1}[j] + pair[j][k]) + node_t[k]
//   c_t = logsumexp_k x_t[k];       la_t[k] = min(x_t[k] - c_t, 0);      log Z = sum_t c_t
// It overwrites every record 0 .. L-1 of the sequence with la_t (padding lanes -inf) and logZ[b] with log Z.  A step with
// no finite entry (log Z = -inf) stores -inf throughout; NaN potentials give NaN records and a NaN log Z: the draw masks
// every index it derives from them.  RAGGED: steps 0 .. L-1 only, nothing from L on is read or written, and the status
// word is left to the scaled filter.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/svae_hip.h"
#include "dpp.hpp"
#include "hmm_sample_kernel.hpp"

namespace svae {

template <int KP, bool RAGGED>
__global__ __launch_bounds__(64) void hmm_filter_log_kernel(const SampleArgsT<RAGGED> a) {
  __shared__ double line[64];
  const int lane = threadIdx.x;
  const int K = a.K, T = a.T;
  const long b = blockIdx.x;
  double* rec = a.ws + (b * T) * KP;
  if (!(rec[0] < 0.0)) return;                        // (wave-uniform) not flagged by the scaled filter
  const bool st = lane < K;
  const int cc = st ? lane : 0;
  const double NEG_INF = -__builtin_inf();
  int TL = T;
  if constexpr (RAGGED) {
    const int l = a.lengths[b];
    TL = l < 1 ? 1 : (l > T ? T : l);
  }
  const double* pp = a.pair_params + b * a.pair_stride;
  const double* nd = a.node_params + (b * T) * K + cc;
  double* wsb = rec + (lane < KP ? lane : 0);

  double Pc[KP];                                      // Pc[i] = pair[i][lane]; padding: -inf
#pragma unroll
  for (int i = 0; i < KP; ++i) {
    const double v = pp[(i < K ? i : 0) * K + cc];
    Pc[i] = (st && i < K) ? v : NEG_INF;
  }

  // x -> la = x - logsumexp(x), clamped to <= 0; returns the logsumexp (a NaN stays a NaN in both)
  auto normalise = [&](double x, double& la) -> double {
    const double m = smp_wave_max(x);
    const bool some = m > NEG_INF;
    const double s = smp_wave_sum((st && some) ? exp(x - m) : 0.0);
    const double c = some ? m + ::log(s) : NEG_INF;
    const double v = x - c;
    la = (st && some) ? (v > 0.0 ? 0.0 : v) : NEG_INF;
    return c;
  };

  double al;
  double logZ = normalise(st ? a.init_params[cc] + nd[0] : NEG_INF, al);
  if (lane < KP) wsb[0] = al;
  for (int t = 1; t < TL; ++t) {
    const double x = nd[(long)t * K];
    __builtin_amdgcn_wave_barrier();
    line[lane] = al;
    smp_lds_sync();
    double m = NEG_INF;
#pragma unroll
    for (int i = 0; i < KP; ++i) m = __builtin_fmax(m, line[i] + Pc[i]);
    // (the line is read again: KP sums kept live across the two loops would not fit beside Pc at KP = 64)
    asm volatile("" ::: "memory");
    double s = 0.0;
    if (m > NEG_INF) {
#pragma unroll
      for (int i = 0; i < KP; ++i) s += exp(line[i] + Pc[i] - m);
    }
    const double pred = m > NEG_INF ? m + ::log(s) : NEG_INF;
    logZ += normalise(st ? pred + x : NEG_INF, al);
    if (lane < KP) wsb[(long)t * KP] = al;
  }
  if (lane == 0 && a.logZ) a.logZ[b] = logZ;
}

template <bool RAGGED>
static int launch_log(const SampleArgsT<RAGGED>& a, hipStream_t s) {
  const dim3 grid(a.B), block(64);
  if (a.K > 32) hipLaunchKernelGGL((hmm_filter_log_kernel<64, RAGGED>), grid, block, 0, s, a);
  else if (a.K > 16) hipLaunchKernelGGL((hmm_filter_log_kernel<32, RAGGED>), grid, block, 0, s, a);
  else hipLaunchKernelGGL((hmm_filter_log_kernel<16, RAGGED>), grid, block, 0, s, a);
  return hipGetLastError() == hipSuccess ? 0 : -1000;
}

}  // namespace svae

extern "C" int svae_hmm_sample_log_launch(const svae::SampleArgs* a, void* stream) {
  return svae::launch_log<false>(*a, (hipStream_t)stream);
}

extern "C" int svae_hmm_sample_log_ragged_launch(const svae::SampleRaggedArgs* a, void* stream) {
  return svae::launch_log<true>(*a, (hipStream_t)stream);
}
