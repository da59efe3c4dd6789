// hmm_sample_ragged.hip -- batched HMM posterior sampling with PER-SEQUENCE LENGTHS for MI355X (gfx950): the RAGGED
// instantiations of the four kernel templates of hmm_sample_kernel.hpp (filter and draw, row K = 1 .. 16, wide KP = 32 and
// 64) and their entry point svae_hmm_ragged_sample_f64 (include/svae_hip.h).  One padded (B, T, K) batch, sequence b
// sampled as if cut to its own L = lengths[b] steps under the arithmetic hmm_sample.hip defines: states[b, :, :L] and
// logZ[b] are those of the cut sequence, states[b, :, L:] = -1, and neither node_params[b, L:] nor u[b, :, L:] is read.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/svae_hip.h"
#include "dpp.hpp"
#include "hmm_sample_kernel.hpp"

// hmm_sample_log.hip: the log-space filter, at work on the sequences the scaled filter flagged
extern "C" int svae_hmm_sample_log_ragged_launch(const svae::SampleRaggedArgs* a, void* stream);

namespace svae {

template <int K>
static void launch_sample_row_ragged(const SampleRaggedArgs& a, hipStream_t s) {
  hipLaunchKernelGGL((hmm_filter_row_kernel<K, true>), dim3((a.B + 3) / 4), dim3(64), 0, s, a);
  svae_hmm_sample_log_ragged_launch(&a, s);
  const long R = (long)a.B * a.S;
  hipLaunchKernelGGL((hmm_draw_row_kernel<K, true>), dim3((unsigned)((R + 3) / 4)), dim3(64), 0, s, a);
}
template <int KP>
static void launch_sample_wide_ragged(const SampleRaggedArgs& a, hipStream_t s) {
  hipLaunchKernelGGL((hmm_filter_wide_kernel<KP, true>), dim3(a.B), dim3(64), 0, s, a);
  svae_hmm_sample_log_ragged_launch(&a, s);
  hipLaunchKernelGGL((hmm_draw_wide_kernel<KP, true>), dim3((unsigned)((long)a.B * a.S)), dim3(64), 0, s, a);
}

}  // namespace svae

extern "C" int svae_hmm_ragged_sample_f64(int B, int T, int K, int S, int pair_batched,
                                          const double* init_params, const double* pair_params,
                                          const double* node_params, const int32_t* lengths, const double* u,
                                          int32_t* states, double* logZ,
                                          int32_t* info, void* workspace, size_t ws_bytes, void* stream) {
  if (B < 0) return -1;
  if (T < 1) return -2;
  if (K < 1 || K > SVAE_HMM_MAX_K) return -3;
  if (pair_batched != 0 && pair_batched != 1) return -4;
  if (!init_params) return -5;
  if (!pair_params) return -6;
  if (B == 0) return 0;
  if (!node_params) return -7;
  if (!lengths) return -8;
  if (S < 1) return -9;
  if (!u) return -10;
  if (!states) return -11;
  if (!info) return -12;
  if (!workspace) return -13;
  if (ws_bytes < svae_hmm_sample_workspace_bytes(B, T, K)) return -14;
  if (((uintptr_t)workspace & 15) != 0) return -15;
  svae::SampleRaggedArgs a;
  a.B = B; a.T = T; a.K = K; a.S = S; a.pair_stride = pair_batched ? (long)K * K : 0;
  a.init_params = init_params; a.pair_params = pair_params; a.node_params = node_params;
  a.u = u; a.states = states; a.logZ = logZ; a.ws = (double*)workspace;
  a.lengths = lengths; a.info = info;
  hipStream_t s = (hipStream_t)stream;
  if (K > 32) {
    svae::launch_sample_wide_ragged<64>(a, s);
  } else if (K > 16) {
    svae::launch_sample_wide_ragged<32>(a, s);
  } else {
    switch (K) {
#define SVAE_CASE(KK) case KK: svae::launch_sample_row_ragged<KK>(a, s); break;
      SVAE_CASE(1) SVAE_CASE(2) SVAE_CASE(3) SVAE_CASE(4) SVAE_CASE(5) SVAE_CASE(6) SVAE_CASE(7)
      SVAE_CASE(8) SVAE_CASE(9) SVAE_CASE(10) SVAE_CASE(11) SVAE_CASE(12) SVAE_CASE(13)
      SVAE_CASE(14) SVAE_CASE(15) SVAE_CASE(16)
#undef SVAE_CASE
    }
  }
  return hipGetLastError() == hipSuccess ? 0 : -1000;
}
