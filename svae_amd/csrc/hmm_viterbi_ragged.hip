// hmm_viterbi_ragged.hip -- batched HMM Viterbi decoding with PER-SEQUENCE LENGTHS for MI355X (gfx950): the RAGGED
// instantiations of the two kernel templates of hmm_viterbi_kernel.hpp (row K = 1 .. 16, wide KP = 32 and 64) and their
// entry point svae_hmm_ragged_viterbi_f64 (include/svae_hip.h).  One padded (B, T, K) batch, sequence b decoded as if cut
// to its own L = lengths[b] steps: states[b, :L] and score[b] under the exact arithmetic hmm_viterbi.hip defines (fp64
// adds in that order, strict compares, ties to the lowest index), states[b, L:] = -1, nothing stored at t >= L read.
// As hmm_viterbi.hip the unit holds no fp64 multiply and must be built without fast-math.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/svae_hip.h"
#include "dpp.hpp"
#include "hmm_viterbi_kernel.hpp"

namespace svae {

template <int K>
static int launch_viterbi_row_ragged(const ViterbiRaggedArgs& a, hipStream_t s) {
  hipLaunchKernelGGL((hmm_viterbi_row_kernel<K, true>), dim3((a.B + 3) / 4), dim3(64), 0, s, a);
  return hipGetLastError() == hipSuccess ? 0 : -1000;
}

}  // namespace svae

extern "C" int svae_hmm_ragged_viterbi_f64(int B, int T, int K, int pair_batched,
                                           const double* init_params, const double* pair_params,
                                           const double* node_params, const int32_t* lengths,
                                           int32_t* states, double* score,
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
  if (!states) return -9;
  if (!info) return -10;
  if (!workspace) return -11;
  if (ws_bytes < svae_hmm_viterbi_workspace_bytes(B, T, K)) return -12;
  if (((uintptr_t)workspace & 15) != 0) return -13;   // back-pointer rows are read back 16 bytes at a time
  svae::ViterbiRaggedArgs a;
  a.B = B; a.T = T; a.K = K; a.pair_stride = pair_batched ? (long)K * K : 0;
  a.init_params = init_params; a.pair_params = pair_params; a.node_params = node_params;
  a.states = states; a.score = score; a.ws = (uint8_t*)workspace;
  a.lengths = lengths; a.info = info;
  hipStream_t s = (hipStream_t)stream;
  if (K > 32) {
    hipLaunchKernelGGL((svae::hmm_viterbi_wide_kernel<64, true>), dim3(B), dim3(64), 0, s, a);
    return hipGetLastError() == hipSuccess ? 0 : -1000;
  }
  if (K > 16) {
    hipLaunchKernelGGL((svae::hmm_viterbi_wide_kernel<32, true>), dim3(B), dim3(64), 0, s, a);
    return hipGetLastError() == hipSuccess ? 0 : -1000;
  }
  switch (K) {
#define SVAE_CASE(KK) case KK: return svae::launch_viterbi_row_ragged<KK>(a, s);
    SVAE_CASE(1) SVAE_CASE(2) SVAE_CASE(3) SVAE_CASE(4) SVAE_CASE(5) SVAE_CASE(6) SVAE_CASE(7)
    SVAE_CASE(8) SVAE_CASE(9) SVAE_CASE(10) SVAE_CASE(11) SVAE_CASE(12) SVAE_CASE(13)
    SVAE_CASE(14) SVAE_CASE(15) SVAE_CASE(16)
#undef SVAE_CASE
  }
  return -3;
}
