// hmm_sample_ragged.hip -- batched HMM posterior sampling with PER-SEQUENCE LENGTHS for MI355X (gfx950): the RAGGED
// instantiations of the four kernel templates of hmm_sample_kernel.hpp (filter and draw, row K = 1 .. 16, wide KP = 32 and
// 64) and their entry point svae_hmm_ragged_sample_f64 (include/svae_hip.h).  One padded (B, T, K) batch, sequence b
// sampled as if cut to its own L = lengths[b] steps under the arithmetic hmm_sample.hip defines: states[b, :, :L] and
// logZ[b] are those of the cut sequence, states[b, :, L:] = -1, and neither node_params[b, L:] nor u[b, :, L:] is read.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/svae_hip.h"
#include "dpp.hpp"
#include "hmm_sample_kernel.hpp"      // the four kernel templates and their launch; this unit instantiates RAGGED = true

extern "C" int svae_hmm_ragged_sample_f64(int B, int T, int K, int S, int pair_batched,
                                          const double* init_params, const double* pair_params,
                                          const double* node_params, const int32_t* lengths, const double* u,
                                          int32_t* states, double* logZ,
                                          int32_t* info, void* workspace, size_t ws_bytes, void* stream) {
  if (const int rc = svae::hmm_check_model(B, T, K, pair_batched, init_params, pair_params)) return rc;
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
  svae::hmm_set_model(a, B, T, K, pair_batched ? (long)K * K : 0, init_params, pair_params, node_params);
  a.S = S; a.u = u; a.states = states; a.logZ = logZ; a.ws = (double*)workspace;
  a.lengths = lengths; a.info = info;
  return svae::launch_sample<true>(a, (hipStream_t)stream);
}
