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
#include "hmm_viterbi_kernel.hpp"     // the two kernel templates and their launch; this unit instantiates RAGGED = true

extern "C" int svae_hmm_ragged_viterbi_f64(int B, int T, int K, int pair_batched,
                                           const double* init_params, const double* pair_params,
                                           const double* node_params, const int32_t* lengths,
                                           int32_t* states, double* score,
                                           int32_t* info, void* workspace, size_t ws_bytes, void* stream) {
  if (const int rc = svae::hmm_check_model(B, T, K, pair_batched, init_params, pair_params)) return rc;
  if (B == 0) return 0;
  if (!node_params) return -7;
  if (!lengths) return -8;
  if (!states) return -9;
  if (!info) return -10;
  if (!workspace) return -11;
  if (ws_bytes < svae_hmm_viterbi_workspace_bytes(B, T, K)) return -12;
  if (((uintptr_t)workspace & 15) != 0) return -13;   // back-pointer rows are read back 16 bytes at a time
  svae::ViterbiRaggedArgs a;
  svae::hmm_set_model(a, B, T, K, pair_batched ? (long)K * K : 0, init_params, pair_params, node_params);
  a.states = states; a.score = score; a.ws = (uint8_t*)workspace;
  a.lengths = lengths; a.info = info;
  return svae::launch_viterbi<true>(a, (hipStream_t)stream);
}
