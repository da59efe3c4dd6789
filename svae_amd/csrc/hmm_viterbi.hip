// hmm_viterbi.hip -- batched HMM Viterbi decoding (most probable state path and its score) for MI355X (gfx950).
//
// What it replaces (reference = mattjj/svae): hmm_viterbi of svae/hmm/hmm_inference.py:54-63, which delegates to the
// un-vendored pyhsmm; parity with it is unpinned, so the arithmetic is DEFINED here, exactly (include/svae_hip.h):
//   delta_0[k] = init[k] + node[0][k];   delta_t[k] = (max_j (delta_{t-1}[j] + pair[j][k])) + node[t][k]
//   psi_t[k] = the LOWEST j attaining the maximum;   z_{T-1} = the lowest k attaining max_k delta_{T-1}[k];
//   z_t = psi_{t+1}[z_{t+1}];   score = delta_{T-1}[z_{T-1}]
// fp64 additions in that order and strict `>` compares only: no multiply, so no FMA can arise, and a NumPy restatement
// in the same order reproduces labels and score bit for bit (tests/_hmm_viterbi_numpy.py).  -inf entries are ordinary
// values here (-inf + -inf = -inf, never greater than anything); NaN inputs lose every compare: unspecified labels in
// 0..K-1, no fault.  The unit must be built without fast-math.
//
// Two mappings, as the E-step's (hmm_estep.hip, hmm_estep_wide.hip):
//   K <= 16      one 16-lane DPP row per sequence, four sequences per wavefront, lane k = state k.  Column k of the
//                transition matrix in registers (K doubles); delta_{t-1}[j] reaches the row as row_newbcast:j (dpp.hpp
//                bcast<j>: compiler-scheduled, hazards padded by hipcc).  A step is K (broadcast, add, compare, select).
//   17 .. 64     one wavefront per sequence, lane = state, KP = 32 or 64 padded states that carry -inf and can never
//                win a strict compare.  Column in registers (KP doubles); delta_{t-1} published through an LDS line
//                and read back as wave-uniform loads.  The running maximum is kept in two halves [0, KP/2), [KP/2, KP)
//                (two independent chains) merged with a strict compare, which keeps the lowest index.
// Node potentials are loaded a block of steps ahead of their use (a step is shorter than a trip to HBM).
//
// Back-pointers: one byte per (step, state) in the caller's workspace, KP bytes per step (KP = 16, 32, 64).
// Backtrace (T dependent look-ups, kept off the HBM latency):
//   K <= 16      16 steps at a time: lane l of the row loads the 16 bytes of step t0 + l (one coalesced 256-byte read
//                per row, the next block's issued before the current one is chased) and packs them into a 64-bit map
//                of 16 nibbles; the chase is then row_newbcast:l of that map, a shift and a mask per step -- registers
//                only.  Lane l keeps the label of its step: 16 labels leave as one 64-byte vector store.
//   17 .. 64     64 steps at a time staged through LDS (64 KP bytes, next block's loads in flight during the chase);
//                the chase reads one LDS byte per step; lane l keeps the label of step t0 + l: one 256-byte store.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/svae_hip.h"
#include "dpp.hpp"
#include "hmm_viterbi_kernel.hpp"     // the two kernel templates and their launch; this unit instantiates RAGGED = false

extern "C" size_t svae_hmm_viterbi_workspace_bytes(int B, int T, int K) {
  if (B <= 0 || T <= 0 || K <= 0 || K > SVAE_HMM_MAX_K) return 0;
  const size_t bytes = (size_t)B * T * svae::hmm_kp(K);
  return (bytes + 7) & ~(size_t)7;
}

extern "C" int svae_hmm_viterbi_f64(int B, int T, int K, int pair_batched,
                                    const double* init_params, const double* pair_params,
                                    const double* node_params, int32_t* states, double* score,
                                    void* workspace, size_t ws_bytes, void* stream) {
  if (const int rc = svae::hmm_check_model(B, T, K, pair_batched, init_params, pair_params)) return rc;
  if (B == 0) return 0;
  if (!node_params) return -7;
  if (!states) return -8;
  if (!workspace) return -10;
  if (ws_bytes < svae_hmm_viterbi_workspace_bytes(B, T, K)) return -11;
  if (((uintptr_t)workspace & 15) != 0) return -12;   // back-pointer rows are read back 16 bytes at a time
  svae::ViterbiArgs a;
  svae::hmm_set_model(a, B, T, K, pair_batched ? (long)K * K : 0, init_params, pair_params, node_params);
  a.states = states; a.score = score; a.ws = (uint8_t*)workspace;
  return svae::launch_viterbi<false>(a, (hipStream_t)stream);
}
