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

#include "hmm_perstep_kernel.hpp"    // HmmPerstepArgs and the kernel template; this unit instantiates the E-step (FILTER = false)

namespace svae {

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
  if (const int rc = svae::hmm_check_model(B, T, K, pair_batched, init_params, pair_params, true)) return rc;
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
  svae::hmm_set_model(a, B, T, K, pair_batched ? (long)(T - 1) * K * K : 0, init_params, pair_params, node_params);
  a.lengths = lengths;
  a.logZ = logZ; a.E_init = E_init; a.E_trans = E_trans; a.E_states = E_states; a.info = info;
  a.ws = (double*)workspace;
  hipStream_t s = (hipStream_t)stream;
  svae::hmm_dispatch_group(K, [&](auto g, auto w) { svae::launch_perstep<g, w>(a, s); });
  return hipGetLastError() == hipSuccess ? 0 : -1000;
}
