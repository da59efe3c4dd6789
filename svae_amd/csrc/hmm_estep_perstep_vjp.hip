// hmm_estep_perstep_vjp.hip -- reverse-mode derivative of the HMM E-step with PER-STEP transition potentials for MI355X
// (gfx950), K <= 64: svae_hmm_perstep_estep_vjp_f64 / svae_hmm_perstep_estep_vjp_workspace_bytes (include/svae_hip.h;
// DESIGN 4.5i).  The arithmetic of hmm_estep_vjp.hip with the step's own matrices P_t and the step's own
// cotangent V_t, in log space throughout like hmm_estep_perstep.hip: ONE route, no flags, no second launch.
//
// The statistics are the gradient of log Z, so their Jacobian is the Hessian of log Z: the posterior covariance of the
// sufficient statistics.  For cotangents g (of logZ), u0 (of E_init), V_t (of E_trans[t]) and W (of E_states) put
//   phi(z) = u0[z_0] + sum_t V_t[z_t, z_{t+1}] + sum_t W[t, z_t];   then, for one sequence of length L,
//   forward   la_0 = init + node_0                         r_0 = u0 + W[0]
//             w_t[j,k] = softmax_j(la_t[j] + P_t[j,k])     (0 where the column is all -inf)
//             la_{t+1}[k] = node_{t+1}[k] + lse_j(la_t[j] + P_t[j,k])
//             r_{t+1}[k]  = sum_j w_t[j,k] (r_t[j] + V_t[j,k]) + W[t+1,k]             (= E[phi up to t+1 | z_{t+1} = k])
//   end       logZ = lse_k la_{L-1};  gamma_{L-1} = exp(la_{L-1} - logZ);  E[phi] = sum_k gamma_{L-1}[k] r_{L-1}[k];  c = g - E[phi]
//   backward  lb_{L-1} = 0, s_{L-1} = 0;   y_{t+1} = W[t+1] + s_{t+1}
//             q_t[j,k] = softmax_k(P_t[j,k] + node_{t+1}[k] + lb_{t+1}[k])              (0 where the row is all -inf)
//             lb_t[j] = lse_k(...),   s_t[j] = sum_k q_t[j,k] (V_t[j,k] + y_{t+1}[k]),   gamma_t = exp(la_t + lb_t - logZ)
//             d_pair[t,j,k] = gamma_t[j] q_t[j,k] (c + r_t[j] + V_t[j,k] + y_{t+1}[k])
//             d_node[t,k]   = gamma_t[k] (c + r_t[k] + s_t[k]),      d_init = d_node[0]
// The softmax weights are the two sweeps' own exponentials -- 2 K^2 exp per step, as in the E-step, no third set.  r and s
// are conditional expectations of partial sums of phi, bounded by L max|cotangent|: they need no scaling.  A -inf entry
// has weight exactly 0 and so d_pair exactly 0 (r and s stay finite by the 0-weight convention: never 0 * inf); an all
// -inf row or column is handled by "the shift of an empty maximum is 0".
//
// Mapping (that of hmm_estep_perstep.hip): a group of G = 8, 16, 32 or 64 lanes per sequence, lane = state, 64 / G
// sequences per workgroup of W wavefronts, W = 1 for K <= 16 and W = 4 above, each wavefront taking a quarter of every
// reduction; the partial (maximum, sum, weighted sum) triples meet in LDS and are combined with the same exp(m_w - M).
// Per group in LDS, 2 K KS + 2 K + 4 W K doubles (KS = K | 1), sized at compile time for K = G:
//   the e tile K x KS, the V tile K x KS, two broadcast vectors, and per wavefront row factors and the partial triples
//   G = 64: 75776 bytes (74 KiB: two workgroups per CU);  G = 32: 43008;  G = 16: 20480;  G = 8: 12288.
//   forward  lane k reads column k of P_t and of V_t from memory (coalesced), keeps la_t[j] + P_t[j,k] in its tile column
//            between the maximum pass and the exponential pass, and accumulates sum_j e_j (r_t[j] + V_t[j,k]) beside the
//            sum; the record of the step is [la_t | r_t].
//   backward P_t and V_t go into their tiles (coalesced), lane j reduces row j, accumulating sum_k e_jk (V_t[j,k] + y[k])
//            beside the sum and overwriting the row with e_jk; then lane k writes column k of d_pair from the e tile, the
//            V tile, the row factors gamma_j / S_j exp(m_w - M_j) and c + r_t[j], which replaces y in its broadcast vector
//            once every wavefront is done with y: full-width coalesced stores.
// g_trans == NULL: V_t is not loaded in either sweep and the V tile is not touched.  d_pair == NULL: the e tile is not
// written back and the store pass is skipped; d_init and d_node do not change a bit.
// Workspace: [la_t | r_t], (B,T,2K) doubles, written by the forward sweep (first wavefront), read back behind barriers.
// Lengths: as hmm_estep_perstep.hip; d_node[b, L:] and d_pair[b, L-1:] are stored as 0.0; nothing at node / g_states steps
// >= L or pair / g_trans steps >= L-1 is loaded.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "../../include/svae_hip.h"

#include "hmm_perstep_vjp_kernel.hpp"

namespace svae {

template <int G, int W>
static void launch_perstep_vjp(const HmmPerstepVjpArgs& a, hipStream_t s) {
  constexpr int SPB = 64 / G;
  hipLaunchKernelGGL((hmm_perstep_vjp_kernel<G, W>), dim3((unsigned)((a.B + SPB - 1) / SPB)), dim3(64 * W), 0, s, a);
}

}  // namespace svae

extern "C" size_t svae_hmm_perstep_estep_vjp_workspace_bytes(int B, int T, int K) {
  if (B <= 0 || T <= 0 || K < 1 || K > SVAE_HMM_MAX_K) return 0;
  const size_t bytes = (size_t)B * T * 2 * K * sizeof(double);
  return (bytes + 127) & ~(size_t)127;
}

extern "C" int svae_hmm_perstep_estep_vjp_f64(int B, int T, int K, int pair_batched,
                                              const double* init_params, const double* pair_params,
                                              const double* node_params, const int32_t* lengths,
                                              const double* g_logZ, const double* g_init, const double* g_trans,
                                              const double* g_states, double* d_init, double* d_pair, double* d_node,
                                              int32_t* info, void* workspace, size_t ws_bytes, void* stream) {
  if (const int rc = svae::hmm_check_model(B, T, K, pair_batched, init_params, pair_params, true)) return rc;
  if (B == 0) return 0;
  if (!node_params) return -7;
  if (!d_init) return -8;
  if (!d_node) return -9;
  if (lengths && !info) return -10;
  if (!workspace) return -11;
  if (ws_bytes < svae_hmm_perstep_estep_vjp_workspace_bytes(B, T, K)) return -12;
  if (((uintptr_t)workspace & 15) != 0) return -13;
  svae::HmmPerstepVjpArgs a;
  svae::hmm_set_model(a, B, T, K, pair_batched ? (long)(T - 1) * K * K : 0, init_params, pair_params, node_params);
  a.lengths = lengths;
  a.g_logZ = g_logZ; a.g_init = g_init; a.g_trans = T > 1 ? g_trans : nullptr; a.g_states = g_states;
  a.d_init = d_init; a.d_pair = T > 1 ? d_pair : nullptr; a.d_node = d_node; a.info = info;
  a.ws = (double*)workspace;
  hipStream_t s = (hipStream_t)stream;
  svae::hmm_dispatch_group(K, [&](auto g, auto w) { svae::launch_perstep_vjp<g, w>(a, s); });
  return hipGetLastError() == hipSuccess ? 0 : -1000;
}
