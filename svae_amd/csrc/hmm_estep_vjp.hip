// hmm_estep_vjp.hip -- reverse-mode derivative of the batched HMM E-step for MI355X (gfx950), 1 <= K <= 64: the
// cotangents of all four outputs (logZ, E_init, E_trans, E_states) pulled back to all three inputs (init, pair and node
// log-potentials).  [The reference differentiates log Z alone (svae/hmm/cython_hmm_inference.pyx:126-166); the statistics
// are that gradient, so this is the Hessian-vector product of log Z -- the arithmetic is DEFINED here.]
//
// The statistics are grad log Z; their Jacobian is the Hessian of log Z = the posterior covariance of the sufficient
// statistics.  For cotangents g (of logZ), u0 (of E_init, K), V (of E_trans, K x K) and W (of E_states, T x K) put
//   phi(z) = u0[z_0] + sum_t V[z_t, z_{t+1}] + sum_t W[t, z_t].
// Then, with gamma_t the state marginals and xi_t the pair marginals,
//   g_node[t,k] = gamma_t[k] (g + E[phi | z_t = k] - E[phi])
//   g_init      = g_node[0]
//   g_pair[i,j] = sum_t xi_t[i,j] (g + E[phi | z_t = i, z_{t+1} = j] - E[phi]).
// The conditional expectations come from two extra K-vectors per step next to the usual messages a_t (filtered
// distribution) and b_t (backward message):
//   forward   r_0 = u0 + W[0];   r_t[j] = sum_i w_t[i,j] (r_{t-1}[i] + V[i,j]) + W[t,j],
//             w_t[i,j] ~ a_{t-1}[i] exp(pair[i,j]) normalised over i (the sampler's backward-draw weights);
//             a state with no incoming mass has r = W[t,j] (any finite value would do: its marginal is 0)
//   backward  s_{T-1} = 0;       s_t[i] = sum_j q_t[i,j] (V[i,j] + W[t+1,j] + s_{t+1}[j]),
//             q_t[i,j] ~ exp(pair[i,j] + node[t+1,j]) b_{t+1}[j] normalised over j; no mass ahead: s = 0
//   E[phi | z_t = k]                = r_t[k] + s_t[k]
//   E[phi | z_t = i, z_{t+1} = j]   = r_t[i] + V[i,j] + W[t+1,j] + s_{t+1}[j]
//   E[phi]                          = sum_k gamma_{T-1}[k] r_{T-1}[k].
// r and s are conditional expectations, bounded by T max|cotangent|: they need no scaling and have no range problem of
// their own; only the weights do.  A -inf potential has gradient exactly 0 and a finite cotangent at a position of
// probability 0 contributes exactly 0 (the weight is an exact 0, the bracket stays finite).  A sequence with
// log Z = -inf is outside the contract, as for the E-step.
//
// One entry = two launches (hmm_estep_vjp_kernel.hpp): the scaled kernels (K <= 16: one DPP row per sequence, four per
// wavefront; 17 .. 64: one wavefront per sequence, KP = 32 or 64), each a forward and a backward sweep, and behind them
// the log-space kernel, at work only on the sequences whose route flag the scaled launch raised (the E-step's range
// criterion, hmm_args.hpp).  The flags stay in the workspace, behind the records, as doubles (1.0 = redone).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/svae_hip.h"
#include "dpp.hpp"
#include "hmm_estep_vjp_kernel.hpp"   // the kernel templates and their launch; this unit instantiates RAGGED = false

extern "C" size_t svae_hmm_estep_vjp_workspace_bytes(int B, int T, int K) {
  if (B <= 0 || T <= 0 || K <= 0 || K > SVAE_HMM_MAX_K) return 0;
  return (svae::vjp_ws_doubles(B, T, K) * sizeof(double) + 127) & ~(size_t)127;
}

extern "C" int svae_hmm_estep_vjp_f64(int B, int T, int K, int pair_batched,
                                      const double* init_params, const double* pair_params,
                                      const double* node_params,
                                      const double* g_logZ, const double* g_init, const double* g_trans,
                                      const double* g_states,
                                      double* d_init, double* d_pair, double* d_node,
                                      void* workspace, size_t ws_bytes, void* stream) {
  if (const int rc = svae::hmm_check_model(B, T, K, pair_batched, init_params, pair_params)) return rc;
  if (B == 0) return 0;
  if (!node_params) return -7;
  if (!d_init) return -8;
  if (!d_pair) return -9;
  if (!d_node) return -10;
  if (!workspace) return -11;
  if (ws_bytes < svae_hmm_estep_vjp_workspace_bytes(B, T, K)) return -12;
  if (((uintptr_t)workspace & 15) != 0) return -13;
  svae::VjpArgs a;
  svae::hmm_set_model(a, B, T, K, pair_batched ? (long)K * K : 0, init_params, pair_params, node_params);
  a.g_logZ = g_logZ; a.g_init = g_init; a.g_trans = g_trans; a.g_states = g_states;
  a.d_init = d_init; a.d_pair = d_pair; a.d_node = d_node; a.ws = (double*)workspace;
  return svae::launch_vjp<false>(a, (hipStream_t)stream);
}
