// hmm_estep_vjp_ragged.hip -- the derivative of the HMM E-step with PER-SEQUENCE LENGTHS for MI355X (gfx950): the RAGGED
// instantiations of the kernel templates of hmm_estep_vjp_kernel.hpp and their entry point
// svae_hmm_ragged_estep_vjp_f64 (include/svae_hip.h).  One padded (B, T, K) batch, sequence b differentiated as if cut
// to its own L = lengths[b] steps under the arithmetic hmm_estep_vjp.hip defines: nothing stored at t >= L is read, in
// the potentials or in the cotangents, and g_node[b, L:] is exactly 0.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/svae_hip.h"
#include "dpp.hpp"
#include "hmm_estep_vjp_kernel.hpp"   // the kernel templates and their launch; this unit instantiates RAGGED = true

extern "C" int svae_hmm_ragged_estep_vjp_f64(int B, int T, int K, int pair_batched,
                                             const double* init_params, const double* pair_params,
                                             const double* node_params, const int32_t* lengths,
                                             const double* g_logZ, const double* g_init, const double* g_trans,
                                             const double* g_states,
                                             double* d_init, double* d_pair, double* d_node,
                                             int32_t* info, void* workspace, size_t ws_bytes, void* stream) {
  if (const int rc = svae::hmm_check_model(B, T, K, pair_batched, init_params, pair_params)) return rc;
  if (B == 0) return 0;
  if (!node_params) return -7;
  if (!lengths) return -8;
  if (!d_init) return -9;
  if (!d_pair) return -10;
  if (!d_node) return -11;
  if (!info) return -12;
  if (!workspace) return -13;
  if (ws_bytes < svae_hmm_estep_vjp_workspace_bytes(B, T, K)) return -14;
  if (((uintptr_t)workspace & 15) != 0) return -15;
  svae::VjpRaggedArgs a;
  svae::hmm_set_model(a, B, T, K, pair_batched ? (long)K * K : 0, init_params, pair_params, node_params);
  a.g_logZ = g_logZ; a.g_init = g_init; a.g_trans = g_trans; a.g_states = g_states;
  a.d_init = d_init; a.d_pair = d_pair; a.d_node = d_node; a.ws = (double*)workspace;
  a.lengths = lengths; a.info = info;
  return svae::launch_vjp<true>(a, (hipStream_t)stream);
}
