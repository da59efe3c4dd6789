// hmm_estep_vjp_ragged.hip -- the derivative of the HMM E-step with PER-SEQUENCE LENGTHS for MI355X (gfx950): the RAGGED
// instantiations of the kernel templates of hmm_estep_vjp_kernel.hpp and their entry point
// svae_hmm_ragged_estep_vjp_f64 (include/svae_hip.h).  One padded (B, T, K) batch, sequence b differentiated as if cut
// to its own L = lengths[b] steps under the arithmetic hmm_estep_vjp.hip defines: nothing stored at t >= L is read, in
// the potentials or in the cotangents, and g_node[b, L:] is exactly 0.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/svae_hip.h"
#include "dpp.hpp"
#include "hmm_estep_vjp_kernel.hpp"

namespace svae {

template <int K>
static void launch_vjp_row_ragged(const VjpRaggedArgs& a, hipStream_t s) {
  hipLaunchKernelGGL((hmm_vjp_row_kernel<K, true>), dim3((a.B + 3) / 4), dim3(64), 0, s, a);
}
template <int KP>
static void launch_vjp_wide_ragged(const VjpRaggedArgs& a, hipStream_t s) {
  if constexpr (KP > 16) hipLaunchKernelGGL((hmm_vjp_wide_kernel<KP, false, true>), dim3(a.B), dim3(64), 0, s, a);
  hipLaunchKernelGGL((hmm_vjp_wide_kernel<KP, true, true>), dim3(a.B), dim3(64), 0, s, a);
}

}  // namespace svae

extern "C" int svae_hmm_ragged_estep_vjp_f64(int B, int T, int K, int pair_batched,
                                             const double* init_params, const double* pair_params,
                                             const double* node_params, const int32_t* lengths,
                                             const double* g_logZ, const double* g_init, const double* g_trans,
                                             const double* g_states,
                                             double* d_init, double* d_pair, double* d_node,
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
  if (!d_init) return -9;
  if (!d_pair) return -10;
  if (!d_node) return -11;
  if (!info) return -12;
  if (!workspace) return -13;
  if (ws_bytes < svae_hmm_estep_vjp_workspace_bytes(B, T, K)) return -14;
  if (((uintptr_t)workspace & 15) != 0) return -15;
  svae::VjpRaggedArgs a;
  a.B = B; a.T = T; a.K = K; a.pair_stride = pair_batched ? (long)K * K : 0;
  a.init_params = init_params; a.pair_params = pair_params; a.node_params = node_params;
  a.g_logZ = g_logZ; a.g_init = g_init; a.g_trans = g_trans; a.g_states = g_states;
  a.d_init = d_init; a.d_pair = d_pair; a.d_node = d_node; a.ws = (double*)workspace;
  a.lengths = lengths; a.info = info;
  hipStream_t s = (hipStream_t)stream;
  if (K > 32) {
    svae::launch_vjp_wide_ragged<64>(a, s);
  } else if (K > 16) {
    svae::launch_vjp_wide_ragged<32>(a, s);
  } else {
    switch (K) {
#define SVAE_CASE(KK) case KK: svae::launch_vjp_row_ragged<KK>(a, s); break;
      SVAE_CASE(1) SVAE_CASE(2) SVAE_CASE(3) SVAE_CASE(4) SVAE_CASE(5) SVAE_CASE(6) SVAE_CASE(7)
      SVAE_CASE(8) SVAE_CASE(9) SVAE_CASE(10) SVAE_CASE(11) SVAE_CASE(12) SVAE_CASE(13)
      SVAE_CASE(14) SVAE_CASE(15) SVAE_CASE(16)
#undef SVAE_CASE
    }
    svae::launch_vjp_wide_ragged<16>(a, s);
  }
  return hipGetLastError() == hipSuccess ? 0 : -1000;
}
