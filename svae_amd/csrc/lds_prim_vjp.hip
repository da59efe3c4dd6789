// lds_prim_vjp.hip -- C ABI of the three reverse-mode primitives (include/svae_hip.h, ABI 15): argument checks, then the
// per-latent-dimension units of lds_prim_vjp_n.hip.  No allocation, no host synchronisation.
#include <cstdint>
#include "lds_prim_vjp.hpp"
#include "lds_units.hpp"
#include "../../include/svae_hip.h"

// the per-n units (lds_prim_vjp_n.hip: one launch function each, `which` = 0 filter, 1 smoother, 2 sampler VJP)
typedef int (*PrimUnit)(int which, const svae::PrimArgs*, void* stream);
#define SVAE_DECL(NN) extern "C" int svae_lds_prim_vjp_n##NN(int, const svae::PrimArgs*, void*);
SVAE_LDS_NS(SVAE_DECL)
#undef SVAE_DECL
#define SVAE_UNIT(NN) svae_lds_prim_vjp_n##NN,
static const PrimUnit prim_units[SVAE_LDS_MAX_N + 1] = {nullptr, SVAE_LDS_NS(SVAE_UNIT)};
#undef SVAE_UNIT

// (prim_common has checked 1 <= n <= SVAE_LDS_MAX_N)
static int prim_dispatch(int which, int n, const svae::PrimArgs* a, void* stream) {
  if (a->B == 0) return 0;
  return prim_units[n](which, a, stream);
}

static int prim_common(int B, int T, int n, int inhomog, int pair_batched, svae::PrimArgs* a) {
  if (B < 0) return -1;
  if (T < 1) return -2;
  if (n < 1 || n > SVAE_LDS_MAX_N) return -3;
  if (pair_batched && !inhomog) return -7;
  *a = svae::PrimArgs{};
  a->B = B; a->T = T;
  a->pair_t_stride = inhomog ? (long)n * n : 0;
  a->pair_seq_stride = pair_batched ? (long)(T - 1) * n * n : 0;
  return 0;
}

extern "C" size_t svae_lds_smoother_vjp_workspace_bytes(int B, int T, int n) {
  if (B <= 0 || T <= 0 || n <= 0 || n > SVAE_LDS_MAX_N) return 0;
  return (size_t)B * T * svae::prim_smoother_step_doubles(n) * sizeof(double);
}

extern "C" int svae_lds_filter_vjp_f64(int B, int T, int n, int inhomog, int pair_batched,
                                       const double* J11, const double* J12,
                                       const double* J_filt, const double* h_filt,
                                       const double* g_J_pred, const double* g_h_pred,
                                       const double* g_J_filt, const double* g_h_filt, const double* g_lognorm,
                                       double* g_node_J, double* g_node_h, double* g_node_logZ,
                                       int32_t* info, void* stream) {
  svae::PrimArgs a;
  const int rc = prim_common(B, T, n, inhomog, pair_batched, &a);
  if (rc) return rc;
  if (T > 1 && (!J11 || !J12)) return -5;
  if (!J_filt || !h_filt) return -6;
  if (!g_J_pred || !g_h_pred || !g_J_filt || !g_h_filt || !g_lognorm) return -8;
  if (!g_node_J || !g_node_h || !g_node_logZ) return -9;
  a.J11 = J11; a.J12 = J12; a.Jf = J_filt; a.hf = h_filt;
  a.gJp = g_J_pred; a.ghp = g_h_pred; a.gJf = g_J_filt; a.ghf = g_h_filt; a.g_lognorm = g_lognorm;
  a.g_node_J = g_node_J; a.g_node_h = g_node_h; a.g_node_logZ = g_node_logZ; a.info = info;
  return prim_dispatch(0, n, &a, stream);
}

extern "C" int svae_lds_smoother_vjp_f64(int B, int T, int n, int inhomog, int pair_batched,
                                         const double* J11, const double* J12, const double* J22,
                                         const double* J_pred, const double* h_pred,
                                         const double* J_filt, const double* h_filt,
                                         const double* g_E_init, const double* g_E_pair,
                                         const double* g_E_node_diagxx, const double* g_E_node_x,
                                         double* g_J_pred, double* g_h_pred, double* g_J_filt, double* g_h_filt,
                                         int32_t* info, void* workspace, size_t ws_bytes, void* stream) {
  svae::PrimArgs a;
  const int rc = prim_common(B, T, n, inhomog, pair_batched, &a);
  if (rc) return rc;
  if (T > 1 && (!J11 || !J12 || !J22)) return -5;
  if (!J_pred || !h_pred || !J_filt || !h_filt) return -6;
  if (!g_J_pred || !g_h_pred || !g_J_filt || !g_h_filt) return -9;
  if (B > 0 && (!workspace || ws_bytes < svae_lds_smoother_vjp_workspace_bytes(B, T, n))) return -14;
  a.J11 = J11; a.J12 = J12; a.J22 = J22; a.Jp = J_pred; a.hp = h_pred; a.Jf = J_filt; a.hf = h_filt;
  a.g_E_init = g_E_init; a.g_E_pair = T > 1 ? g_E_pair : nullptr; a.g_dxx = g_E_node_diagxx; a.g_x = g_E_node_x;
  a.g_pair_per_step = inhomog;
  a.oJp = g_J_pred; a.ohp = g_h_pred; a.oJf = g_J_filt; a.ohf = g_h_filt;
  a.ws = (double*)workspace; a.info = info;
  return prim_dispatch(1, n, &a, stream);
}

extern "C" int svae_lds_sample_vjp_f64(int B, int T, int n, int S, int inhomog, int pair_batched,
                                       const double* J11, const double* J12,
                                       const double* J_filt, const double* h_filt,
                                       const double* eps, const double* samples, const double* g_samples,
                                       double* g_J_pred, double* g_h_pred, double* g_J_filt, double* g_h_filt,
                                       int32_t* info, void* stream) {
  svae::PrimArgs a;
  const int rc = prim_common(B, T, n, inhomog, pair_batched, &a);
  if (rc) return rc;
  if (S < 1 || S > 16) return -4;
  if (T > 1 && (!J11 || !J12)) return -5;
  if (!J_filt || !h_filt) return -6;
  if (!eps || !samples || !g_samples) return -8;
  if (!g_J_pred || !g_h_pred || !g_J_filt || !g_h_filt) return -9;
  a.S = S; a.J11 = J11; a.J12 = J12; a.Jf = J_filt; a.hf = h_filt;
  a.eps = eps; a.samples = samples; a.g_samples = g_samples;
  a.oJp = g_J_pred; a.ohp = g_h_pred; a.oJf = g_J_filt; a.ohf = g_h_filt; a.info = info;
  return prim_dispatch(2, n, &a, stream);
}
