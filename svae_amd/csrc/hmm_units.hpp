// hmm_units.hpp -- host side of the HMM ABI (1 <= K <= SVAE_HMM_MAX_K = 64), the counterpart of lds_units.hpp: what every
// HMM entry point does before it comes to its own arguments.  The sixteen row sizes are named once (SVAE_HMM_ROW_KS); a
// unit hands hmm_dispatch_k its row launcher and its wide launcher as generic lambdas over std::integral_constant and
// hmm_dispatch_group the launcher of its lane groups; hmm_check_model and hmm_set_model are the checks and the argument
// fill that the entry points share.  Host code only: no kernel and no struct passed to one is defined here.
#pragma once
#include <stdint.h>

#include <type_traits>

#include "../../include/svae_hip.h"
#include "hmm_args.hpp"

// the numbers of states that have a DPP-row kernel of their own: X(1) X(2) ... X(16)
#define SVAE_HMM_ROW_KS(X) X(1) X(2) X(3) X(4) X(5) X(6) X(7) X(8) X(9) X(10) X(11) X(12) X(13) X(14) X(15) X(16)

namespace svae {

// K -> row(integral_constant<int, K>) for K <= 16, wide(integral_constant<int, KP>) with KP = 32 or 64 padded states
// above; -3 for a K outside 1 .. 64.  Both launchers return int.  What a unit launches behind its row kernel (the
// log-space redo of the E-step's derivative, say) belongs in its `row`.
template <class Row, class Wide>
static inline int hmm_dispatch_k(int K, Row&& row, Wide&& wide) {
  if (K > HMM_WIDE_MAX_K) return -3;
  if (K > 32) return wide(std::integral_constant<int, 64>{});
  if (K > 16) return wide(std::integral_constant<int, 32>{});
  switch (K) {
#define SVAE_HMM_ROW_CASE(KK) case KK: return row(std::integral_constant<int, KK>{});
    SVAE_HMM_ROW_KS(SVAE_HMM_ROW_CASE)
#undef SVAE_HMM_ROW_CASE
  }
  return -3;
}

// per-step units: K -> launch(integral_constant<int, G>, integral_constant<int, W>), G = hmm_perstep_group(K) lanes per
// sequence, W = hmm_perstep_waves(K) wavefronts per workgroup (hmm_args.hpp)
template <class Launch>
static inline void hmm_dispatch_group(int K, Launch&& launch) {
#define SVAE_HMM_GROUP_CASE(G) \
  case G: launch(std::integral_constant<int, G>{}, std::integral_constant<int, hmm_perstep_waves(G)>{}); break;
  switch (hmm_perstep_group(K)) { SVAE_HMM_GROUP_CASE(8) SVAE_HMM_GROUP_CASE(16) SVAE_HMM_GROUP_CASE(32) SVAE_HMM_GROUP_CASE(64) }
#undef SVAE_HMM_GROUP_CASE
}

// The checks every entry point opens with: -1 .. -6, else 0.  An entry returns 0 for B == 0 right behind them and goes on
// with codes of its own from -7.  pair_optional_at_T1: the per-step entries take pair_params == NULL where T == 1 (the
// (T-1,K,K) layout is empty).
static inline int hmm_check_model(int B, int T, int K, int pair_batched, const double* init_params,
                                  const double* pair_params, bool pair_optional_at_T1 = false) {
  if (B < 0) return -1;
  if (T < 1) return -2;
  if (K < 1 || K > SVAE_HMM_MAX_K) return -3;
  if (pair_batched != 0 && pair_batched != 1) return -4;
  if (!init_params) return -5;
  if (!pair_params && !(pair_optional_at_T1 && T == 1)) return -6;
  return 0;
}

// sizes and model of any of the args structs (they share these field names).  pair_stride: doubles between two
// sequences' pair parameters -- K K, or (T-1) K K per step -- where they are per sequence, else 0.
template <class Args>
static inline void hmm_set_model(Args& a, int B, int T, int K, long pair_stride, const double* init_params,
                                 const double* pair_params, const double* node_params) {
  a.B = B; a.T = T; a.K = K; a.pair_stride = pair_stride;
  a.init_params = init_params; a.pair_params = pair_params; a.node_params = node_params;
}

}  // namespace svae
