// lds_units.hpp -- host side of the register-path LDS ABI (1 <= n <= SVAE_LDS_MAX_N = 15): what a per-latent-dimension
// unit offers the C-ABI dispatchers, and the argument fill and pointer checks the E-step-like entry points share.
// Every per-n unit defines ONE table of launch functions (extern "C" const, named by its SVAE_N); a dispatcher names the
// fifteen dimensions once (SVAE_LDS_NS), keeps a `const Unit* const [16]` and calls units[n]->entry(...).
#pragma once
#include <stdint.h>

#include "lds_args.hpp"

// the latent dimensions that have units: X(1) X(2) ... X(15)
#define SVAE_LDS_NS(X) X(1) X(2) X(3) X(4) X(5) X(6) X(7) X(8) X(9) X(10) X(11) X(12) X(13) X(14) X(15)

namespace svae {

// lds_estep_n.hip (svae_lds_estep_unit_n<N>).  Every entry returns 0, -1000 (launch error) or -1001 (LDS grant refused).
// Entries marked TE / LEAN exist for n <= TE_MAX_N / LEAN_MAX_N only: in the other units they return -3, and the
// dispatchers reach them behind the same range tests as the kernels' own headers.
struct EstepUnit {
  int (*estep)(const LdsArgs&, int inhomog, void* stream);                       // packed: four sequences per wavefront
  int (*estep_split)(const LdsArgs&, int inhomog, void* stream);                 // one sequence per wavefront
  // TE.  layout: 0 = by batch size (one sequence per wavefront below TE_RPC_MIN_B, two per wavefront from there), 1 = one
  // sequence per wavefront, 2 = two per wavefront (row-per-chain kernel; homogeneous lean launches without the
  // cross-moment hand-off)
  int (*twoend)(const LdsArgs&, int inhomog, int lean, int layout, void* stream);
  int (*twoend_mix)(const LdsArgs&, void* stream);                               // TE.  SLDS mean-field step, K sets as LDS tables
  // TE.  the SLDS mean-field step in the row-per-chain layout with producer wavefronts (refprod != 0: reference producers)
  int (*slds_rpc)(const LdsArgs&, int refprod, int seq_ok, void* stream);
  int (*forward_pair)(const LdsArgs& filter, const LdsArgs& estep, int inhomog, void* stream);   // TE.  both in one launch
  int (*filter)(const LdsArgs&, int inhomog, void* stream);                      // packed
  int (*filter_split)(const LdsArgs&, int inhomog, void* stream);
  int (*filter_1r)(const LdsArgs&, int inhomog, void* stream);                   // TE.  one-register filter
  int (*sample)(const SampleArgs&, void* stream);
  // LEAN.  E-step + sampler in one launch on lean records (lds_lean_estep.hpp): homogeneous pair parameters
  int (*infer_lean)(const LdsArgs&, const LeanSample&, int inhomog, void* stream);
  // per-sequence lengths (svae_lds_ragged_*): the packed E-step and samplers in their ragged instantiations ...
  int (*ragged)(const LdsArgs&, void* stream);
  int (*sample_ragged)(const SampleArgs&, void* stream);
  // ... with per-step pair parameters and an optional per-sequence init potential (svae_lds_ragged_perstep_*)
  int (*ragged_perstep)(const LdsPerstepArgs&, void* stream);
};

// lds_vjp_n.hip (svae_lds_vjp_unit_n<N>)
struct VjpUnit {
  int (*vjp)(const VjpArgs&, void* stream);
  int (*vjp_lean)(const VjpArgs&, void* stream);      // LEAN.  the two sweeps on the lean records of svae_lds_inference_f64
  int (*vjp_ragged)(const VjpArgs&, void* stream);    // svae_lds_ragged_vjp_f64: the packed sweeps, ragged instantiations
  // svae_lds_ragged_perstep_vjp_f64: the packed ragged sweeps on per-step pair parameters, statistics cotangents included
  int (*vjp_ragged_perstep)(const VjpPerstepArgs&, void* stream);
};

// ---- host helpers of the E-step-like entry points (lds_estep.hip, lds_estep_xl.hip) ---------------------------------
// The block every such entry supplies: sizes, model, outputs, info, workspace.  `a` arrives value-initialised (LdsArgs
// a{}): whatever an entry point does not set stays 0 / nullptr.
static inline void set_estep_args(LdsArgs& a, int B, int T, int n, int pair_batched,
                                  const double* init_J, const double* init_h, const double* init_logZ,
                                  const double* J11, const double* J12, const double* J22, const double* logZ_pair,
                                  const double* node_J, const double* node_h, const double* node_logZ,
                                  double* lognorm, double* E_init, double* E_pair, double* E_node_diagxx, double* E_node_x,
                                  int32_t* info, void* workspace) {
  a.B = B; a.T = T;
  a.init_J = init_J; a.init_h = init_h; a.init_logZ = init_logZ;
  a.J11 = J11; a.J12 = J12; a.J22 = J22; a.logZ_pair = logZ_pair;
  a.node_J = node_J; a.node_h = node_h; a.node_logZ = node_logZ;
  a.lognorm = lognorm; a.E_init = E_init; a.E_pair = E_pair;
  a.E_node_diagxx = E_node_diagxx; a.E_node_x = E_node_x;
  a.info = info; a.ws = (double*)workspace;
  a.pair_seq_stride = pair_batched ? (long)(T - 1) * n * n : 0;
}

// the model: -6 -7 -8, and -9 where the chain has a pair
static inline int check_model(const LdsArgs& a) {
  if (!a.init_J) return -6;
  if (!a.init_h) return -7;
  if (!a.init_logZ) return -8;
  if (a.T > 1 && (!a.J11 || !a.J12 || !a.J22 || !a.logZ_pair)) return -9;
  return 0;
}

// the per-sequence arrays of an E-step: -13 -14 (node potentials; node_logZ may be NULL), -16 .. -20 (statistics), -21.
// pair_stats = false: E_pair may be NULL (the (B,T-1,3,n,n) layout is empty at T = 1)
static inline int check_arrays(const LdsArgs& a, bool pair_stats = true) {
  if (!a.node_J) return -13;
  if (!a.node_h) return -14;
  if (!a.lognorm) return -16;
  if (!a.E_init) return -17;
  if (pair_stats && !a.E_pair) return -18;
  if (!a.E_node_diagxx) return -19;
  if (!a.E_node_x) return -20;
  if (!a.info) return -21;
  return 0;
}

}  // namespace svae
