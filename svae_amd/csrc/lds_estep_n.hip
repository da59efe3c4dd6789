// lds_estep_n.hip -- one translation unit per latent dimension (compiled with -DSVAE_N=<n>), so
// that `make -j` builds the 15 specialisations of the E-step kernel in parallel.
#if defined(SVAE_N) && SVAE_N > 13
// n = 14, 15: the tiles exceed 256 VGPRs and hipcc moves values through AGPRs (VALU writes the DPP
// hazard bookkeeping in dpp.hpp cannot see): make every DPP statement self-fenced (slower, safe).
#define SVAE_DPP_ALWAYS_FENCED 1
#endif
#include "lds_estep_kernel.hpp"
#include "lds_estep_split.hpp"
#include "lds_estep_twoend.hpp"
#include "lds_estep_twoend_rpc.hpp"
#include "lds_estep_twoend_rpcmix.hpp"
#include "lds_filter_1r.hpp"
#include "lds_lean_estep.hpp"
#include "lds_units.hpp"

#ifndef SVAE_N
#error "compile with -DSVAE_N=<latent dim>"
#endif
#define SVAE_CAT_(a, b) a##b
#define SVAE_CAT(a, b) SVAE_CAT_(a, b)

// The table's entries (lds_units.hpp says what each one is): file-local, reached only through svae_lds_estep_unit_n<N>.
static int estep(const svae::LdsArgs& a, int inhomog, void* stream) {
  return svae::launch_estep<SVAE_N>(a, inhomog != 0, (hipStream_t)stream);
}

static int sample(const svae::SampleArgs& a, void* stream) { return svae::launch_sample<SVAE_N>(a, (hipStream_t)stream); }

static int estep_split(const svae::LdsArgs& a, int inhomog, void* stream) {
  return svae::launch_estep_split<SVAE_N>(a, inhomog != 0, (hipStream_t)stream);
}

static int twoend(const svae::LdsArgs& a, int inhomog, int lean, int layout, void* stream) {
  const bool rpc_ok = !inhomog && lean && !a.ws3 && a.T >= svae::TE_MIN_T;
  if (rpc_ok && (layout == 2 || (layout == 0 && a.B >= svae::TE_RPC_MIN_B)))
    return svae::launch_estep_twoend_rpc<SVAE_N>(a, (hipStream_t)stream);
  return svae::launch_estep_twoend<SVAE_N>(a, inhomog != 0, lean != 0, (hipStream_t)stream);
}

static int twoend_mix(const svae::LdsArgs& a, void* stream) {
  return svae::launch_estep_twoend_mix<SVAE_N>(a, (hipStream_t)stream);
}

static int slds_rpc(const svae::LdsArgs& a, int refprod, int seq_ok, void* stream) {
  return svae::launch_slds_meanfield_rpc<SVAE_N>(a, refprod, seq_ok, (hipStream_t)stream);
}

static int filter(const svae::LdsArgs& a, int inhomog, void* stream) {
  return svae::launch_filter<SVAE_N>(a, inhomog != 0, (hipStream_t)stream);
}

static int filter_1r(const svae::LdsArgs& a, int inhomog, void* stream) {
  return svae::launch_filter_1r<SVAE_N>(a, inhomog != 0, (hipStream_t)stream);
}

static int forward_pair(const svae::LdsArgs& f, const svae::LdsArgs& e, int inhomog, void* stream) {
  return svae::launch_forward_pair<SVAE_N>(f, e, inhomog != 0, (hipStream_t)stream);
}

static int filter_split(const svae::LdsArgs& a, int inhomog, void* stream) {
  return svae::launch_filter_split<SVAE_N>(a, inhomog != 0, (hipStream_t)stream);
}

static int infer_lean(const svae::LdsArgs& a, const svae::LeanSample& ls, int inhomog, void* stream) {
  return svae::launch_infer_lean<SVAE_N>(a, ls, inhomog != 0, (hipStream_t)stream);
}

static int ragged(const svae::LdsArgs& a, void* stream) { return svae::launch_estep_ragged<SVAE_N>(a, (hipStream_t)stream); }

static int sample_ragged(const svae::SampleArgs& a, void* stream) {
  return svae::launch_sample_ragged<SVAE_N>(a, (hipStream_t)stream);
}

static int ragged_perstep(const svae::LdsPerstepArgs& a, void* stream) {
  return svae::launch_estep_ragged_perstep<SVAE_N>(a, (hipStream_t)stream);
}

#ifndef __HIP_DEVICE_COMPILE__   /* host data: a const table with a constant initialiser would be emitted for the device too */
extern "C" const svae::EstepUnit SVAE_CAT(svae_lds_estep_unit_n, SVAE_N) = {
  .estep = estep, .estep_split = estep_split, .twoend = twoend, .twoend_mix = twoend_mix, .slds_rpc = slds_rpc,
  .forward_pair = forward_pair, .filter = filter, .filter_split = filter_split, .filter_1r = filter_1r, .sample = sample,
  .infer_lean = infer_lean, .ragged = ragged, .sample_ragged = sample_ragged, .ragged_perstep = ragged_perstep,
};
#endif
