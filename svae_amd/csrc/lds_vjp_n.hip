// lds_vjp_n.hip -- one translation unit per latent dimension (-DSVAE_N=<n>) for the VJP sweeps.
// DPP hazards are handled per product stage (one fence on the DPP-read operand array, dpp.hpp /
// lds_vjp_kernel.hpp) and checked on the generated ISA for every n by `make audit`;
// -DSVAE_DPP_ALWAYS_FENCED=1 falls back to a self-fenced build (every DPP statement carries its own
// wait states, about twice the instructions).
#ifndef SVAE_DPP_ALWAYS_FENCED
#define SVAE_DPP_ALWAYS_FENCED 0
#endif
#include "lds_vjp_kernel.hpp"
#include "lds_lean_vjp.hpp"
#include "lds_units.hpp"

#ifndef SVAE_N
#error "compile with -DSVAE_N=<latent dim>"
#endif
#define SVAE_CAT_(a, b) a##b
#define SVAE_CAT(a, b) SVAE_CAT_(a, b)

// The table's entries (lds_units.hpp says what each one is): file-local, reached only through svae_lds_vjp_unit_n<N>.
static int vjp(const svae::VjpArgs& a, void* stream) { return svae::launch_vjp<SVAE_N>(a, (hipStream_t)stream); }
static int vjp_lean(const svae::VjpArgs& a, void* stream) { return svae::launch_vjp_lean<SVAE_N>(a, (hipStream_t)stream); }
static int vjp_ragged(const svae::VjpArgs& a, void* stream) { return svae::launch_vjp_ragged<SVAE_N>(a, (hipStream_t)stream); }
static int vjp_ragged_perstep(const svae::VjpPerstepArgs& a, void* stream) {
  return svae::launch_vjp_ragged_perstep<SVAE_N>(a, (hipStream_t)stream);
}

#ifndef __HIP_DEVICE_COMPILE__   /* host data: a const table with a constant initialiser would be emitted for the device too */
extern "C" const svae::VjpUnit SVAE_CAT(svae_lds_vjp_unit_n, SVAE_N) = {.vjp = vjp, .vjp_lean = vjp_lean, .vjp_ragged = vjp_ragged,
  .vjp_ragged_perstep = vjp_ragged_perstep};
#endif
