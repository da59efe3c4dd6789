// lds_prim_vjp_n.hip -- one translation unit per latent dimension (-DSVAE_N=<n>) for the three reverse-mode primitives
// of lds_prim_vjp.hpp (filter, smoother and sampler VJPs on caller-held forward messages).  Every DPP broadcast is a
// self-fenced inline-asm statement (dpp.hpp mac_bc<K, NEG, true> / bcast_fenced); `make audit` checks the ISA of every
// latent dimension.
#include "lds_prim_vjp.hpp"

#ifndef SVAE_N
#error "compile with -DSVAE_N=<latent dim>"
#endif
#define SVAE_CAT_(a, b) a##b
#define SVAE_CAT(a, b) SVAE_CAT_(a, b)

// which: 0 filter VJP, 1 smoother VJP, 2 sampler VJP
extern "C" int SVAE_CAT(svae_lds_prim_vjp_n, SVAE_N)(int which, const svae::PrimArgs* a, void* stream) {
  return svae::launch_prim<SVAE_N>(which, *a, (hipStream_t)stream);
}
