// hmm_sample.hip -- batched HMM posterior sampling, z_{0:T-1} ~ p(z | potentials), by forward filtering and backward
// sampling, for MI355X (gfx950).
//
// What it replaces (reference = mattjj/svae): nothing the reference vendors -- its HMM work goes to pyhsmm's message
// interface, which has the operation; the arithmetic is DEFINED here (include/svae_hip.h, svae_hmm_sample_f64):
//   filter   a_t[k] = p(z_t = k | node_{0..t}): scaled forward recursion, per-step max-shift of the node potentials,
//            renormalisation to sum 1, log Z accumulated as mantissa/exponent pairs; a sequence with a live component of
//            an unnormalised message below 1e-250 or a normaliser below 1e-200 (the E-step's range, hmm_args.hpp) is
//            filtered again, all of it, in log space (hmm_sample_log.hip) and stores log a_t.
//   weights  t = T-1: w = a_{T-1};  t < T-1: w[k] = a_t[k] exp(pair[k][z_{t+1}] - M), M = the matrix' largest entry;
//            a total below 1e-200, and every step of a sequence whose record is log a_t:
//            w[k] = exp(log a_t[k] + pair[k][z_{t+1}] - max_k(..)), inline.
//   select   C[k] = w[0] + .. + w[k], fp64 adds IN INDEX ORDER;  thr = clamp(u, 0, 1) C[K-1] (NaN u = 0);
//            z_t = #{k : C[k] <= thr}, and the lowest k with C[k] = C[K-1] if that count is K.
//            Both rules are one test, (C[k] <= thr and C[k] < C[K-1]): C only rises where w[k] > 0, so on a chain with
//            finite log Z the drawn state has positive weight -- a forbidden transition or observation is never drawn.
// The caller supplies the uniforms u (B,S,T), as eps of the LDS sampler.
//
// One entry = three launches: filter and draw, each in Viterbi's two mappings (hmm_sample_kernel.hpp), and between them
// the log-space filter of hmm_sample_log.hip, one wavefront per sequence, which leaves at once where the scaled filter
// raised no flag (the flag is the sequence's step-0 record itself: hmm_sample_kernel.hpp):
//   filter   K <= 16: one 16-lane DPP row per sequence, four per wavefront; 17 .. 64: one wavefront per sequence.  The
//            forward half of the one-directional E-step kernels, restated (hmm_estep.hip and hmm_estep_wide.hip are not
//            touched and share no code with this unit).  Writes a_t, KP = 16 / 32 / 64 doubles per step (padding 0), to the
//            caller's workspace, and log Z.
//   draw     the B S chains are independent: one row (K <= 16) or one wavefront (wide) per (b, s), b = r / S, so S
//            scales by occupancy.  K <= 16 keeps the step in registers: lane k holds row k of exp(pair - M), z_{t+1}
//            is a one-hot row vector, the matrix column is K broadcast FMAs with it, the cumulative sum K masked
//            broadcast FMAs (x 1.0 or 0.0: exact adds), the new one-hot the difference of the compare and its one-lane
//            shift; labels leave 16 per row and store.  Wide: the matrix transposed in LDS (lane k reads AT[z][k], z
//            wave-uniform), the cumulative sum through an LDS line behind KP zeros (unit stride, index order), z from a
//            ballot; labels leave 64 per store.  a_t and u_t do not depend on the path: they are loaded a block ahead,
//            and no memory access on the serial chain has an address that depends on z (the wide kernel's LDS row aside).
// Every data-dependent index is masked into range before it addresses LDS or memory.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/svae_hip.h"
#include "dpp.hpp"
#include "hmm_sample_kernel.hpp"      // the four kernel templates and their launch; this unit instantiates RAGGED = false

extern "C" size_t svae_hmm_sample_workspace_bytes(int B, int T, int K) {
  if (B <= 0 || T <= 0 || K <= 0 || K > SVAE_HMM_MAX_K) return 0;
  return (size_t)B * T * svae::hmm_kp(K) * sizeof(double);      // (a multiple of 128)
}

extern "C" int svae_hmm_sample_f64(int B, int T, int K, int S, int pair_batched,
                                   const double* init_params, const double* pair_params,
                                   const double* node_params, const double* u,
                                   int32_t* states, double* logZ,
                                   void* workspace, size_t ws_bytes, void* stream) {
  if (const int rc = svae::hmm_check_model(B, T, K, pair_batched, init_params, pair_params)) return rc;
  if (B == 0) return 0;
  if (!node_params) return -7;
  if (S < 1) return -8;
  if (!u) return -9;
  if (!states) return -10;
  if (!workspace) return -11;
  if (ws_bytes < svae_hmm_sample_workspace_bytes(B, T, K)) return -12;
  if (((uintptr_t)workspace & 15) != 0) return -13;
  svae::SampleArgs a;
  svae::hmm_set_model(a, B, T, K, pair_batched ? (long)K * K : 0, init_params, pair_params, node_params);
  a.S = S; a.u = u; a.states = states; a.logZ = logZ; a.ws = (double*)workspace;
  return svae::launch_sample<false>(a, (hipStream_t)stream);
}
