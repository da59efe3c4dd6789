// hmm_args.hpp -- launch arguments shared by the HMM kernel units (hmm_estep.hip: K <= 16; hmm_estep_wide.hip: K <= 64)
// and the sizes every HMM unit derives from K.  The host side of the entry points is hmm_units.hpp.
#pragma once
#include <stdint.h>

namespace svae {

struct HmmArgs {
  int B, T, K;
  long pair_stride;                       // doubles between sequences' pair params (0 = shared)
  const double* __restrict__ init_params; // (K)      log pi_0 (unnormalised ok)
  const double* __restrict__ pair_params; // (K,K) or (B,K,K)   log P[j][k]  (j -> k)
  const double* __restrict__ node_params; // (B,T,K)  log-likelihood potentials
  double* __restrict__ logZ;              // (B)
  double* __restrict__ E_init;            // (B,K)
  double* __restrict__ E_trans;           // (B,K,K)
  double* __restrict__ E_states;          // (B,T,K)
  double* __restrict__ ws;                // (B,T,HMM_WS)
  // indexed launches (SLDS coordinate ascent): slot i of the launch works on row seq_index[i] of every array
  const int32_t* __restrict__ seq_index;  // (B) or nullptr
  // FUSED node potentials (get_arhmm_local_nodeparams, slds_svae.py:131-147, from the fused LDS mean-field kernel's
  // outputs): node[b,0,k] = <E x0 x0', J_k> + <E x0, h_k> + cinit_k;  node[b,t,k] = pc[b,t-1,0,k] + pc[b,t,1,k] + lz_k
  int n;                                  // latent dimension of the LDS
  const double* __restrict__ pair_contr;  // (rows,T,2,K)
  const double* __restrict__ lds_E_init;  // (rows, n*n+n)
  const double* __restrict__ init_J;      // (K,n,n)
  const double* __restrict__ init_h;      // (K,n)
  const double* __restrict__ cinit;       // (K)
  const double* __restrict__ lz;          // (K)
  double* __restrict__ node_out;          // (rows,T,K) or nullptr: the node potentials used
};
// per-sequence lengths (svae_hmm_ragged_estep_f64): sequence b occupies steps 0 .. lengths[b]-1 of its (T, K) block; the
// arrays and the workspace records keep stride T.  A separate type: the uniform kernels' arguments stay what they are.
struct HmmRaggedArgs : HmmArgs {
  const int32_t* __restrict__ lengths;    // (B) device data, clamped to [1, T] for addressing and trip counts
  int32_t* __restrict__ info;             // status word: bit 0 = a length outside 1..T
};
// DPP-row kernels (K <= 16, hmm_estep.hip): HMM_WS doubles per (sequence, step); entry HMM_REDO of the sequence's FIRST
// record is its REDO flag (1.0: the scaled pass left its range, the log-space launch behind it recomputed the sequence).
constexpr int HMM_WS = 50;
constexpr int HMM_REDO = 49;
// Range of the scaled recursions (every kernel unit): a step is trusted while every live state's unnormalised message
// component -- (sum_j alpha^[j] P[j][k]) e[k], with alpha^ of sum <= 1 up to the unnormalised steps in between, P and e
// shifted to a maximum of 1 -- stays >= HMM_LOW.  Then every term a scaled step drops (an entry of P or e, or a product,
// below 2.3e-308) is more than 1e-50 below the positive sum it is dropped from, and every component keeps its relative
// accuracy.  A sequence with one component below it (or a normaliser below 1e-200) is REDONE IN LOG SPACE, all of it.
constexpr double HMM_LOW = 1e-250;
// wide kernel (17 <= K <= 64, one wavefront per sequence): workspace record per (sequence, step) =
// [alpha^_t or log alpha_t (KP) | normaliser c_t | REDO flag of the sequence (first record only)]
constexpr int HMM_WIDE_MAX_K = 64;
constexpr int hmm_wide_kp(int K) { return K <= 32 ? 32 : 64; }
constexpr int hmm_wide_rec(int KP) { return KP + 2; }
constexpr double HMM_WIDE_TINY = 1e-200;
// padded states of the Viterbi, sampling and derivative units, whose records have no width of their own below 17
// states: 16 (one DPP row per sequence), 32 or 64 (one wavefront per sequence)
constexpr int hmm_kp(int K) { return K <= 16 ? 16 : (K <= 32 ? 32 : 64); }
// per-step units (hmm_perstep_kernel.hpp, hmm_perstep_vjp_kernel.hpp and the per-step decoders): lanes per sequence,
// the smallest group that holds K states, and wavefronts per workgroup
constexpr int hmm_perstep_group(int K) { return K <= 8 ? 8 : K <= 16 ? 16 : K <= 32 ? 32 : 64; }
constexpr int hmm_perstep_waves(int K) { return K <= 16 ? 1 : 4; }

// time-chunked E-step (hmm_estep_chunked.hip; K <= HMM_CHUNKED_MAX_K, DPP rows): C = ceil(T / chunk) chunks per sequence,
// stage-3 records of HMM_CHUNK_REC doubles per (sequence, step) = [alpha^_t (16) | e_t / c_t (16)].  The workspace, in
// doubles (svae_hmm_chunked_workspace_bytes = 8 x total):
//   route   B                  the route words (B int32: 1 = recomputed by the serial route), then the B int32 slots of the
//                              indexed recompute launch
//   serial  B T HMM_WS         the serial E-step's records (recompute, chunk >= T); stage 3's records alias their head
//   stats   B (T K + K K + K)  E_states | E_trans | E_init of the serial route where the caller passes none (logZ only)
//   ops     B C K K            chunk operators, rows renormalised (chunk 0: row 0 = its filtered message)
//   scale   B C K              log scales of those rows
//   ahat    B C K              filtered message at every chunk's last step
//   bhat    B C K              backward message at every chunk's last step
//   ctrans  B C K K            every chunk's own transition counts, its entering boundary term included
constexpr int HMM_CHUNKED_MAX_K = 16;
constexpr int HMM_CHUNK_REC = 32;
static_assert(HMM_CHUNK_REC <= HMM_WS, "stage 3's records alias the serial records");
struct HmmChunkedLayout {
  long C, route, serial, stats, ops, scale, ahat, bhat, ctrans, total;      // offsets and total, in doubles
};
constexpr HmmChunkedLayout hmm_chunked_layout(long B, long T, long K, long chunk) {
  HmmChunkedLayout l{};
  l.C = chunk >= T ? 1 : (T + chunk - 1) / chunk;
  l.route = 0;
  l.serial = l.route + B;
  l.stats = l.serial + B * T * HMM_WS;
  l.ops = l.stats + B * (T * K + K * K + K);
  l.scale = l.ops + B * l.C * K * K;
  l.ahat = l.scale + B * l.C * K;
  l.bhat = l.ahat + B * l.C * K;
  l.ctrans = l.bhat + B * l.C * K;
  l.total = l.ctrans + B * l.C * K * K;
  return l;
}

// time-chunked Viterbi decoding (hmm_viterbi_chunked.hip; K <= HMM_CHUNKED_MAX_K, DPP rows): C = ceil(T / chunk) chunks
// per sequence (1 for chunk >= T).  The workspace, in BYTES (svae_hmm_chunked_viterbi_workspace_bytes = total); every
// offset is a multiple of 16:
//   psi    B T 16             back-pointers, one byte per step and padded state -- the head of the workspace, where the
//                             serial decoder keeps its own: the chunk >= T route (svae_hmm_viterbi_f64) fits
//   cand   B T 16             candidate labels [b][t][k]: the label at t of the path that ends t's chunk in state k
//                             (a buffer of its own: it does not alias psi)
//   fmap   B C 16             f_c[k]: the end state of chunk c - 1 on the path that ends chunk c in state k
//   ends   16 ceil(B C / 16)  e_c, one byte per chunk: the end state of chunk c on the decoded path
//   ops    8 B C K K          max-plus chunk operators M_c (chunk 0's block is not used)
//   delta  8 B C K            D_c, the recursion's value at every chunk's last step
struct HmmChunkedViterbiLayout {
  long C, psi, cand, fmap, ends, ops, delta, total;                         // offsets and total, in bytes
};
constexpr HmmChunkedViterbiLayout hmm_chunked_viterbi_layout(long B, long T, long K, long chunk) {
  HmmChunkedViterbiLayout l{};
  l.C = chunk >= T ? 1 : (T + chunk - 1) / chunk;
  l.psi = 0;
  l.cand = l.psi + B * T * 16;
  l.fmap = l.cand + B * T * 16;
  l.ends = l.fmap + B * l.C * 16;
  l.ops = l.ends + (B * l.C + 15) / 16 * 16;
  l.delta = l.ops + 8 * B * l.C * K * K;
  l.total = l.delta + 8 * B * l.C * K;
  return l;
}

// time-chunked posterior sampling (hmm_sample_chunked.hip; K <= HMM_CHUNKED_MAX_K, DPP rows): C = ceil(T / chunk) chunks
// per sequence (1 for chunk >= T), R = B S chains.  The workspace, in BYTES (svae_hmm_chunked_sample_workspace_bytes =
// total); every offset is a multiple of 16, r16(x) = x rounded up to one:
//   rec    128 B T            the serial sampler's records a_t (16 doubles per step; a redone sequence: log a_t) -- the
//                             head of the workspace, where svae_hmm_sample_f64 keeps its own: the chunk >= T route fits
//                             and sample_redone_sequences reads a chunked workspace unchanged
//   lz     r16(8 B)           log Z where the caller passes none
//   route  r16(4 B)           the route words (int32: 1 = left the range of stages 1 - 3, filtered again in log space)
//   ops    r16(8 B C K K)     chunk operators of the chunked E-step's stage 1
//   scale  r16(8 B C K)       their rows' log scales
//   ahat   r16(8 B C K)       filtered message at every chunk's last step
//   maps   16 R T             state maps psi_t[k], one byte per step and padded state
//   cand   16 R T             candidate labels [r][t][k] (a buffer of its own: it does not alias the maps)
//   fmap   16 R C             f_c[k]: the end state of chunk c - 1 on the path that ends chunk c in state k
//   ends   r16(R C)           e_c, one byte per chunk
struct HmmChunkedSampleLayout {
  long C, rec, lz, route, ops, scale, ahat, maps, cand, fmap, ends, total;  // offsets and total, in bytes
};
constexpr long hmm_r16(long x) { return (x + 15) / 16 * 16; }
constexpr HmmChunkedSampleLayout hmm_chunked_sample_layout(long B, long T, long K, long S, long chunk) {
  HmmChunkedSampleLayout l{};
  const long R = B * S;
  l.C = chunk >= T ? 1 : (T + chunk - 1) / chunk;
  l.rec = 0;
  l.lz = l.rec + 128 * B * T;
  l.route = l.lz + hmm_r16(8 * B);
  l.ops = l.route + hmm_r16(4 * B);
  l.scale = l.ops + hmm_r16(8 * B * l.C * K * K);
  l.ahat = l.scale + hmm_r16(8 * B * l.C * K);
  l.maps = l.ahat + hmm_r16(8 * B * l.C * K);
  l.cand = l.maps + 16 * R * T;
  l.fmap = l.cand + 16 * R * T;
  l.ends = l.fmap + 16 * R * l.C;
  l.total = l.ends + hmm_r16(R * l.C);
  return l;
}

}  // namespace svae
