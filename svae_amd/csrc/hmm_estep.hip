// hmm_estep.hip -- batched HMM E-step (forward-backward + expected statistics) for MI355X (gfx950).
//
// What it replaces (reference = mattjj/svae, /root/reference):
//   hmm_logZ        svae/hmm/cython_hmm_inference.pyx:93-121   (log-space forward pass)
//   hmm_logZ_grad   svae/hmm/cython_hmm_inference.pyx:126-166  (its reverse pass at g = 1 IS the
//                   E-step: expected initial state, transition counts, state marginals;
//                   `hmm_estep_slow = vgrad(hmm_logZ)`, svae/hmm/hmm_inference.py:65)
//   hmm_estep       svae/hmm/hmm_inference.py:21-41, which delegates to the un-vendored pyhsmm
//                   messages (parity pinned on hmm_logZ / hmm_logZ_grad).
// Used by the SLDS-SVAE coordinate ascent (svae/models/slds_svae.py:108-115, 159-175).
//
// Mapping: one DPP row (16 lanes) per sequence, 4 sequences per wavefront, lane k = discrete state k
// (K <= 16).  The matrix-vector products alpha' P and P (e . beta) are row_newbcast FMAs like the
// LDS kernels.  Scaled (not log-space) recursions: per step the node log-potentials are shifted by
// their maximum and exponentiated ONCE per lane (the reference does K logsumexp's of K terms per
// step), alpha is renormalised to sum 1, and log Z accumulates the scales as mantissa/exponent
// pairs (one log per sequence).  Forward quantities needed by the backward pass (alpha_t, e_t/c_t)
// go through a caller-owned workspace of HMM_WS doubles per (sequence, step).
// Dynamic range: a scaled step loses what falls below 2.3e-308 of its scale -- a transition entry more than ~708 nats
// below the matrix' maximum, a likelihood that far below the step's best, a message component below that share of
// the total -- and a component lost is never rebuilt: the chain stays in the wrong state with an ordinary normaliser.
// So a sequence is trusted only while EVERY live component of every step's unnormalised message stays >= HMM_LOW =
// 1e-250 (hmm_args.hpp: what a step drops is then 1e-50 below the positive sum it is dropped from) and every
// normaliser above 1e-200.  Any other sequence -- a state forbidden by a -1e4 or -inf potential counts -- raises its
// REDO flag in the workspace and is recomputed by the launch behind this one, ALL of it in log space, the reference's
// own arithmetic (hmm_estep_wide.hip, ROW instantiation: one wavefront per flagged sequence, K log-sum-exps of 16
// terms per step -- by the operation count roughly 10x a scaled sequence's time, not measured; the other workgroups
// read one flag and leave).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/svae_hip.h"
#include <type_traits>

#include "dpp.hpp"
#include "hmm_units.hpp"

#ifndef SVAE_HMM_TWOEND
#define SVAE_HMM_TWOEND 1      // two-ended kernel + one-directional fallback for flagged sequences (0: the one-directional kernel alone; A/B)
#endif

// hmm_estep_wide.hip: the all-log-space pass over the sequences the kernels of this file flagged
extern "C" int svae_hmm_row_logspace_launch(const svae::HmmArgs* a, void* stream);
extern "C" int svae_hmm_row_logspace_ragged_launch(const svae::HmmRaggedArgs* a, void* stream);
// ... and its scaled kernels of 17 <= K <= 64
extern "C" int svae_hmm_wide_launch(const svae::HmmArgs* a, void* stream);
extern "C" int svae_hmm_wide_ragged_launch(const svae::HmmRaggedArgs* a, void* stream);

namespace svae {

// workspace record per (sequence, step).  One-directional kernel (hmm_estep_kernel): [alpha (16) | e/c (16) | ..].
// Two-ended kernel (hmm_estep2_kernel): [alpha^ | e | w = e o beta^] in slots of 8 (K <= 8) or
// 16 lanes, then the maximum of the node potentials; entry HMM_REDO of the sequence's FIRST record is its REDO flag
// (hmm_args.hpp).  The log-space launch overwrites entries 0 .. 15 of a flagged sequence's records with log alpha_t.
constexpr double HMM_TINY = 1e-200;

// Maximum over the 16 lanes of a DPP row, in every lane: four rotate-and-max steps (row_ror:8/4/2/1 on the two halves
// of the double; compiler-scheduled, hazards padded by hipcc) instead of K broadcasts.
template <int R>
__device__ __forceinline__ double row_ror(double x) {
  const int lo = __builtin_amdgcn_update_dpp(0, __double2loint(x), 0x120 + R, 0xf, 0xf, false);
  const int hi = __builtin_amdgcn_update_dpp(0, __double2hiint(x), 0x120 + R, 0xf, 0xf, false);
  return __hiloint2double(hi, lo);
}
__device__ __forceinline__ double row_max16(double x) {
  x = __builtin_fmax(x, row_ror<8>(x));
  x = __builtin_fmax(x, row_ror<4>(x));
  x = __builtin_fmax(x, row_ror<2>(x));
  x = __builtin_fmax(x, row_ror<1>(x));
  return x;
}

// RAG (svae_hmm_ragged_estep_f64; never with FUSED): the four rows of a wavefront have their own lengths.  The trip count
// is the longest of them (wave-uniform) and every row runs under its own mask, by SELECTS, not by a neutral tail (an
// identity transition would have to replace the register-resident P / PT per row and step): the row's loads are clamped
// to its last step L-1 -- nothing stored at t >= L is read --, a step at t >= L is computed on that clamped data and
// dropped (alpha, the logZ accumulators and their renormalisation, the range test `bad` and every workspace store are
// conditional on t < L, so a row's results depend on its own length and data only), the backward pass leaves beta = 1
// and the xi sums alone while t >= L-1, and E_states from L on is zeroed after the last cross-lane operation.  A row's
// REDO flag depends on its own live steps only; the log-space launch behind the kernel cuts at the same length.
// All of it is `if constexpr`: the uniform instantiations
// compile to what they were.
template <int K, bool FUSED = false, bool RAG = false>
__global__ __launch_bounds__(64) void hmm_estep_kernel(const std::conditional_t<RAG, HmmRaggedArgs, HmmArgs> a) {
  static_assert(!(RAG && FUSED), "ragged launches take node potentials");
  const int lane = threadIdx.x;
  const int c = lane & 15;
  const int brow = blockIdx.x * 4 + (lane >> 4);
  const int bslot = brow < a.B ? brow : a.B - 1;
  // (indexed launches: a negative entry marks an unused slot -- the list is compacted, so a wavefront's row 0 is live
  //  whenever any of its rows is; idle rows repeat it)
  const int braw = a.seq_index ? a.seq_index[bslot] : bslot;
  const bool valid = brow < a.B && braw >= 0;
  if (!__any(valid)) return;
  const int b = valid ? braw : __shfl(braw, 0);
  const bool col = c < K;
  const int cc = col ? c : 0;
  const int T = a.T;
  const double NEG_BIG = -1.0e300;
  // RAG: TL = the row's own length (clamped for addressing; a value outside 1..T raises the status word), TW = the
  // longest of the wavefront's rows
  int TL = T, TW = T;
  if constexpr (RAG) {
    const int l = a.lengths[b];
    if ((l < 1 || l > T) && valid && c == 0) atomicOr(a.info, 1);
    TL = l < 1 ? 1 : (l > T ? T : l);
    int m = TL;
    const int m1 = __shfl_xor(m, 16, 64);
    m = m1 > m ? m1 : m;
    const int m2 = __shfl_xor(m, 32, 64);
    m = m2 > m ? m2 : m;
    TW = __builtin_amdgcn_readfirstlane(m);
  }
  // transition matrix in both layouts, shifted by its maximum (the shift goes into logZ)
  const double* pp = a.pair_params + (long)b * a.pair_stride;
  double lp[K], lpT[K];
  static_for<0, K>([&](auto j) {
    const double v = pp[j * K + cc], vt = pp[cc * K + j];
    lp[j] = col ? v : NEG_BIG;            // lp[j][c] = log P[j][c]
    lpT[j] = col ? vt : NEG_BIG;          // lpT[k][c] = log P[c][k]
  });
  double pmax = NEG_BIG;
  static_for<0, K>([&](auto j) { pmax = fmax(pmax, lp[j]); });
  static_for<0, 4>([&](auto s) { pmax = fmax(pmax, __shfl_xor(pmax, 1 << s, 16)); });
  double P[K], PT[K];
  static_for<0, K>([&](auto j) { P[j] = col ? exp(lp[j] - pmax) : 0.0; PT[j] = col ? exp(lpT[j] - pmax) : 0.0; });

  const double* node = FUSED ? nullptr : a.node_params + ((long)b * T) * K + cc;
  // FUSED: node potential of step t >= 1 = pc[t-1][0] + pc[t][1] + lz (two loads instead of one)
  const double* pc = FUSED ? a.pair_contr + ((long)b * T) * 2 * K + cc : nullptr;
  const double lzc = FUSED ? a.lz[cc] : 0.0;
  // (callers clamp t to [1, T-1]; with T = 1 the second FUSED read is clamped into the row as well: the value is unused)
  auto node_at = [&](int t) -> double {
    if constexpr (FUSED) return (pc[(long)(t - 1) * 2 * K] + pc[(long)(t < T ? t : T - 1) * 2 * K + K]) + lzc;
    else if constexpr (RAG) return node[(long)(t < TL ? t : TL - 1) * K];
    else return node[(long)(t < T ? t : T - 1) * K];
  };
  double node0;
  if constexpr (FUSED) {
    // <E x0 x0', J_c> + <E x0, h_c> + cinit_c: lane c = state (once per sequence)
    const int n = a.n;
    const double* ei = a.lds_E_init + (long)b * (n * n + n);
    const double* Jc = a.init_J + (long)cc * n * n;
    const double* hc = a.init_h + (long)cc * n;
    double s0 = 0.0;
    for (int q = 0; q < n * n; ++q) s0 = __builtin_fma(ei[q], Jc[q], s0);
    double s1 = 0.0;
    for (int q = 0; q < n; ++q) s1 = __builtin_fma(ei[n * n + q], hc[q], s1);
    node0 = (s0 + s1) + a.cinit[cc];
  } else {
    node0 = node[0];
  }
  double* nout = a.node_out ? a.node_out + ((long)b * T) * K + cc : nullptr;
  double* wsb = a.ws + ((long)b * T) * HMM_WS + c;
  double one = 1.0;
  bool bad = false;            // this lane saw a component below HMM_LOW or a normaliser below HMM_TINY

  // ---- forward ------------------------------------------------------------------------------------
  double lzM = 1.0;            // product of scales (mantissa) ...
  long lzE = 0;                // ... exponent
  double lzS = 0.0;            // sum of the subtracted maxima
  double alpha = 0.0;
  double nd_n = node0;
  for (int t = 0; t < TW; ++t) {
    const bool live = !RAG || t < TL;       // (RAG: a row past its length computes on its last step's data and keeps nothing)
    double nd = col ? nd_n : NEG_BIG;
    if (nout && valid && col) nout[(long)t * K] = nd_n;
    // next step's potentials, UNCONDITIONALLY (clamped): a load inside `if (t + 1 < T)` is waited for at the end of
    // its block, i.e. every step stalled for the full memory latency (0.55 -> ... us per step)
    if constexpr (RAG) nd_n = node_at(t + 1);
    else nd_n = node_at(t + 1 < T ? t + 1 : (T > 1 ? T - 1 : 1));
    if (t == 0) nd += col ? a.init_params[cc] : 0.0;
    const double m = row_max16(nd);         // m = max_k node[k]
    const double e = col ? exp_nonpos(nd - m) : 0.0;      // (nd - m <= 0: m is the row maximum)
    double pred;
    if (t == 0) {
      pred = col ? 1.0 : 0.0;
    } else {
      pred = 0.0;
      dpp_fence(alpha);
      static_for<0, K>([&](auto j) { mac_bc<j>(pred, alpha, P[j]); });   // sum_j alpha[j] P[j][k]
    }
    double al = pred * e;
    double cs = 0.0;
    dpp_fence(al);
    static_for<0, K>([&](auto k) { mac_bc<k>(cs, al, one); });            // c_t = sum_k
    const double rc = rcp_nr(cs);           // (v_rcp_f64 + two Newton steps: no fp64 divide on the serial chain)
    const double u_st = e * rc, shift = m + (t > 0 ? pmax : 0.0);
    bad = bad || (live && ((col && !(al >= HMM_LOW)) || !(cs > HMM_TINY)));
    if constexpr (RAG) {
      alpha = live ? al * rc : alpha;
      if (valid && live) { wsb[(long)t * HMM_WS] = alpha; wsb[(long)t * HMM_WS + 16] = u_st; }
      lzM = live ? lzM * __builtin_amdgcn_frexp_mant(cs) : lzM;
      lzE += live ? __builtin_amdgcn_frexp_exp(cs) : 0;
      lzS = live ? lzS + shift : lzS;
      if ((t & 15) == 15) {
        lzE += live ? __builtin_amdgcn_frexp_exp(lzM) : 0;
        lzM = live ? __builtin_amdgcn_frexp_mant(lzM) : lzM;
      }
    } else {
    alpha = al * rc;
    if (valid) { wsb[(long)t * HMM_WS] = alpha; wsb[(long)t * HMM_WS + 16] = u_st; }
    lzM *= __builtin_amdgcn_frexp_mant(cs);
    lzE += __builtin_amdgcn_frexp_exp(cs);
    lzS += shift;
    if ((t & 15) == 15) { lzE += __builtin_amdgcn_frexp_exp(lzM); lzM = __builtin_amdgcn_frexp_mant(lzM); }
    }
  }
  if (valid && c == 0) a.logZ[b] = lzS + ::log(lzM) + (double)lzE * 0.6931471805599453094;
  {
    // the row's REDO flag, written either way: the log-space launch behind this kernel reads it
    const bool redo = ((__ballot(bad) >> (lane & 48)) & 0xffffull) != 0;
    if (valid && c == 0) a.ws[((long)b * T) * HMM_WS + HMM_REDO] = redo ? 1.0 : 0.0;
  }

  // ---- backward + statistics ----------------------------------------------------------------------
  double beta = col ? 1.0 : 0.0;
  double acc[K];                       // xi sums without the transition factor
  static_for<0, K>([&](auto j) { acc[j] = 0.0; });
  double* oS = a.E_states + ((long)b * T) * K + cc;
  {
    const double gam = alpha * beta;      // t = T-1  (RAG: the row's own last step, where alpha froze)
    if (valid && col) oS[(long)(TL - 1) * K] = gam;
    if (TL == 1 && valid && col) a.E_init[(long)b * K + c] = gam;
  }
  // (u, alpha) of a step are fetched one step ahead: the loop is serial in t and the forward pass
  // wrote them ~T steps ago
  // (RAG: record indices clamped into the row's own steps; a row with t > L-2 is not `act`ive yet)
  auto rec_hi = [&](int t) -> long { return RAG ? (long)(t < TL - 1 ? t : (TL > 1 ? TL - 1 : 0)) : (long)t; };
  auto rec_lo = [&](int t) -> long { return RAG ? (long)(t < TL - 2 ? t : (TL > 2 ? TL - 2 : 0)) : (long)t; };
  double u_n = TW > 1 ? wsb[rec_hi(TW - 1) * HMM_WS + 16] : 0.0, al_n = TW > 1 ? wsb[rec_lo(TW - 2) * HMM_WS] : 0.0;
  for (int t = TW - 2; t >= 0; --t) {
    const double u = u_n;                              // e_{t+1} / c_{t+1}
    const double al = al_n;
    const bool act = !RAG || t <= TL - 2;
    {
      const int tp = t > 0 ? t - 1 : 0;                // unconditional (clamped) prefetch of step t-1
      u_n = wsb[rec_hi(tp + 1) * HMM_WS + 16];
      al_n = wsb[rec_lo(tp) * HMM_WS];
    }
    double w = u * beta;
    double al_f = al;
    if constexpr (RAG) { w = act ? w : 0.0; al_f = act ? al : 0.0; }       // (0 * 0 into the xi sums: exact)
    dpp_fence(w);
    dpp_fence(al_f);
    double bn = 0.0;
    static_for<0, K>([&](auto k) { mac_bc<k>(bn, w, PT[k]); });            // beta_t[j] = sum_k P[j][k] w[k]
    static_for<0, K>([&](auto j) { mac_bc<j>(acc[j], al_f, w); });         // xi sums (without P)
    if constexpr (RAG) beta = act ? bn : beta;
    else beta = bn;
    const double gam = al * beta;
    if (valid && col && act) oS[(long)t * K] = gam;
    if (t == 0 && valid && col && act) a.E_init[(long)b * K + c] = gam;
  }
  if (valid && col) {
    static_for<0, K>([&](auto j) { a.E_trans[(long)b * K * K + j * K + c] = acc[j] * P[j]; });
  }
  if constexpr (RAG) {
    // E_states from the row's length on: zeros, the 16 lanes of the row over the contiguous tail (after the last
    // cross-lane operation: the trip count differs between rows)
    if (valid) {
      double* tail = a.E_states + ((long)b * T) * K;
      for (long q = (long)TL * K + c; q < (long)T * K; q += 16) tail[q] = 0.0;
    }
  }
}

// ---- two-ended scaled forward-backward (round 4) ----------------------------------------------------------------------
// The one-directional kernel above runs 2 T dependent steps of ~190 / ~150 instructions on ONE wavefront per four
// sequences: 0.35 - 0.6 ms at T = 500 whatever the batch (latency-bound: the SLDS ascent launches it a dozen times per
// step).  Most of a step does not depend on the recursion, and alpha and beta do not depend on each other:
//   phase 1 (parallel in t, both wavefronts of the workgroup, half of the steps each): node potentials (FUSED: built from
//            the LDS kernel's contractions), their row maximum m_t, e_t = exp(node_t - m_t)            -> workspace
//   phase 2 (serial, concurrent): wavefront 0  alpha^_t = normalise((alpha^_{t-1} P) o e_t), log Z     (~55 instructions)
//                                  wavefront 1  beta^_t = normalise(P w_{t+1}),  w_t = e_t o beta^_t   (~50 instructions)
//            -- each with its OWN scaling: gamma and xi are normalised per step in phase 3, so the scalings cancel
//   phase 3 (parallel in t, half each): q = P w_{t+1},  Z_t = <alpha^_t, q>,  gamma_t = alpha^_t o q / Z_t,
//            xi sums  acc[j][k] += alpha^_t[j] w_{t+1}[k] / Z_t  (E_trans = P o acc), summed over the two wavefronts in LDS.
// Every phase streams its operands through a register ring HMM2_D steps deep (a serial step is ~0.15 us of arithmetic
// against 1 - 2 us of memory latency); no branch inside the steady-state loops (hipcc's wait counts degrade to
// vmcnt(0) across one).  The records are compact -- [alpha^ | e | w] in slots of 8 lanes for K <= 8 -- inside the common
// record stride: half the traffic of full-width slots at 2048 sequences.
// Range (see the head of the file): a live component of the forward message alpha^_t or of the backward message w_t
// below HMM_LOW, or a normaliser below HMM_TINY, anywhere raises the sequence's REDO flag -- a compare and an OR beside
// the dependent chain, no branch.  The threshold is absolute: between two renormalisations a message's sum only leaves
// [HMM_LOW, 16^3], so what an unnormalised step drops (below 16^3 * 2.3e-308) is still 1e-50 below every component kept.
// alpha^ and w both keep their relative accuracy then, and phase 3 (Z_t > HMM_TINY) loses at most 1e-100 of a step's
// posterior mass.  The log-space launch behind this kernel recomputes the flagged sequences (hmm_estep_wide.hip, ROW
// instantiation; its other workgroups leave at once).  Same mapping: one DPP row per sequence, lane = state.
constexpr int HMM2_D = 8;
#ifndef SVAE_HMM2_NORM
#define SVAE_HMM2_NORM 4
#endif
constexpr int HMM2_NORM = SVAE_HMM2_NORM;     // renormalise the forward / backward messages every HMM2_NORM-th step (1: every step)
static_assert(HMM2_D % HMM2_NORM == 0, "ring positions fix the renormalisation steps");
constexpr int HMM2_WAVES = 4;     // wavefronts per workgroup: all of them share phases 1 and 3, two run the recursions
template <int K, bool FUSED>
__global__ __launch_bounds__(64 * HMM2_WAVES) void hmm_estep2_kernel(const HmmArgs a) {
  constexpr int D = HMM2_D, NW = HMM2_WAVES;
  constexpr int KS = K <= 8 ? 8 : 16;                    // slot width
  constexpr int OA = 0, OE = KS, OW = 2 * KS, OM = 3 * KS;
  static_assert(OM < HMM_REDO, "record layout");
  __shared__ double xacc[(NW - 1) * 16 * 64];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int c = lane & 15;
  const int brow = blockIdx.x * 4 + (lane >> 4);
  const int bslot = brow < a.B ? brow : a.B - 1;
  const int braw = a.seq_index ? a.seq_index[bslot] : bslot;         // negative: unused slot (see hmm_estep_kernel)
  const bool valid = brow < a.B && braw >= 0;
  if (!__any(valid)) return;                                         // (the same rows in every wavefront of the workgroup)
  const int b = valid ? braw : __shfl(braw, 0);
  const bool col = c < K;
  const int cc = col ? c : 0;
  const int T = a.T;
  const double NEG_BIG = -1.0e300;
  const bool st = valid && col;

  const double* pp = a.pair_params + (long)b * a.pair_stride;
  double lp[K], lpT[K];
  static_for<0, K>([&](auto j) {
    const double v = pp[j * K + cc], vt = pp[cc * K + j];
    lp[j] = col ? v : NEG_BIG;
    lpT[j] = col ? vt : NEG_BIG;
  });
  double pmax = NEG_BIG;
  static_for<0, K>([&](auto j) { pmax = fmax(pmax, lp[j]); });
  static_for<0, 4>([&](auto s) { pmax = fmax(pmax, __shfl_xor(pmax, 1 << s, 16)); });
  double P[K], PT[K];        // P[j][lane c] = P[j][c];  PT[k][lane c] = P[c][k]   (shifted by the matrix' maximum; 0 in idle lanes)
  static_for<0, K>([&](auto j) { P[j] = col ? exp(lp[j] - pmax) : 0.0; PT[j] = col ? exp(lpT[j] - pmax) : 0.0; });

  // this lane's column of the records (idle lanes alias lane 0: they only ever load, and what they load is multiplied
  // by the zero columns of P / PT), and the records' scalars
  double* wsb = a.ws + ((long)b * T) * HMM_WS + cc;
  double* wsr = a.ws + ((long)b * T) * HMM_WS;
  double one = 1.0;
  bool bad = false;
  auto clampi = [](int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); };

  // ---- phase 1: e_t, m_t (and node_out) for this wavefront's half of the steps ---------------------------------------------
  {
    const double* node = FUSED ? nullptr : a.node_params + ((long)b * T) * K + cc;
    const double* pc = FUSED ? a.pair_contr + ((long)b * T) * 2 * K + cc : nullptr;
    const double lzc = FUSED ? a.lz[cc] : 0.0;
    double* nout = a.node_out ? a.node_out + ((long)b * T) * K + cc : nullptr;
    auto emit = [&](int t, double ndraw, double extra) {
      if (nout && st) nout[(long)t * K] = ndraw;
      const double nd = col ? ndraw + extra : NEG_BIG;
      const double m = row_max16(nd);
      const double e = col ? exp_nonpos(nd - m) : 0.0;
      if (st) wsb[(long)t * HMM_WS + OE] = e;
      if (valid && c == 0) wsr[(long)t * HMM_WS + OM] = m;
    };
    int p0 = (int)((long)T * wv / NW);
    const int p1 = (int)((long)T * (wv + 1) / NW);
    if (wv == 0) {
      if (valid && c == 0) wsr[HMM_REDO] = 0.0;
      double nd0;
      if constexpr (FUSED) {
        // <E x0 x0', J_c> + <E x0, h_c> + cinit_c: lane c = state (once per sequence)
        const int n = a.n;
        const double* ei = a.lds_E_init + (long)b * (n * n + n);
        const double* Jc = a.init_J + (long)cc * n * n;
        const double* hc = a.init_h + (long)cc * n;
        double s0 = 0.0;
        for (int q = 0; q < n * n; ++q) s0 = __builtin_fma(ei[q], Jc[q], s0);
        double s1 = 0.0;
        for (int q = 0; q < n; ++q) s1 = __builtin_fma(ei[n * n + q], hc[q], s1);
        nd0 = (s0 + s1) + a.cinit[cc];
      } else {
        nd0 = node[0];
      }
      emit(0, nd0, a.init_params[cc]);
    }
    if (p0 == 0) p0 = 1;                                 // (step 0 is wavefront 0's, above; T < NW: another range may start at 0)
    // steps p0 .. p1-1 (all >= 1), potentials requested D steps ahead
    auto node_at = [&](int t, double& x0, double& x1) {
      if constexpr (FUSED) { x0 = pc[(long)(t - 1) * 2 * K]; x1 = pc[(long)t * 2 * K + K]; }
      else { x0 = node[(long)t * K]; x1 = 0.0; }
    };
    if (p0 < p1) {
      double r0[D], r1[D];
      static_for<0, D>([&](auto u) { node_at(clampi(p0 + u, 1, p1 - 1), r0[u], r1[u]); });
      int t = p0;
      for (; t + D <= p1; t += D) {
        static_for<0, D>([&](auto u) {
          const double x0 = r0[u], x1 = r1[u];
          node_at(clampi(t + u + D, 1, p1 - 1), r0[u], r1[u]);
          emit(t + u, FUSED ? (x0 + x1) + lzc : x0, 0.0);
        });
      }
      static_for<0, D>([&](auto u) { if (t + u < p1) emit(t + u, FUSED ? (r0[u] + r1[u]) + lzc : r0[u], 0.0); });
    }
  }
  __syncthreads();

  // ---- phase 2: the two recursions, concurrently ------------------------------------------------------------------------------
  if (wv == 0) {
    double lzM = 1.0, lzS = 0.0, alpha = 0.0;
    long lzE = 0;
    const double colone = col ? 1.0 : 0.0;
    // (the message is renormalised every HMM2_NORM-th step only -- the sum, its reciprocal and the scaling are half of a
    //  step's dependent chain; phase 3 normalises per step anyway, so any positive scaling of alpha^_t will do.  Every
    //  step, normalised or not, checks its components against HMM_LOW)
    auto fstep = [&](int t, double e, double m, auto norm, auto renorm) {
      double p0 = 0.0, p1 = 0.0;                        // two accumulators: half the dependent chain
      dpp_fence(alpha);
      static_for<0, K>([&](auto j) { if constexpr (j % 2 == 0) mac_bc<j>(p0, alpha, P[j]); else mac_bc<j>(p1, alpha, P[j]); });
      const double first = t == 0 ? 1.0 : 0.0;          // (alpha starts at 0: pred_0 = 1 in the live lanes)
      const double pred = __builtin_fma(first, colone, p0 + p1);
      double al = pred * e;
      bad = bad || (col && !(al >= HMM_LOW));
      if constexpr (decltype(norm)::value) {
        double c0 = 0.0, c1 = 0.0;
        dpp_fence(al);
        static_for<0, K>([&](auto k) { if constexpr (k % 2 == 0) mac_bc<k>(c0, al, one); else mac_bc<k>(c1, al, one); });
        const double cs = c0 + c1;
        bad = bad || !(cs > HMM_TINY);
        al *= rcp_nr(cs);
        lzM *= __builtin_amdgcn_frexp_mant(cs);
        lzE += __builtin_amdgcn_frexp_exp(cs);
      }
      alpha = al;
      if (st) wsb[(long)t * HMM_WS + OA] = alpha;
      lzS += m + (t > 0 ? pmax : 0.0);
      if constexpr (decltype(renorm)::value) { lzE += __builtin_amdgcn_frexp_exp(lzM); lzM = __builtin_amdgcn_frexp_mant(lzM); }
    };
    double er[D], mr[D];
    static_for<0, D>([&](auto u) {
      const int tt = clampi(u, 0, T - 1);
      er[u] = wsb[(long)tt * HMM_WS + OE];
      mr[u] = wsr[(long)tt * HMM_WS + OM];
    });
    int t = 0;
    for (; t + D <= T; t += D) {
      static_for<0, D>([&](auto u) {
        const double e = er[u], m = mr[u];
        const int tn = clampi(t + u + D, 0, T - 1);
        er[u] = wsb[(long)tn * HMM_WS + OE];
        mr[u] = wsr[(long)tn * HMM_WS + OM];
        fstep(t + u, e, m, std::integral_constant<bool, (u % HMM2_NORM) == HMM2_NORM - 1>{}, std::integral_constant<bool, u == D - 1>{});
      });
    }
    static_for<0, D>([&](auto u) {
      if (t + u < T) fstep(t + u, er[u], mr[u], std::integral_constant<bool, (u % HMM2_NORM) == HMM2_NORM - 1>{},
                           std::integral_constant<bool, u == D - 1>{});
    });
    {
      // what the last renormalisation left unscaled
      double f0 = 0.0, f1 = 0.0;
      dpp_fence(alpha);
      static_for<0, K>([&](auto k) { if constexpr (k % 2 == 0) mac_bc<k>(f0, alpha, one); else mac_bc<k>(f1, alpha, one); });
      const double fs = f0 + f1;
      bad = bad || !(fs > HMM_TINY);
      lzM *= __builtin_amdgcn_frexp_mant(fs);
      lzE += __builtin_amdgcn_frexp_exp(fs);
    }
    if (valid && c == 0) a.logZ[b] = lzS + ::log(lzM) + (double)lzE * 0.6931471805599453094;
  } else if (wv == 1) {
    // w_{T-1} = e_{T-1} (beta_{T-1} = 1);  t = T-2 .. 1:  beta^_t = P w_{t+1} / sum,  w_t = e_t o beta^_t
    double w = col ? wsb[(long)(T - 1) * HMM_WS + OE] : 0.0;
    bad = bad || (col && !(w >= HMM_LOW));
    if (st) wsb[(long)(T - 1) * HMM_WS + OW] = w;
    auto bstep = [&](int t, double e, auto norm) {
      double q0 = 0.0, q1 = 0.0;
      dpp_fence(w);
      static_for<0, K>([&](auto k) { if constexpr (k % 2 == 0) mac_bc<k>(q0, w, PT[k]); else mac_bc<k>(q1, w, PT[k]); });
      double q = q0 + q1;                                 // lane j: sum_k P[j][k] w[k]
      if constexpr (decltype(norm)::value) {
        double d0 = 0.0, d1 = 0.0;
        dpp_fence(q);
        static_for<0, K>([&](auto j) { if constexpr (j % 2 == 0) mac_bc<j>(d0, q, one); else mac_bc<j>(d1, q, one); });
        const double d = d0 + d1;
        bad = bad || !(d > HMM_TINY);
        q *= rcp_nr(d);
      }
      w = e * q;
      bad = bad || (col && !(w >= HMM_LOW));
      if (st) wsb[(long)t * HMM_WS + OW] = w;
    };
    const int nsteps = T - 2 > 0 ? T - 2 : 0;            // step i: t = T-2-i  (t >= 1)
    if (nsteps > 0) {
      double er[D];
      static_for<0, D>([&](auto u) { er[u] = wsb[(long)clampi(T - 2 - u, 1, T - 1) * HMM_WS + OE]; });
      int i = 0;
      for (; i + D <= nsteps; i += D) {
        static_for<0, D>([&](auto u) {
          const double e = er[u];
          er[u] = wsb[(long)clampi(T - 2 - (i + u + D), 1, T - 1) * HMM_WS + OE];
          bstep(T - 2 - (i + u), e, std::integral_constant<bool, (u % HMM2_NORM) == HMM2_NORM - 1>{});
        });
      }
      static_for<0, D>([&](auto u) {
        if (i + u < nsteps) bstep(T - 2 - (i + u), er[u], std::integral_constant<bool, (u % HMM2_NORM) == HMM2_NORM - 1>{});
      });
    }
  }
  __syncthreads();

  // ---- phase 3: marginals and transition counts, half of the steps each -----------------------------------------------------------
  double acc[K];
  static_for<0, K>([&](auto j) { acc[j] = 0.0; });
  {
    const int q0_ = (int)((long)T * wv / NW);
    const int p1 = (int)((long)T * (wv + 1) / NW);
    const int q1_ = p1 < T - 1 ? p1 : T - 1;             // steps q0_ .. q1_-1 have a successor
    double* oS = a.E_states + ((long)b * T) * K + cc;
    double gam0 = 0.0;
    auto cstep = [&](int t, double al, double w1) {
      double s0 = 0.0, s1 = 0.0;
      dpp_fence(w1);
      static_for<0, K>([&](auto k) { if constexpr (k % 2 == 0) mac_bc<k>(s0, w1, PT[k]); else mac_bc<k>(s1, w1, PT[k]); });
      double g = al * (s0 + s1);
      double z0 = 0.0, z1 = 0.0;
      dpp_fence(g);
      static_for<0, K>([&](auto j) { if constexpr (j % 2 == 0) mac_bc<j>(z0, g, one); else mac_bc<j>(z1, g, one); });
      const double Z = z0 + z1;
      bad = bad || !(Z > HMM_TINY);
      const double rz = rcp_nr(Z);
      const double gam = g * rz;
      if (st) oS[(long)t * K] = gam;
      gam0 = t == 0 ? gam : gam0;
      double alz = al * rz;
      dpp_fence(alz);
      static_for<0, K>([&](auto j) { mac_bc<j>(acc[j], alz, w1); });     // lane k: alpha^_t[j] w_{t+1}[k] / Z_t
    };
    if (q0_ < q1_) {
      double ar[D], wr[D];
      static_for<0, D>([&](auto u) {
        const int tt = clampi(q0_ + u, 0, T - 2);
        ar[u] = wsb[(long)tt * HMM_WS + OA];
        wr[u] = wsb[(long)(tt + 1) * HMM_WS + OW];
      });
      int t = q0_;
      for (; t + D <= q1_; t += D) {
        static_for<0, D>([&](auto u) {
          const double al = ar[u], w1 = wr[u];
          const int tn = clampi(t + u + D, 0, T - 2);
          ar[u] = wsb[(long)tn * HMM_WS + OA];
          wr[u] = wsb[(long)(tn + 1) * HMM_WS + OW];
          cstep(t + u, al, w1);
        });
      }
      static_for<0, D>([&](auto u) { if (t + u < q1_) cstep(t + u, ar[u], wr[u]); });
    }
    if (q0_ == 0 && q0_ < q1_ && st) a.E_init[(long)b * K + c] = gam0;      // (the wavefront whose range holds step 0)
    if (wv == NW - 1) {                                   // beta_{T-1} = 1: gamma = alpha^ / its sum
      double al = col ? wsb[(long)(T - 1) * HMM_WS + OA] : 0.0;
      double f0 = 0.0, f1 = 0.0;
      dpp_fence(al);
      static_for<0, K>([&](auto k) { if constexpr (k % 2 == 0) mac_bc<k>(f0, al, one); else mac_bc<k>(f1, al, one); });
      const double fs = f0 + f1;
      bad = bad || !(fs > HMM_TINY);
      al *= rcp_nr(fs);
      if (st) oS[(long)(T - 1) * K] = al;
      if (T == 1 && st) a.E_init[(long)b * K + c] = al;
    }
  }
  // (`bad` is per lane: the row's sixteen bits of the ballot)
  if (((__ballot(bad) >> (lane & 48)) & 0xffffull) != 0 && valid && c == 0) wsr[HMM_REDO] = 1.0;
  if (wv > 0) static_for<0, K>([&](auto j) { xacc[((wv - 1) * 16 + j) * 64 + lane] = acc[j]; });
  __syncthreads();
  if (wv == 0 && st)
    static_for<0, K>([&](auto j) {
      double s = acc[j];
      static_for<0, NW - 1>([&](auto w) { s += xacc[(w * 16 + j) * 64 + lane]; });       // (fixed order)
      a.E_trans[(long)b * K * K + j * K + c] = s * P[j];
    });
}

// the scaled pass, then the log-space pass over the sequences it flagged.  The scaled pass is the two-ended kernel
// where there is a step for each of its wavefronts (T >= HMM2_WAVES; SVAE_HMM_TWOEND = 0: nowhere), else the
// one-directional kernel: one wavefront does all there is.  RAG (per-sequence lengths): the one-directional kernel's
// ragged instantiation, whatever T
template <int K, bool RAG>
static int launch_hmm(const std::conditional_t<RAG, HmmRaggedArgs, HmmArgs>& a, hipStream_t s) {
  const dim3 grid((a.B + 3) / 4);
  if constexpr (RAG) {
    hipLaunchKernelGGL((hmm_estep_kernel<K, false, true>), grid, dim3(64), 0, s, a);
  } else if (SVAE_HMM_TWOEND && a.T >= HMM2_WAVES) {
    if (a.pair_contr) hipLaunchKernelGGL((hmm_estep2_kernel<K, true>), grid, dim3(64 * HMM2_WAVES), 0, s, a);
    else hipLaunchKernelGGL((hmm_estep2_kernel<K, false>), grid, dim3(64 * HMM2_WAVES), 0, s, a);
  } else {
    if (a.pair_contr) hipLaunchKernelGGL((hmm_estep_kernel<K, true>), grid, dim3(64), 0, s, a);
    else hipLaunchKernelGGL((hmm_estep_kernel<K, false>), grid, dim3(64), 0, s, a);
  }
  if (hipGetLastError() != hipSuccess) return -1000;
  if constexpr (RAG) return svae_hmm_row_logspace_ragged_launch(&a, s);
  else return svae_hmm_row_logspace_launch(&a, s);
}

// K -> the launch above (K <= 16) or the wide unit's (hmm_estep_wide.hip: 17 <= K <= 64), for either kind of arguments
template <bool RAG>
static int hmm_dispatch(const std::conditional_t<RAG, HmmRaggedArgs, HmmArgs>& a, void* stream) {
  return hmm_dispatch_k(
      a.K, [&](auto k) { return launch_hmm<k, RAG>(a, (hipStream_t)stream); },
      [&](auto) {
        if constexpr (RAG) return svae_hmm_wide_ragged_launch(&a, stream);
        else return svae_hmm_wide_launch(&a, stream);
      });
}

// ---- glue of one SLDS coordinate-ascent sweep (slds_svae.py:159-175), after the HMM and the fused LDS kernels ----------
// one wavefront per active slot: lds_vlb = lognorm + <E z_0, cinit> + sum_{t>=1} <E z_t, lz>;  vlb_new = hmm_vlb + lds_vlb;
// iters += 1;  keep[slot] = |vlb_new - vlb| >= tol;  vlb = vlb_new
struct SldsGlueArgs {
  int nrun, T, K;
  double tol;
  const int32_t* __restrict__ seq_index;   // (nrun) or nullptr
  const double* __restrict__ E_states;     // (rows,T,K)
  const double* __restrict__ cinit;        // (K)
  const double* __restrict__ lz;           // (K)
  const double* __restrict__ lognorm;      // (rows) fused LDS kernel
  const double* __restrict__ hmm_vlb;      // (rows)
  double* __restrict__ lds_vlb;            // (rows) out
  double* __restrict__ vlb;                // (rows) in/out
  int32_t* __restrict__ iters;             // (rows) in/out
  int32_t* __restrict__ keep;              // (nrun) out: 1 = still iterating
};

__global__ __launch_bounds__(256) void slds_glue_kernel(const SldsGlueArgs a) {
  const int slot = blockIdx.x * 4 + (threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  if (slot >= a.nrun) return;
  const int r = a.seq_index ? a.seq_index[slot] : slot;
  if (r < 0) { if (lane == 0) a.keep[slot] = 0; return; }            // unused slot
  const double* es = a.E_states + (long)r * a.T * a.K;
  const int K = a.K, TK = a.T * K;
  double acc = 0.0;
  for (int q = lane; q < TK; q += 64) {
    const int k = q % K;
    acc = __builtin_fma(es[q], q < K ? a.cinit[k] : a.lz[k], acc);
  }
  for (int off = 32; off > 0; off >>= 1) acc += __shfl_xor(acc, off);       // (fixed order: reproducible)
  if (lane == 0) {
    const double lv = a.lognorm[r] + acc;
    const double nv = a.hmm_vlb[r] + lv;
    a.lds_vlb[r] = lv;
    a.iters[r] += 1;
    a.keep[slot] = !(fabs(nv - a.vlb[r]) < a.tol) ? 1 : 0;
    a.vlb[r] = nv;
  }
}

// stable compaction of the active list: out = [seq_index[i] : keep[i]], count[0] = its length (one workgroup)
__global__ __launch_bounds__(1024) void slds_compact_kernel(int nrun, const int32_t* __restrict__ seq_index,
                                                            const int32_t* __restrict__ keep, int32_t* __restrict__ out,
                                                            int32_t* __restrict__ count) {
  __shared__ int part[1024];
  const int tid = threadIdx.x;
  const int per = (nrun + 1023) / 1024;
  const int lo = tid * per, hi = lo + per < nrun ? lo + per : nrun;
  int cnt = 0;
  for (int i = lo; i < hi; ++i) cnt += keep[i] != 0;
  part[tid] = cnt;
  __syncthreads();
  for (int off = 1; off < 1024; off <<= 1) {          // inclusive scan
    const int v = tid >= off ? part[tid - off] : 0;
    __syncthreads();
    part[tid] += v;
    __syncthreads();
  }
  int pos = part[tid] - cnt;
  for (int i = lo; i < hi; ++i)
    if (keep[i] != 0) out[pos++] = seq_index ? seq_index[i] : i;
  // the slots behind the new list are marked unused (-1): a caller may launch the next sweep on `nrun` slots before it
  // has read the new count (slds_svae.py: the host reads the count one sweep late); the kernels skip negative entries
  const int total = part[1023];
  for (int i = total + tid; i < nrun; i += 1024) out[i] = -1;
  if (tid == 1023) count[0] = total;
}

// ---- the two dense contractions at the ends of the SLDS coordinate ascent ------------------------------------------------------
// Node potentials of the HMM for ONE sample path x (B,T,n) (initialize_local_meanfield + get_arhmm_local_nodeparams,
// slds_svae.py:203-226, 131-147): the statistics of a path are outer products, so the contraction with state k's
// parameters is three quadratic forms.  One thread per (sequence, step), loop over the states: the parameters are
// wave-uniform (scalar loads), the path values sit in registers, each thread writes its K potentials contiguously.
template <int N>
__global__ __launch_bounds__(256) void slds_path_nodeparams_kernel(int B, int T, int K, const double* __restrict__ x,
                                                                   const double* __restrict__ init_J,
                                                                   const double* __restrict__ init_h,
                                                                   const double* __restrict__ cinit,
                                                                   const double* __restrict__ J11,
                                                                   const double* __restrict__ J12,
                                                                   const double* __restrict__ J22,
                                                                   const double* __restrict__ lz,
                                                                   double* __restrict__ out) {
  const long q = (long)blockIdx.x * 256 + threadIdx.x;
  if (q >= (long)B * T) return;
  const int t = (int)(q % T);
  double xa[N], xb[N];                       // x_{t-1} (t >= 1), x_t
  const double* xt = x + q * N;
  static_for<0, N>([&](auto i) { xb[i] = xt[i]; xa[i] = t > 0 ? xt[i - N] : 0.0; });
  double* o = out + q * K;
  for (int k = 0; k < K; ++k) {
    double acc;
    if (t == 0) {
      const double* J = init_J + (long)k * N * N;
      acc = cinit[k];
      static_for<0, N>([&](auto i) {
        double r = init_h[(long)k * N + i];
        static_for<0, N>([&](auto j) { r = __builtin_fma(J[i * N + j], xb[j], r); });
        acc = __builtin_fma(xb[i], r, acc);
      });
    } else {
      const double* A = J11 + (long)k * N * N;
      const double* C = J12 + (long)k * N * N;
      const double* D = J22 + (long)k * N * N;
      acc = lz[k];
      static_for<0, N>([&](auto i) {
        double ra = 0.0, rb = 0.0;
        static_for<0, N>([&](auto j) {
          ra = __builtin_fma(A[i * N + j], xa[j], ra);
          ra = __builtin_fma(C[i * N + j], xb[j], ra);
          rb = __builtin_fma(D[i * N + j], xb[j], rb);
        });
        acc = __builtin_fma(xa[i], ra, acc);
        acc = __builtin_fma(xb[i], rb, acc);
      });
    }
    o[k] = acc;
  }
}

// Per-step pair parameters of the LDS factor under the HMM marginals (get_var_lds_local_natparam, slds_svae.py:92-103):
// out_m[b,t,:] = sum_k w[b,t+1,k] P_m[k,:] for the three n x n blocks and the constant.  Bound by the 3 n^2 + 1 doubles
// written per (sequence, step): thread e of a workgroup owns output element e and keeps its K parameters in
// registers; the weights of a row are wave-uniform (scalar loads); workgroups stride over the rows.
__global__ __launch_bounds__(1024) void slds_mix_pair_kernel(int B, int T, int K, int nn, const double* __restrict__ w,
                                                             const double* __restrict__ J11, const double* __restrict__ J12,
                                                             const double* __restrict__ J22, const double* __restrict__ lz,
                                                             double* __restrict__ o11, double* __restrict__ o12,
                                                             double* __restrict__ o22, double* __restrict__ olz) {
  const int e = threadIdx.x;
  const int m = e / nn, ee = e - m * nn;             // block (0..2: the matrices, 3: the constant), element
  if (m > 3 || (m == 3 && ee > 0)) return;
  const double* P = m == 0 ? J11 : (m == 1 ? J12 : (m == 2 ? J22 : lz));
  double* O = m == 0 ? o11 : (m == 1 ? o12 : (m == 2 ? o22 : olz));
  const int es = m == 3 ? 1 : nn;                    // elements per state / per output row
  double pk[16];
  static_for<0, 16>([&](auto k) { pk[k] = k < K ? P[(long)k * es + ee] : 0.0; });
#ifndef SVAE_MIXPAIR_U
#define SVAE_MIXPAIR_U 4
#endif
#ifndef SVAE_MIXPAIR_NT
#define SVAE_MIXPAIR_NT 1
#endif
  constexpr int U = SVAE_MIXPAIR_U;                  // steps in flight per thread (their weight loads and stores overlap)
  for (long b = blockIdx.y; b < B; b += gridDim.y) {  // (no division in the loops: grid rows stride over the sequences)
    const double* wb = w + (b * T + 1) * K;
    double* Ob = O + b * (T - 1) * es + ee;
    for (int t0 = blockIdx.x * U; t0 < T - 1; t0 += gridDim.x * U) {
      double acc[U];
      static_for<0, U>([&](auto u) {
        const int t = t0 + u < T - 1 ? t0 + u : T - 2;
        const double* wr = wb + (long)t * K;
        acc[u] = 0.0;
        static_for<0, 16>([&](auto k) { if (k < K) acc[u] = __builtin_fma(wr[k], pk[k], acc[u]); });
      });
      // (non-temporal: 2.45 GB at configs[3], read by a later kernel -- 1.07 -> 0.64 ms)
      static_for<0, U>([&](auto u) { if (t0 + u < T - 1) st_stream<SVAE_MIXPAIR_NT != 0>(&Ob[(long)(t0 + u) * es], acc[u]); });
    }
  }
}


// The two contractions of the SLDS final pass over the per-step pair statistics S (B, T-1, E = 3 n^2) of the last LDS
// E-step (run_inference, /root/reference/svae/models/slds_svae.py:289-310), in ONE pass over the 2.45 GB they are at
// configs[3] (they were two library GEMMs, each reading S: 2.2 + 1.0 ms):
//   node[b, t+1, k] = <S[b,t], P_k> + lz_k           get_arhmm_local_nodeparams  :131-147
//   G[k]           += w[b, t+1, k] S[b,t]            get_global_stats            :229-243 (summed over b and t)
// A wavefront takes one step at a time: lane l holds the entries l, l + 64, .. of S[b,t] (coalesced 512-byte rows, two
// steps prefetched), the K parameter rows of its entries and the K x EJ accumulators of G in registers; the K inner
// products are reduced across the wavefront by ONE multi-value butterfly (7 shuffles for 8 sums: each exchange halves the
// number of sums a lane still carries); the weights of a step are wave-uniform scalars.  Workgroups stride over the
// sequences and leave one (KK, E) partial of G each (summed by the caller in index order: deterministic).
#ifndef SVAE_PC_WPC
#define SVAE_PC_WPC 2
#endif
template <int EJ, int KK>
__global__ __launch_bounds__(256, SVAE_PC_WPC) void slds_pair_contract_kernel(int B, int T, int K, int E, const double* __restrict__ S,
                                                                   const double* __restrict__ P, const double* __restrict__ lz,
                                                                   const double* __restrict__ w, double* __restrict__ node,
                                                                   double* __restrict__ gpart) {
  static_assert(KK == 8, "the butterfly below is written for eight sums");
  __shared__ double red[EJ * KK * 64];
  const int lane = threadIdx.x & 63, wv = __builtin_amdgcn_readfirstlane((int)threadIdx.x >> 6);
  double pk[EJ][KK], ga[EJ][KK];
  int eo[EJ];
  static_for<0, EJ>([&](auto j) {
    const int e = lane + 64 * j;
    eo[j] = 8 * (e < E ? e : E - 1);                 // byte offset inside a row of S
    static_for<0, KK>([&](auto k) { pk[j][k] = (e < E && k < K) ? P[(long)(k < K ? k : 0) * E + eo[j] / 8] : 0.0; ga[j][k] = 0.0; });
  });
  const double lzl = lz[lane < K ? lane : 0];
  const bool b0 = lane & 1, b1 = lane & 2, b2 = lane & 4;
  // (no branch inside the time loop -- across one hipcc's wait counts degrade to vmcnt(0) and the prefetched rows are
  //  waited for at once: state indices are clamped and masked, and the lanes without a state store to a dummy word)
  int kx[KK];
  double mk[KK];
  static_for<0, KK>([&](auto k) { kx[k] = k < K ? k : K - 1; mk[k] = k < K ? 1.0 : 0.0; });
  const bool writer = lane < K;
  const int steps = T - 1;
  // store target of the lanes without a state: one word per WAVEFRONT inside this workgroup's own partial block (entries
  // e = wv of row k = 0), which the reduction below overwrites after its barriers -- no word shared between workgroups,
  // nothing the caller has to over-allocate
  double* const dummy = gpart + (long)blockIdx.x * KK * E + (wv < E ? wv : 0);
  for (long b = blockIdx.x; b < B; b += gridDim.x) {
    const double* Sb = S + b * steps * E;
    const double* wb = w + (b * T + 1) * K;
    double* nb = node + (b * T + 1) * K + (writer ? lane : 0);
    // register ring of D rows, every slot with a fixed role in the unrolled body (a rotation by moves would make each
    // move wait for the load it forwards): slot r is consumed and at once re-requested D steps further on
#ifndef SVAE_PC_D
#define SVAE_PC_D 2
#endif
    constexpr int D = SVAE_PC_D;
    double ring[D][EJ], wring[D];          // wring: the step's K weights, one per lane (read back with v_readlane:
    const int wl = 8 * (lane < K ? lane : K - 1);     // as eight scalar loads they were waited for one by one)
    // (row base through readfirstlane: a scalar base + the lane's 32-bit offset per load; left to itself hipcc keeps one
    //  64-bit pointer per (slot, chunk) in vector registers -- 30 of them -- and spills)
    auto load = [&](int t, double (&v)[EJ], double& wv_) {
      const uint64_t a = (uint64_t)(Sb + (long)(t < steps ? t : steps - 1) * E);
      const char* r = (const char*)(((uint64_t)(uint32_t)__builtin_amdgcn_readfirstlane((int)(a >> 32)) << 32) |
                                    (uint32_t)__builtin_amdgcn_readfirstlane((int)a));
      static_for<0, EJ>([&](auto j) { v[j] = *(const double*)(r + eo[j]); });
      const uint64_t aw = (uint64_t)(wb + (long)(t < steps ? t : steps - 1) * K);
      const char* rw = (const char*)(((uint64_t)(uint32_t)__builtin_amdgcn_readfirstlane((int)(aw >> 32)) << 32) |
                                     (uint32_t)__builtin_amdgcn_readfirstlane((int)aw));
      wv_ = *(const double*)(rw + wl);
    };
    static_for<0, D>([&](auto r) { load(wv + 4 * r, ring[r], wring[r]); });
    for (int t0 = wv; t0 < steps; t0 += 4 * D) {
      static_for<0, D>([&](auto r) {
        const int t = t0 + 4 * r;
        const bool live = t < steps;                       // (wave-uniform; a dead step computes on a clamped row)
        const double lv = live ? 1.0 : 0.0;
        double acc[KK];
        static_for<0, KK>([&](auto k) { acc[k] = 0.0; });
        static_for<0, KK>([&](auto k) {
          const double wk = __hiloint2double(__builtin_amdgcn_readlane(__double2hiint(wring[r]), kx[k]),
                                             __builtin_amdgcn_readlane(__double2loint(wring[r]), kx[k])) * (mk[k] * lv);
          static_for<0, EJ>([&](auto j) {
            acc[k] = __builtin_fma(ring[r][j], pk[j][k], acc[k]);
            ga[j][k] = __builtin_fma(wk, ring[r][j], ga[j][k]);
          });
        });
        load(t + 4 * D, ring[r], wring[r]);
        double r4[4], r2[2];
        static_for<0, 4>([&](auto i) {
          const double send = b0 ? acc[2 * i] : acc[2 * i + 1], keep = b0 ? acc[2 * i + 1] : acc[2 * i];
          r4[i] = keep + __shfl_xor(send, 1, 64);
        });
        static_for<0, 2>([&](auto i) {
          const double send = b1 ? r4[2 * i] : r4[2 * i + 1], keep = b1 ? r4[2 * i + 1] : r4[2 * i];
          r2[i] = keep + __shfl_xor(send, 2, 64);
        });
        double tot = (b2 ? r2[1] : r2[0]) + __shfl_xor(b2 ? r2[0] : r2[1], 4, 64);     // lane: the sum of state (lane & 7)
        tot += __shfl_xor(tot, 8, 64);
        tot += __shfl_xor(tot, 16, 64);
        tot += __shfl_xor(tot, 32, 64);
        double* dst = (writer && live) ? nb + (long)t * K : dummy;
        *dst = tot + lzl;
      });
    }
  }
  // the workgroup's partial of G: the four wavefronts' accumulators added in index order through LDS
  for (int q = 0; q < 4; ++q) {
    if (wv == q) {
      static_for<0, EJ>([&](auto j) {
        static_for<0, KK>([&](auto k) {
          double* r = red + (j * KK + k) * 64 + lane;
          *r = q == 0 ? ga[j][k] : *r + ga[j][k];
        });
      });
    }
    __syncthreads();
  }
  double* gp = gpart + (long)blockIdx.x * KK * E;
  for (int idx = threadIdx.x; idx < EJ * KK * 64; idx += 256) {
    const int l = idx & 63, k = (idx >> 6) % KK, j = idx / (64 * KK);
    const int e = l + 64 * j;
    if (e < E) gp[(long)k * E + e] = red[idx];
  }
}

}  // namespace svae

extern "C" size_t svae_hmm_workspace_bytes(int B, int T, int K) {
  if (B <= 0 || T <= 0 || K <= 0 || K > SVAE_HMM_MAX_K) return 0;
  if (K > 16) return (size_t)B * T * svae::hmm_wide_rec(svae::hmm_wide_kp(K)) * sizeof(double);
  return (size_t)B * T * svae::HMM_WS * sizeof(double);
}

extern "C" int svae_hmm_estep_f64(int B, int T, int K, int pair_batched,
                                  const double* init_params, const double* pair_params,
                                  const double* node_params,
                                  double* logZ, double* E_init, double* E_trans, double* E_states,
                                  void* workspace, size_t ws_bytes, void* stream) {
  if (B < 0) return -1;
  if (T < 1) return -2;
  if (K < 1 || K > SVAE_HMM_MAX_K) return -3;
  if (!init_params) return -5;
  if (!pair_params) return -6;
  if (!node_params) return -7;
  if (!logZ) return -8;
  if (!E_init) return -9;
  if (!E_trans) return -10;
  if (!E_states) return -11;
  if (!workspace || ws_bytes < svae_hmm_workspace_bytes(B, T, K)) return -12;
  if (B == 0) return 0;
  svae::HmmArgs a;
  a.B = B; a.T = T; a.K = K; a.pair_stride = pair_batched ? (long)K * K : 0;
  a.init_params = init_params; a.pair_params = pair_params; a.node_params = node_params;
  a.logZ = logZ; a.E_init = E_init; a.E_trans = E_trans; a.E_states = E_states;
  a.ws = (double*)workspace;
  a.seq_index = nullptr; a.n = 0; a.pair_contr = nullptr; a.lds_E_init = nullptr; a.init_J = nullptr; a.init_h = nullptr;
  a.cinit = nullptr; a.lz = nullptr; a.node_out = nullptr;
  return svae::hmm_dispatch<false>(a, stream);
}

// The launches of svae_hmm_estep_f64 on arguments a sibling unit has checked and filled (hmm_estep_chunked.hip: the
// indexed recompute of the sequences it flagged, with per-sequence pair parameters where the caller has them, and the
// whole call where one chunk holds the sequence).
extern "C" int svae_hmm_estep_args_launch(const svae::HmmArgs* a, void* stream) {
  return svae::hmm_dispatch<false>(*a, stream);
}

// HMM step of the SLDS coordinate ascent (hmm_meanfield, /root/reference/svae/models/slds_svae.py:108-115) on the rows
// `seq_index` lists, the node potentials taken from `node_params` (rows,T,K) if given, else built on the fly from the
// fused LDS mean-field kernel's outputs (get_arhmm_local_nodeparams, :131-147).
extern "C" int svae_slds_hmm_meanfield_f64(int B, int rows, int T, int K, int n,
                                           const double* hmm_init, const double* hmm_pair, const double* node_params,
                                           const double* pair_contr, const double* lds_E_init, const double* init_J,
                                           const double* init_h, const double* cinit, const double* lz,
                                           const int32_t* seq_index,
                                           double* logZ, double* E_init, double* E_trans, double* E_states,
                                           double* node_out, void* workspace, size_t ws_bytes, void* stream) {
  if (B < 0 || B > rows) return -1;
  if (T < 1) return -3;
  if (K < 1 || K > SVAE_HMM_MAX_K) return -4;
  if (n < 1 || n > 64) return -5;
  if (!hmm_init) return -6;
  if (!hmm_pair) return -7;
  if (!node_params && (K > 16 || !pair_contr || !lds_E_init || !init_J || !init_h || !cinit || !lz)) return -8;   /* K > 16: node potentials given */
  if (!logZ) return -16;
  if (!E_init) return -17;
  if (!E_trans) return -18;
  if (!E_states) return -19;
  if (!workspace || ws_bytes < svae_hmm_workspace_bytes(rows, T, K)) return -21;
  if (B == 0) return 0;
  svae::HmmArgs a;
  a.B = B; a.T = T; a.K = K; a.pair_stride = 0;
  a.init_params = hmm_init; a.pair_params = hmm_pair; a.node_params = node_params;
  a.logZ = logZ; a.E_init = E_init; a.E_trans = E_trans; a.E_states = E_states;
  a.ws = (double*)workspace;
  a.seq_index = seq_index; a.n = n;
  a.pair_contr = node_params ? nullptr : pair_contr; a.lds_E_init = lds_E_init; a.init_J = init_J; a.init_h = init_h;
  a.cinit = cinit; a.lz = lz; a.node_out = node_out;
  return svae::hmm_dispatch<false>(a, stream);
}

// After the HMM and the fused LDS kernels of a sweep: per listed row the LDS bound with its mixed constants, the
// stopping test |vlb_new - vlb| < tol of slds_svae.py:170-172, the sweep counter, and the compacted list of the rows
// still iterating (`next_index`, `next_count[0]`; stable order) -- no host arithmetic between two sweeps.
extern "C" int svae_slds_sweep_glue_f64(int B, int T, int K, double tol, const int32_t* seq_index,
                                        const double* E_states, const double* cinit, const double* lz,
                                        const double* lognorm, const double* hmm_vlb, double* lds_vlb, double* vlb,
                                        int32_t* iters, int32_t* keep_scratch, int32_t* next_index, int32_t* next_count,
                                        void* stream) {
  if (B < 0) return -1;
  if (T < 1) return -2;
  if (K < 1 || K > 16) return -3;
  if (!E_states || !cinit || !lz || !lognorm || !hmm_vlb) return -6;
  if (!lds_vlb || !vlb || !iters || !keep_scratch || !next_index || !next_count) return -11;
  hipStream_t s = (hipStream_t)stream;
  if (B > 0) {
    svae::SldsGlueArgs g;
    g.nrun = B; g.T = T; g.K = K; g.tol = tol; g.seq_index = seq_index; g.E_states = E_states; g.cinit = cinit; g.lz = lz;
    g.lognorm = lognorm; g.hmm_vlb = hmm_vlb; g.lds_vlb = lds_vlb; g.vlb = vlb; g.iters = iters; g.keep = keep_scratch;
    hipLaunchKernelGGL(svae::slds_glue_kernel, dim3((B + 3) / 4), dim3(256), 0, s, g);
    if (hipGetLastError() != hipSuccess) return -1000;
  }
  hipLaunchKernelGGL(svae::slds_compact_kernel, dim3(1), dim3(1024), 0, s, B, seq_index, keep_scratch, next_index, next_count);
  return hipGetLastError() == hipSuccess ? 0 : -1000;
}

// Sweep 0 of the ascent: HMM node potentials from one sample path (see slds_path_nodeparams_kernel).
extern "C" int svae_slds_path_nodeparams_f64(int B, int T, int K, int n, const double* x, const double* init_J,
                                             const double* init_h, const double* cinit, const double* J11,
                                             const double* J12, const double* J22, const double* lz, double* node_out,
                                             void* stream) {
  if (B < 0) return -1;
  if (T < 1) return -2;
  if (K < 1 || K > 16) return -3;
  if (n < 1 || n > 15) return -4;
  if (!x) return -5;
  if (!init_J || !init_h || !cinit) return -6;
  if (T > 1 && (!J11 || !J12 || !J22 || !lz)) return -9;
  if (!node_out) return -13;
  if (B == 0) return 0;
  hipStream_t s = (hipStream_t)stream;
  const dim3 grid((unsigned)(((long)B * T + 255) / 256)), block(256);
  switch (n) {
#define SVAE_CASE(NN) case NN: hipLaunchKernelGGL((svae::slds_path_nodeparams_kernel<NN>), grid, block, 0, s, B, T, K, x, \
                                                  init_J, init_h, cinit, J11, J12, J22, lz, node_out); break;
    SVAE_CASE(1) SVAE_CASE(2) SVAE_CASE(3) SVAE_CASE(4) SVAE_CASE(5) SVAE_CASE(6) SVAE_CASE(7) SVAE_CASE(8)
    SVAE_CASE(9) SVAE_CASE(10) SVAE_CASE(11) SVAE_CASE(12) SVAE_CASE(13) SVAE_CASE(14) SVAE_CASE(15)
#undef SVAE_CASE
  }
  return hipGetLastError() == hipSuccess ? 0 : -1000;
}

// The per-step pair parameters of the converged mean field (see slds_mix_pair_kernel): E_states (B,T,K) ->
// J11 / J12 / J22 (B,T-1,n,n), logZ (B,T-1).
extern "C" int svae_slds_mix_pair_natparam_f64(int B, int T, int K, int n, const double* E_states, const double* J11,
                                               const double* J12, const double* J22, const double* lz, double* out_J11,
                                               double* out_J12, double* out_J22, double* out_logZ, void* stream) {
  if (B < 0) return -1;
  if (T < 1) return -2;
  if (K < 1 || K > 16) return -3;
  if (n < 1 || 3 * n * n + 1 > 1024) return -4;
  if (!E_states) return -5;
  if (!J11 || !J12 || !J22 || !lz) return -6;
  if (!out_J11 || !out_J12 || !out_J22 || !out_logZ) return -10;
  if (B == 0 || T == 1) return 0;
  const int threads = ((3 * n * n + 1) + 63) / 64 * 64;
  const int per_seq = (T - 1 + SVAE_MIXPAIR_U - 1) / SVAE_MIXPAIR_U;    // U steps per thread and trip
#ifndef SVAE_MIXPAIR_GX
#define SVAE_MIXPAIR_GX 8
#endif
  const unsigned gx = (unsigned)(per_seq < SVAE_MIXPAIR_GX ? per_seq : SVAE_MIXPAIR_GX);
  hipLaunchKernelGGL(svae::slds_mix_pair_kernel, dim3(gx, (unsigned)(B < 65535 ? B : 65535)), dim3(threads), 0, (hipStream_t)stream, B, T, K, n * n,
                     E_states, J11, J12, J22, lz, out_J11, out_J12, out_J22, out_logZ);
  return hipGetLastError() == hipSuccess ? 0 : -1000;
}

// One pass over the per-step pair statistics of the SLDS final pass (see slds_pair_contract_kernel): node_out (B,T,K) rows
// 1 .. T-1 and `blocks` partials (blocks, 8, 3 n^2) of the weighted sums.  n <= 10, K <= 8.
extern "C" int svae_slds_pair_contract_f64(int B, int T, int K, int n, const double* pair_stats, const double* P,
                                           const double* lz, const double* weights, double* node_out, double* gpart,
                                           int blocks, void* stream) {
  if (B < 0) return -1;
  if (T < 2) return -2;
  if (K < 1 || K > 8) return -3;
  if (n < 1 || n > 10) return -4;
  if (!pair_stats) return -5;
  if (!P || !lz) return -6;
  if (!weights) return -8;
  if (!node_out || !gpart) return -9;
  if (blocks < 1) return -11;
  const int E = 3 * n * n;
  hipStream_t s = (hipStream_t)stream;
  if (B == 0) {
    (void)hipMemsetAsync(gpart, 0, sizeof(double) * (size_t)blocks * 8 * E, s);
    return 0;
  }
  if (blocks > B) {       // (workgroups without a sequence would leave their partial unwritten)
    (void)hipMemsetAsync(gpart + (size_t)B * 8 * E, 0, sizeof(double) * (size_t)(blocks - B) * 8 * E, s);
    blocks = B;
  }
  hipLaunchKernelGGL((svae::slds_pair_contract_kernel<5, 8>), dim3(blocks), dim3(256), 0, s, B, T, K, E, pair_stats, P, lz,
                     weights, node_out, gpart);
  return hipGetLastError() == hipSuccess ? 0 : -1000;
}

// svae_hmm_estep_f64 with per-sequence lengths (include/svae_hip.h): every check before any HIP call
extern "C" int svae_hmm_ragged_estep_f64(int B, int T, int K, int pair_batched,
                                         const double* init_params, const double* pair_params,
                                         const double* node_params, const int32_t* lengths,
                                         double* logZ, double* E_init, double* E_trans, double* E_states,
                                         int32_t* info, void* workspace, size_t ws_bytes, void* stream) {
  if (const int rc = svae::hmm_check_model(B, T, K, pair_batched, init_params, pair_params)) return rc;
  if (B == 0) return 0;
  if (!node_params) return -7;
  if (!lengths) return -8;
  if (!logZ) return -9;
  if (!E_init) return -10;
  if (!E_trans) return -11;
  if (!E_states) return -12;
  if (!info) return -13;
  if (!workspace) return -14;
  if (ws_bytes < svae_hmm_workspace_bytes(B, T, K)) return -15;
  svae::HmmRaggedArgs a;
  svae::hmm_set_model(a, B, T, K, pair_batched ? (long)K * K : 0, init_params, pair_params, node_params);
  a.logZ = logZ; a.E_init = E_init; a.E_trans = E_trans; a.E_states = E_states;
  a.ws = (double*)workspace;
  a.seq_index = nullptr; a.n = 0; a.pair_contr = nullptr; a.lds_E_init = nullptr; a.init_J = nullptr; a.init_h = nullptr;
  a.cinit = nullptr; a.lz = nullptr; a.node_out = nullptr;
  a.lengths = lengths; a.info = info;
  return svae::hmm_dispatch<true>(a, stream);
}
