// hmm_viterbi_perstep.hip -- batched HMM Viterbi decoding with PER-STEP transition potentials for MI355X (gfx950), K <= 64:
// svae_hmm_perstep_viterbi_f64 (include/svae_hip.h).
//
// The definition of svae_hmm_viterbi_f64 (hmm_viterbi.hip) with the step's own matrix, pair (T-1,K,K) or (B,T-1,K,K):
//   delta_0[k] = init[k] + node[0][k];   delta_t[k] = (max_j (delta_{t-1}[j] + pair[t-1][j][k])) + node[t][k]
//   psi_t[k] = the LOWEST j attaining the maximum;   z_{L-1} = the lowest k attaining max_k delta_{L-1}[k];
//   z_t = psi_{t+1}[z_{t+1}];   score = delta_{L-1}[z_{L-1}]
// fp64 additions in that order and strict `>` compares only (no multiply, so no FMA can arise): labels and score are
// reproducible bit for bit (tests/_hmm_perstep_decode_numpy.py).  -inf entries are ordinary values; NaN inputs lose every
// compare: unspecified labels in 0..K-1, no fault.  The unit must be built without fast-math.
//
// Mapping: the E-step's grouping (hmm_perstep_kernel.hpp): a group of G = 8, 16, 32 or 64 lanes per sequence (the
// smallest G >= K), lane = DESTINATION state k, 64 / G sequences per wavefront; W = 1 wavefront for K <= 16, W = 4 above.
//   P_t        the uniform kernels hold the one matrix in registers for the whole sequence; here lane k reads column k of
//              P_t straight from memory (consecutive lanes, consecutive addresses), and the entries of the next PF steps
//              are in flight in registers while the current PF are used (PF = 4 or 2 steps: 32 doubles each way).  A
//              max-plus step has no exp to hide a load -> LDS -> barrier chain behind; there is no LDS tile at all.
//              An entry beyond the share, the states or the length is -inf and its load goes to init_params (a select
//              of addresses, no branch per entry); where every lane wants every entry (wave-uniform) the loads are plain.
//   W = 4      every wavefront holds the same groups and takes a quarter of the j reduction (Q = ceil(K/4) source states:
//              Q entries per lane and step instead of K); the four partial (maximum, argument) pairs meet in LDS and
//              every wavefront combines them alike IN ASCENDING j WITH A STRICT `>`, which keeps the lowest index exactly
//              as the one-lane running maximum does; all four hold the same delta_t, the first stores psi_t.
//   delta      G <= 16: row_newbcast of the 16-lane DPP row (dpp.hpp bcast<j>; a group of 8 is half a row and selects
//              between lanes j and 8 + j); G >= 32: an LDS line per wavefront, read back as group-uniform loads.
// Padding source states carry P = -inf and can never win a strict compare.
// Back-pointers: one byte per (step, padded state) in the caller's workspace, KP = 16, 32 or 64 bytes per step
// (svae_hmm_viterbi_workspace_bytes).  Backtrace, by the first wavefront, in the manner of hmm_viterbi_kernel.hpp: G steps
// at a time staged through LDS (next block's loads in flight during the chase); the chase reads one LDS byte per step, its
// index masked into the stage; lane l keeps the label of step t0 + l: the labels leave as one vector store per block.
// Lengths: L = lengths[b] clamped to [1,T] (a value outside ORs 1 into the status word); a workgroup loops to the longest
// of its sequences with the shorter ones predicated off (no load, no store, delta frozen), the backtrace starts at the
// sequence's own L-1 inside the common block structure, labels from L on are -1.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/svae_hip.h"
#include "dpp.hpp"
#include "hmm_viterbi_kernel.hpp"     // vit_lds_sync, VitBlock; hmm_units.hpp (no kernel of that header is instantiated here)

namespace svae {

struct PerstepViterbiArgs {
  int B, T, K;
  long pair_stride;                        // doubles between sequences' (T-1,K,K) blocks (0 = shared)
  const double* __restrict__ init_params;  // (K)
  const double* __restrict__ pair_params;  // (T-1,K,K) or (B,T-1,K,K)
  const double* __restrict__ node_params;  // (B,T,K)
  const int32_t* __restrict__ lengths;     // (B) or nullptr
  int32_t* __restrict__ states;            // (B,T)
  double* __restrict__ score;              // (B) or nullptr
  int32_t* __restrict__ info;              // status word (nullptr only with lengths == nullptr)
  uint8_t* ws;                             // (B,T,KP) back-pointers
};

// lane J of the caller's group of G = 8 or 16 lanes
template <int G, int J>
__device__ __forceinline__ double vps_bcast(double x, int tl) {
  if constexpr (G == 16) {
    return bcast<J>(x);
  } else {
    const double lo = bcast<J>(x), hi = bcast<J + 8>(x);
    return (tl & 8) ? hi : lo;
  }
}

template <int G, int W>
__global__ __launch_bounds__(64 * W) void hmm_perstep_viterbi_kernel(const PerstepViterbiArgs a) {
  constexpr int KP = G < 16 ? 16 : G;            // back-pointer bytes per step (hmm_kp)
  constexpr int QMAX = G / W;                    // the most source states a wavefront reduces per step: 8 or 16
  constexpr int PF = 32 / QMAX;                  // steps of P_t in flight
  constexpr int NQ = KP / 16;                    // 16-byte pieces of a G-step back-pointer block, per lane
  __shared__ double pmv[2][W][64];               // partial maxima, by step parity
  __shared__ int pma[2][W][64];                  // their arguments
  __shared__ double line[W][64];                 // delta_{t-1}, one copy per wavefront
  __shared__ uint4 stage[64 * NQ];               // G steps x KP back-pointer bytes per group
  const int K = a.K, T = a.T;
  const int wv = threadIdx.x >> 6, tl = threadIdx.x & 63;
  const int lane = tl & (G - 1), grp = tl / G;
  const long b = (long)blockIdx.x * (64 / G) + grp;
  const bool valid = b < a.B;                    // an idle group shadows the last sequence for one step and stores nothing
  const long bb = valid ? b : a.B - 1;
  const bool live = lane < K;
  const int lk = live ? lane : 0;
  const bool first = wv == 0;
  const int Q = (K + W - 1) / W;                 // this wavefront's share of the j reduction: q0 .. q1-1
  const int q0 = min(wv * Q, K), q1 = min(q0 + Q, K), nq = q1 - q0;
  const double NINF = -__builtin_inf();

  int L = T;
  if (a.lengths) {
    const int l = a.lengths[bb];
    if ((l < 1 || l > T) && valid && first && lane == 0) atomicOr(a.info, 1);
    L = min(max(l, 1), T);
  }
  if (!valid) L = 1;
  int Lmax = L;                                  // the workgroup's trip count (every wavefront holds the same groups)
  for (int o = G; o < 64; o <<= 1) Lmax = max(Lmax, __shfl_xor(Lmax, o));

  const long KK = (long)K * K;
  const double* node = a.node_params + bb * T * K + lk;
  const double* pair = a.pair_params + bb * a.pair_stride + (long)q0 * K + lk;
  uint8_t* psi = a.ws + bb * T * KP + lane;

  // step t uses P_{t-1}: rows q0 .. q1-1 of column `lane`; beyond the share, the states or the length: -inf, and the load
  // goes to init_params instead (a select of addresses, not a branch per entry: nothing past the length is loaded)
  const double* safe = a.init_params + lk;
  auto load_p = [&](int t, double (&dst)[QMAX]) {
    const bool on = live && t < L;
    const double* P = pair + (long)(t - 1) * KK;
    if (nq == QMAX && __all(on)) {                    // (wave-uniform) every entry of every lane is wanted: plain loads
#pragma unroll
      for (int jj = 0; jj < QMAX; ++jj) dst[jj] = P[(long)jj * K];
    } else {
#pragma unroll
      for (int jj = 0; jj < QMAX; ++jj) {
        const bool in = on && jj < nq;
        const double v = *(in ? P + (long)jj * K : safe);
        dst[jj] = in ? v : NINF;
      }
    }
  };
  auto load_n = [&](int t) -> double {
    const bool in = live && t < L;
    const double v = *(in ? node + (long)t * K : safe);
    return in ? v : NINF;
  };

  double delta = live ? a.init_params[lk] + node[0] : NINF;

  auto step = [&](int t, const double (&Pc)[QMAX], double nd) __attribute__((always_inline)) {
    double best;
    int arg;
    if constexpr (W == 1) {
      best = vps_bcast<G, 0>(delta, tl) + Pc[0];
      arg = 0;
      static_for<1, QMAX>([&](auto j) {
        const double v = vps_bcast<G, j>(delta, tl) + Pc[j];
        const bool w = v > best;                      // strict: the first (lowest) j keeps a tie
        best = w ? v : best;
        arg = w ? (int)j : arg;
      });
    } else {
      __builtin_amdgcn_wave_barrier();
      line[wv][tl] = delta;
      vit_lds_sync();
      const double* ln = line[wv] + grp * G;
      best = ln[min(q0, G - 1)] + Pc[0];
      arg = min(q0, K - 1);
#pragma unroll
      for (int jj = 1; jj < QMAX; ++jj) {
        const double v = ln[min(q0 + jj, G - 1)] + Pc[jj];   // (beyond the share Pc = -inf: never greater)
        const bool w = v > best;
        best = w ? v : best;
        arg = w ? q0 + jj : arg;
      }
      const int buf = t & 1;
      pmv[buf][wv][tl] = best;
      pma[buf][wv][tl] = arg;
      __syncthreads();
      best = pmv[buf][0][tl];
      arg = pma[buf][0][tl];
#pragma unroll
      for (int w = 1; w < W; ++w) {                   // ascending j, strict: the lowest index is kept
        const double v = pmv[buf][w][tl];
        const bool g = v > best;
        best = g ? v : best;
        arg = g ? pma[buf][w][tl] : arg;
      }
    }
    const bool act = live && t < L;                   // a group past its length keeps delta_{L-1} and stores nothing
    delta = act ? best + nd : delta;
    if (valid && act && first) psi[(long)t * KP] = (uint8_t)arg;
  };

  double cur[PF][QMAX], nxt[PF][QMAX], ncur[PF], nnxt[PF];
#pragma unroll
  for (int u = 0; u < PF; ++u) {
    load_p(1 + u, cur[u]);
    ncur[u] = load_n(1 + u);
  }
  for (int t0 = 1; t0 < Lmax; t0 += PF) {
#pragma unroll
    for (int u = 0; u < PF; ++u) {
      load_p(t0 + PF + u, nxt[u]);
      nnxt[u] = load_n(t0 + PF + u);
    }
#pragma unroll
    for (int u = 0; u < PF; ++u) {
      const int t = t0 + u;
      if (t < Lmax) step(t, cur[u], ncur[u]);         // (workgroup-uniform)
    }
#pragma unroll
    for (int u = 0; u < PF; ++u) {
#pragma unroll
      for (int jj = 0; jj < QMAX; ++jj) cur[u][jj] = nxt[u][jj];
      ncur[u] = nnxt[u];
    }
  }
  if (!first) return;                                 // (no workgroup barrier below)

  // ---- z_{L-1}: the lowest k attaining the maximum ------------------------------------------------------------------------
  double best;
  int z = 0;
  if constexpr (W == 1) {
    best = vps_bcast<G, 0>(delta, tl);
    static_for<1, G>([&](auto k) {
      const double v = vps_bcast<G, k>(delta, tl);
      const bool w = v > best;
      best = w ? v : best;
      z = w ? (int)k : z;
    });
  } else {
    __builtin_amdgcn_wave_barrier();
    line[0][tl] = delta;
    vit_lds_sync();
    const double* ln = line[0] + grp * G;
    best = ln[0];
#pragma unroll 8
    for (int k = 1; k < G; ++k) {                     // (padding lanes hold -inf)
      const double v = ln[k];
      const bool w = v > best;
      best = w ? v : best;
      z = w ? k : z;
    }
  }
  if (valid && lane == 0 && a.score) a.score[b] = best;

  // ---- backtrace: G steps at a time through LDS; the back-pointers were written above by other lanes of this wavefront ----
  __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "agent");
  const uint4* src0 = reinterpret_cast<const uint4*>(a.ws + bb * T * KP);
  uint4* stg = stage + grp * G * NQ;
  int32_t* out = a.states + bb * T;
  auto load_block = [&](int blk) {
    VitBlock<NQ> d;
    const int t0 = min(blk, (L - 1) / G) * G;         // (a block past the group's length: its last one again, never chased)
    const int rows = min(L - t0, G);
    const uint4* src = src0 + (long)t0 * NQ;
    static_for<0, NQ>([&](auto r) {
      const int i = lane + G * (int)r;
      d.v[r] = src[i < rows * NQ ? i : 0];            // (pieces beyond the chain: never read back)
    });
    return d;
  };
  int blk = (Lmax - 1) / G;
  VitBlock<NQ> q = load_block(blk);
  for (; blk >= 0; --blk) {
    const VitBlock<NQ> qn = load_block(blk > 0 ? blk - 1 : 0);
    __builtin_amdgcn_wave_barrier();
    static_for<0, NQ>([&](auto r) { stg[lane + G * (int)r] = q.v[r]; });
    vit_lds_sync();
    const uint8_t* bytes = reinterpret_cast<const uint8_t*>(stg);
    int lab = 0;
    for (int l = G - 1; l >= 0; --l) {
      const int t = blk * G + l;
      const bool in = t < L;                          // steps beyond the chain pass z through
      lab = (in && lane == l) ? z : lab;
      const int zn = bytes[l * KP + (z & (G - 1))] & (G - 1);   // (masked: the read stays in the stage whatever it holds)
      z = (in && t > 0) ? zn : z;                     // (psi_0 is never followed)
    }
    const int t = blk * G + lane;
    if (valid && t < L) out[t] = lab;
    q = qn;
  }
  if (valid)
    for (int t = L + lane; t < T; t += G) out[t] = -1;
}

template <int G, int W>
static void launch_perstep_viterbi(const PerstepViterbiArgs& a, hipStream_t s) {
  constexpr int SPB = 64 / G;
  hipLaunchKernelGGL((hmm_perstep_viterbi_kernel<G, W>), dim3((unsigned)((a.B + SPB - 1) / SPB)), dim3(64 * W), 0, s, a);
}

}  // namespace svae

extern "C" int svae_hmm_perstep_viterbi_f64(int B, int T, int K, int pair_batched,
                                            const double* init_params, const double* pair_params,
                                            const double* node_params, const int32_t* lengths,
                                            int32_t* states, double* score,
                                            int32_t* info, void* workspace, size_t ws_bytes, void* stream) {
  if (const int rc = svae::hmm_check_model(B, T, K, pair_batched, init_params, pair_params, true)) return rc;
  if (B == 0) return 0;
  if (!node_params) return -7;
  if (!states) return -8;
  if (lengths && !info) return -9;
  if (!workspace) return -10;
  if (ws_bytes < svae_hmm_viterbi_workspace_bytes(B, T, K)) return -11;
  if (((uintptr_t)workspace & 15) != 0) return -12;   // back-pointer blocks are read back 16 bytes at a time
  svae::PerstepViterbiArgs a;
  svae::hmm_set_model(a, B, T, K, pair_batched ? (long)(T - 1) * K * K : 0, init_params, pair_params, node_params);
  a.lengths = lengths;
  a.states = states; a.score = score; a.info = info; a.ws = (uint8_t*)workspace;
  hipStream_t s = (hipStream_t)stream;
  svae::hmm_dispatch_group(K, [&](auto g, auto w) { svae::launch_perstep_viterbi<g, w>(a, s); });
  return hipGetLastError() == hipSuccess ? 0 : -1000;
}
