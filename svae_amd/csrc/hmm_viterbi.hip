// hmm_viterbi.hip -- batched HMM Viterbi decoding (most probable state path and its score) for MI355X (gfx950).
//
// What it replaces (reference = mattjj/svae): hmm_viterbi of svae/hmm/hmm_inference.py:54-63, which delegates to the
// un-vendored pyhsmm; parity with it is unpinned, so the arithmetic is DEFINED here, exactly (include/svae_hip.h):
//   delta_0[k] = init[k] + node[0][k];   delta_t[k] = (max_j (delta_{t-1}[j] + pair[j][k])) + node[t][k]
//   psi_t[k] = the LOWEST j attaining the maximum;   z_{T-1} = the lowest k attaining max_k delta_{T-1}[k];
//   z_t = psi_{t+1}[z_{t+1}];   score = delta_{T-1}[z_{T-1}]
// fp64 additions in that order and strict `>` compares only: no multiply, so no FMA can arise, and a NumPy restatement
// in the same order reproduces labels and score bit for bit (tests/_hmm_viterbi_numpy.py).  -inf entries are ordinary
// values here (-inf + -inf = -inf, never greater than anything); NaN inputs lose every compare: unspecified labels in
// 0..K-1, no fault.  The unit must be built without fast-math.
//
// Two mappings, as the E-step's (hmm_estep.hip, hmm_estep_wide.hip):
//   K <= 16      one 16-lane DPP row per sequence, four sequences per wavefront, lane k = state k.  Column k of the
//                transition matrix in registers (K doubles); delta_{t-1}[j] reaches the row as row_newbcast:j (dpp.hpp
//                bcast<j>: compiler-scheduled, hazards padded by hipcc).  A step is K (broadcast, add, compare, select).
//   17 .. 64     one wavefront per sequence, lane = state, KP = 32 or 64 padded states that carry -inf and can never
//                win a strict compare.  Column in registers (KP doubles); delta_{t-1} published through an LDS line
//                and read back as wave-uniform loads.  The running maximum is kept in two halves [0, KP/2), [KP/2, KP)
//                (two independent chains) merged with a strict compare, which keeps the lowest index.
// Node potentials are loaded a block of steps ahead of their use (a step is shorter than a trip to HBM).
//
// Back-pointers: one byte per (step, state) in the caller's workspace, KP bytes per step (KP = 16, 32, 64).
// Backtrace (T dependent look-ups, kept off the HBM latency):
//   K <= 16      16 steps at a time: lane l of the row loads the 16 bytes of step t0 + l (one coalesced 256-byte read
//                per row, the next block's issued before the current one is chased) and packs them into a 64-bit map
//                of 16 nibbles; the chase is then row_newbcast:l of that map, a shift and a mask per step -- registers
//                only.  Lane l keeps the label of its step: 16 labels leave as one 64-byte vector store.
//   17 .. 64     64 steps at a time staged through LDS (64 KP bytes, next block's loads in flight during the chase);
//                the chase reads one LDS byte per step; lane l keeps the label of step t0 + l: one 256-byte store.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/svae_hip.h"
#include "dpp.hpp"

namespace svae {

struct ViterbiArgs {
  int B, T, K;
  long pair_stride;           // doubles between sequences' pair params (0 = shared)
  const double* init_params;  // (K)
  const double* pair_params;  // (K,K) or (B,K,K)   [j][k] = j -> k
  const double* node_params;  // (B,T,K)
  int32_t* states;            // (B,T)
  double* score;              // (B) or nullptr
  uint8_t* ws;                // (B,T,KP) back-pointers
};

constexpr int viterbi_kp(int K) { return K <= 16 ? 16 : (K <= 32 ? 32 : 64); }
constexpr int VIT_AHEAD = 8;          // node potentials in flight, steps

// 16 back-pointer bytes (values 0..15) -> 16 nibbles
__device__ __forceinline__ unsigned vit_pack4(unsigned w) {
  const unsigned x = w | (w >> 4);
  return (x & 0xffu) | ((x >> 8) & 0xff00u);
}
__device__ __forceinline__ unsigned long long vit_pack16(uint4 q) {
  const unsigned lo = vit_pack4(q.x) | (vit_pack4(q.y) << 16), hi = vit_pack4(q.z) | (vit_pack4(q.w) << 16);
  return ((unsigned long long)hi << 32) | lo;
}
// lane L of the caller's 16-lane row (row_newbcast:L on both halves; compiler-scheduled)
template <int L>
__device__ __forceinline__ unsigned long long vit_bcast_u64(unsigned long long x) {
  const int lo = __builtin_amdgcn_update_dpp(0, (int)(unsigned)(x & 0xffffffffull), DPP_ROW_NEWBCAST0 + L, 0xf, 0xf, true);
  const int hi = __builtin_amdgcn_update_dpp(0, (int)(unsigned)(x >> 32), DPP_ROW_NEWBCAST0 + L, 0xf, 0xf, true);
  return ((unsigned long long)(unsigned)hi << 32) | (unsigned)lo;
}

// ---- K <= 16: one DPP row per sequence ------------------------------------------------------------------------------
template <int K>
__global__ __launch_bounds__(64) void hmm_viterbi_row_kernel(const ViterbiArgs a) {
  const int lane = threadIdx.x;
  const int c = lane & 15;
  const int brow = blockIdx.x * 4 + (lane >> 4);
  const bool valid = brow < a.B;                      // idle rows repeat the last sequence and store nothing
  const long b = valid ? brow : a.B - 1;
  const bool col = c < K;
  const int cc = col ? c : 0;
  const int T = a.T;
  const double NEG_INF = -__builtin_inf();

  const double* pp = a.pair_params + b * a.pair_stride;
  double P[K];                                        // P[j] = pair[j][c]
  static_for<0, K>([&](auto j) { P[j] = pp[j * K + cc]; });
  const double* node = a.node_params + (b * T) * K + cc;
  uint8_t* psi = a.ws + (b * T) * 16 + c;

  double delta = col ? a.init_params[cc] + node[0] : NEG_INF;
  if (valid) psi[0] = 0;                              // (psi_0 is never followed; written so that every byte read is defined)

  auto load = [&](int t) -> double { return node[(long)(t < T ? t : T - 1) * K]; };
  double cur[VIT_AHEAD], nxt[VIT_AHEAD];
  static_for<0, VIT_AHEAD>([&](auto u) { cur[u] = load(1 + u); });
  for (int t0 = 1; t0 < T; t0 += VIT_AHEAD) {
    static_for<0, VIT_AHEAD>([&](auto u) { nxt[u] = load(t0 + VIT_AHEAD + u); });
    static_for<0, VIT_AHEAD>([&](auto u) {
      const int t = t0 + u;
      if (t < T) {                                    // (wave-uniform)
        double best = bcast<0>(delta) + P[0];
        int arg = 0;
        static_for<1, K>([&](auto j) {
          const double v = bcast<j>(delta) + P[j];
          const bool w = v > best;                    // strict: the first (lowest) j keeps a tie
          best = w ? v : best;
          arg = w ? (int)j : arg;
        });
        delta = col ? best + cur[u] : NEG_INF;
        if (valid) psi[(long)t * 16] = (uint8_t)arg;
      }
    });
    static_for<0, VIT_AHEAD>([&](auto u) { cur[u] = nxt[u]; });
  }

  double best = bcast<0>(delta);
  int z = 0;
  static_for<1, K>([&](auto k) {
    const double v = bcast<k>(delta);
    const bool w = v > best;
    best = w ? v : best;
    z = w ? (int)k : z;
  });
  if (valid && c == 0 && a.score) a.score[b] = best;

  // ---- backtrace: the back-pointers written above by OTHER lanes of this wavefront are read back below ---------------
  __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "agent");
  const uint4* rows = reinterpret_cast<const uint4*>(a.ws + (b * T) * 16);
  int32_t* out = a.states + b * T;
  auto load_row = [&](int blk) -> uint4 {
    const int t = blk * 16 + c;
    return rows[t < T ? t : T - 1];
  };
  int blk = (T - 1) >> 4;
  uint4 q = load_row(blk);
  for (; blk >= 0; --blk) {
    const uint4 qn = load_row(blk > 0 ? blk - 1 : 0);
    const int t = blk * 16 + c;
    // steps beyond the chain: the identity map (z passes through)
    const unsigned long long map = t < T ? vit_pack16(q) : 0xFEDCBA9876543210ull;
    int lab = 0;
    static_for<0, 16>([&](auto i) {
      constexpr int l = 15 - (int)i;
      lab = c == l ? z : lab;                         // z = the label of step blk*16 + l ...
      const unsigned long long m = vit_bcast_u64<l>(map);
      z = (int)((unsigned)(m >> (4 * z)) & 15u);      // ... and psi of that step leads to the step before
    });
    if (valid && t < T) out[t] = lab;
    q = qn;
  }
}

// ---- 17 <= K <= 64: one wavefront per sequence ----------------------------------------------------------------------
__device__ __forceinline__ void vit_lds_sync() {
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

template <int NQ>
struct VitBlock { uint4 v[NQ]; };

template <int KP>
__global__ __launch_bounds__(64) void hmm_viterbi_wide_kernel(const ViterbiArgs a) {
  constexpr int H = KP / 2;
  constexpr int NQ = KP / 16;                         // 16-byte pieces of a 64-step block, per lane
  __shared__ double line[64];
  __shared__ uint4 stage[64 * NQ];                    // 64 steps x KP back-pointer bytes
  const int lane = threadIdx.x;
  const int K = a.K, T = a.T;
  const long b = blockIdx.x;
  const bool st = lane < K;
  const int cc = st ? lane : 0;
  const double NEG_INF = -__builtin_inf();

  const double* pp = a.pair_params + b * a.pair_stride;
  const double* nd = a.node_params + (b * T) * K + cc;
  double Pc[KP];                                      // Pc[j] = pair[j][lane]; padding states: -inf
#pragma unroll
  for (int j = 0; j < KP; ++j) {
    const double v = pp[(j < K ? j : 0) * K + cc];
    Pc[j] = j < K ? v : NEG_INF;
  }
  uint8_t* psi = a.ws + (b * T) * KP + lane;
  double delta = st ? a.init_params[cc] + nd[0] : NEG_INF;
  if (lane < KP) psi[0] = 0;

  auto load = [&](int t) -> double { return nd[(long)(t < T ? t : T - 1) * K]; };
  constexpr int AHEAD = 4;
  double cur[AHEAD], nxt[AHEAD];
#pragma unroll
  for (int u = 0; u < AHEAD; ++u) cur[u] = load(1 + u);
  for (int t0 = 1; t0 < T; t0 += AHEAD) {
#pragma unroll
    for (int u = 0; u < AHEAD; ++u) nxt[u] = load(t0 + AHEAD + u);
#pragma unroll
    for (int u = 0; u < AHEAD; ++u) {
      const int t = t0 + u;
      if (t < T) {                                    // (wave-uniform)
        __builtin_amdgcn_wave_barrier();
        line[lane] = delta;
        vit_lds_sync();
        double b0 = line[0] + Pc[0], b1 = line[H] + Pc[H];
        int a0 = 0, a1 = H;
#pragma unroll
        for (int j = 1; j < H; ++j) {
          const double v0 = line[j] + Pc[j], v1 = line[H + j] + Pc[H + j];
          const bool w0 = v0 > b0, w1 = v1 > b1;
          b0 = w0 ? v0 : b0; a0 = w0 ? j : a0;
          b1 = w1 ? v1 : b1; a1 = w1 ? H + j : a1;
        }
        const bool w = b1 > b0;                       // the upper half wins only if strictly greater: lowest index kept
        b0 = w ? b1 : b0; a0 = w ? a1 : a0;
        delta = st ? b0 + cur[u] : NEG_INF;
        if (lane < KP) psi[(long)t * KP] = (uint8_t)a0;
      }
    }
#pragma unroll
    for (int u = 0; u < AHEAD; ++u) cur[u] = nxt[u];
  }

  __builtin_amdgcn_wave_barrier();
  line[lane] = delta;
  vit_lds_sync();
  double best = line[0];
  int z = 0;
#pragma unroll
  for (int k = 1; k < KP; ++k) {
    const double v = line[k];
    const bool w = v > best;
    best = w ? v : best;
    z = w ? k : z;
  }
  if (lane == 0 && a.score) a.score[b] = best;

  // ---- backtrace: 64 steps at a time through LDS ----------------------------------------------------------------------
  __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "agent");  // back-pointers written by other lanes of this wavefront
  const uint8_t* base = a.ws + (b * T) * KP;
  int32_t* out = a.states + b * T;
  auto load_block = [&](int t0) {
    VitBlock<NQ> d;
    const int rows = T - t0 < 64 ? T - t0 : 64;
    const uint4* src = reinterpret_cast<const uint4*>(base + (long)t0 * KP);
    static_for<0, NQ>([&](auto r) {
      const int i = lane + 64 * (int)r;
      d.v[r] = src[i < rows * NQ ? i : 0];            // (pieces beyond the chain: never read back)
    });
    return d;
  };
  int t0 = ((T - 1) >> 6) << 6;
  VitBlock<NQ> q = load_block(t0);
  for (; t0 >= 0; t0 -= 64) {
    const int rows = T - t0 < 64 ? T - t0 : 64;
    const VitBlock<NQ> qn = load_block(t0 >= 64 ? t0 - 64 : 0);
    __builtin_amdgcn_wave_barrier();
    static_for<0, NQ>([&](auto r) { stage[lane + 64 * (int)r] = q.v[r]; });
    vit_lds_sync();
    const uint8_t* bytes = reinterpret_cast<const uint8_t*>(stage);
    int lab = 0;
    for (int l = rows - 1; l >= 0; --l) {
      lab = lane == l ? z : lab;
      z = bytes[l * KP + z] & (KP - 1);               // (every byte is an index below K; the mask keeps the read in the stage whatever it holds)
    }
    if (lane < rows) out[t0 + lane] = lab;
    q = qn;
  }
}

template <int K>
static int launch_viterbi_row(const ViterbiArgs& a, hipStream_t s) {
  hipLaunchKernelGGL((hmm_viterbi_row_kernel<K>), dim3((a.B + 3) / 4), dim3(64), 0, s, a);
  return hipGetLastError() == hipSuccess ? 0 : -1000;
}

}  // namespace svae

extern "C" size_t svae_hmm_viterbi_workspace_bytes(int B, int T, int K) {
  if (B <= 0 || T <= 0 || K <= 0 || K > SVAE_HMM_MAX_K) return 0;
  const size_t bytes = (size_t)B * T * svae::viterbi_kp(K);
  return (bytes + 7) & ~(size_t)7;
}

extern "C" int svae_hmm_viterbi_f64(int B, int T, int K, int pair_batched,
                                    const double* init_params, const double* pair_params,
                                    const double* node_params, int32_t* states, double* score,
                                    void* workspace, size_t ws_bytes, void* stream) {
  if (B < 0) return -1;
  if (T < 1) return -2;
  if (K < 1 || K > SVAE_HMM_MAX_K) return -3;
  if (pair_batched != 0 && pair_batched != 1) return -4;
  if (!init_params) return -5;
  if (!pair_params) return -6;
  if (B == 0) return 0;
  if (!node_params) return -7;
  if (!states) return -8;
  if (!workspace) return -10;
  if (ws_bytes < svae_hmm_viterbi_workspace_bytes(B, T, K)) return -11;
  if (((uintptr_t)workspace & 15) != 0) return -12;   // back-pointer rows are read back 16 bytes at a time
  svae::ViterbiArgs a;
  a.B = B; a.T = T; a.K = K; a.pair_stride = pair_batched ? (long)K * K : 0;
  a.init_params = init_params; a.pair_params = pair_params; a.node_params = node_params;
  a.states = states; a.score = score; a.ws = (uint8_t*)workspace;
  hipStream_t s = (hipStream_t)stream;
  if (K > 32) {
    hipLaunchKernelGGL((svae::hmm_viterbi_wide_kernel<64>), dim3(B), dim3(64), 0, s, a);
    return hipGetLastError() == hipSuccess ? 0 : -1000;
  }
  if (K > 16) {
    hipLaunchKernelGGL((svae::hmm_viterbi_wide_kernel<32>), dim3(B), dim3(64), 0, s, a);
    return hipGetLastError() == hipSuccess ? 0 : -1000;
  }
  switch (K) {
#define SVAE_CASE(KK) case KK: return svae::launch_viterbi_row<KK>(a, s);
    SVAE_CASE(1) SVAE_CASE(2) SVAE_CASE(3) SVAE_CASE(4) SVAE_CASE(5) SVAE_CASE(6) SVAE_CASE(7)
    SVAE_CASE(8) SVAE_CASE(9) SVAE_CASE(10) SVAE_CASE(11) SVAE_CASE(12) SVAE_CASE(13)
    SVAE_CASE(14) SVAE_CASE(15) SVAE_CASE(16)
#undef SVAE_CASE
  }
  return -3;
}
