// hmm_viterbi_kernel.hpp -- the two Viterbi kernel templates (see hmm_viterbi.hip for the definition of the arithmetic,
// the mappings and the backtrace), shared by
//   hmm_viterbi.hip          RAGGED = false: one T per launch (16 row kernels + 2 wide kernels)
//   hmm_viterbi_ragged.hip   RAGGED = true:  per-sequence lengths (the same 18 shapes)
// RAGGED: sequence b occupies steps 0 .. L-1 of its (T, K) block, L = lengths[b] clamped to [1, T] (a value outside
// raises the status word).  delta freezes at L-1 (a select per row for K <= 16, the trip count itself for the wide
// kernel), node potentials are loaded at steps clamped to L-1 -- nothing stored at t >= L is ever read --, the
// backtrace starts at the sequence's own L-1 inside the same block structure (steps t >= L of a row's block map z to
// itself), and labels at t >= L are stored as -1.  Every RAGGED difference is an `if constexpr`: the uniform
// instantiations compile to what they were.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <type_traits>

#include "dpp.hpp"
#include "hmm_units.hpp"

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
struct ViterbiRaggedArgs : ViterbiArgs {
  const int32_t* lengths;     // (B)
  int32_t* info;              // status word: bit 0 = a length outside 1..T
};
template <bool RAGGED>
using ViterbiArgsT = std::conditional_t<RAGGED, ViterbiRaggedArgs, ViterbiArgs>;

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
template <int K, bool RAGGED>
__global__ __launch_bounds__(64) void hmm_viterbi_row_kernel(const ViterbiArgsT<RAGGED> a) {
  const int lane = threadIdx.x;
  const int c = lane & 15;
  const int brow = blockIdx.x * 4 + (lane >> 4);
  const bool valid = brow < a.B;                      // idle rows repeat the last sequence and store nothing
  const long b = valid ? brow : a.B - 1;
  const bool col = c < K;
  const int cc = col ? c : 0;
  const int T = a.T;
  const double NEG_INF = -__builtin_inf();
  // RAGGED: TL = the row's own length; TW = the longest of the wavefront's four rows (wave-uniform trip count)
  int TL = T, TW = T;
  if constexpr (RAGGED) {
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

  const double* pp = a.pair_params + b * a.pair_stride;
  double P[K];                                        // P[j] = pair[j][c]
  static_for<0, K>([&](auto j) { P[j] = pp[j * K + cc]; });
  const double* node = a.node_params + (b * T) * K + cc;
  uint8_t* psi = a.ws + (b * T) * 16 + c;

  double delta = col ? a.init_params[cc] + node[0] : NEG_INF;
  if (valid) psi[0] = 0;                              // (psi_0 is never followed; written so that every byte read is defined)

  auto load = [&](int t) -> double { return node[(long)(t < TL ? t : TL - 1) * K]; };
  double cur[VIT_AHEAD], nxt[VIT_AHEAD];
  static_for<0, VIT_AHEAD>([&](auto u) { cur[u] = load(1 + u); });
  for (int t0 = 1; t0 < TW; t0 += VIT_AHEAD) {
    static_for<0, VIT_AHEAD>([&](auto u) { nxt[u] = load(t0 + VIT_AHEAD + u); });
    static_for<0, VIT_AHEAD>([&](auto u) {
      const int t = t0 + u;
      if (t < TW) {                                   // (wave-uniform)
        double best = bcast<0>(delta) + P[0];
        int arg = 0;
        static_for<1, K>([&](auto j) {
          const double v = bcast<j>(delta) + P[j];
          const bool w = v > best;                    // strict: the first (lowest) j keeps a tie
          best = w ? v : best;
          arg = w ? (int)j : arg;
        });
        if constexpr (RAGGED) {
          const bool live = t < TL;                   // a row past its length keeps delta_{L-1} and stores nothing
          const double dn = col ? best + cur[u] : NEG_INF;
          delta = live ? dn : delta;
          if (valid && live) psi[(long)t * 16] = (uint8_t)arg;
        } else {
          delta = col ? best + cur[u] : NEG_INF;
          if (valid) psi[(long)t * 16] = (uint8_t)arg;
        }
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
    return rows[t < TL ? t : TL - 1];
  };
  int blk = (TW - 1) >> 4;
  uint4 q = load_row(blk);
  for (; blk >= 0; --blk) {
    const uint4 qn = load_row(blk > 0 ? blk - 1 : 0);
    const int t = blk * 16 + c;
    // steps beyond the chain: the identity map (z passes through)
    const unsigned long long map = t < TL ? vit_pack16(q) : 0xFEDCBA9876543210ull;
    int lab = 0;
    static_for<0, 16>([&](auto i) {
      constexpr int l = 15 - (int)i;
      lab = c == l ? z : lab;                         // z = the label of step blk*16 + l ...
      const unsigned long long m = vit_bcast_u64<l>(map);
      z = (int)((unsigned)(m >> (4 * z)) & 15u);      // ... and psi of that step leads to the step before
    });
    if (valid && t < TL) out[t] = lab;
    q = qn;
  }
  if constexpr (RAGGED) {
    // labels from the row's length on (after the last cross-lane operation: the trip count differs between rows)
    if (valid)
      for (int t = TL + c; t < T; t += 16) out[t] = -1;
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

template <int KP, bool RAGGED>
__global__ __launch_bounds__(64) void hmm_viterbi_wide_kernel(const ViterbiArgsT<RAGGED> a) {
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
  // RAGGED: TL = the sequence's own length (wave-uniform); arrays keep stride T
  int TL = T;
  if constexpr (RAGGED) {
    const int l = a.lengths[b];
    if ((l < 1 || l > T) && lane == 0) atomicOr(a.info, 1);
    TL = l < 1 ? 1 : (l > T ? T : l);
  }

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

  auto load = [&](int t) -> double { return nd[(long)(t < TL ? t : TL - 1) * K]; };
  constexpr int AHEAD = 4;
  double cur[AHEAD], nxt[AHEAD];
#pragma unroll
  for (int u = 0; u < AHEAD; ++u) cur[u] = load(1 + u);
  for (int t0 = 1; t0 < TL; t0 += AHEAD) {
#pragma unroll
    for (int u = 0; u < AHEAD; ++u) nxt[u] = load(t0 + AHEAD + u);
#pragma unroll
    for (int u = 0; u < AHEAD; ++u) {
      const int t = t0 + u;
      if (t < TL) {                                   // (wave-uniform)
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
    const int rows = TL - t0 < 64 ? TL - t0 : 64;
    const uint4* src = reinterpret_cast<const uint4*>(base + (long)t0 * KP);
    static_for<0, NQ>([&](auto r) {
      const int i = lane + 64 * (int)r;
      d.v[r] = src[i < rows * NQ ? i : 0];            // (pieces beyond the chain: never read back)
    });
    return d;
  };
  int t0 = ((TL - 1) >> 6) << 6;
  VitBlock<NQ> q = load_block(t0);
  for (; t0 >= 0; t0 -= 64) {
    const int rows = TL - t0 < 64 ? TL - t0 : 64;
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
  if constexpr (RAGGED) {
    for (int t = TL + lane; t < T; t += 64) out[t] = -1;
  }
}

// ---- host: the launch behind svae_hmm_viterbi_f64 (RAGGED = false) and svae_hmm_ragged_viterbi_f64 (RAGGED = true) ------
template <bool RAGGED>
static int launch_viterbi(const ViterbiArgsT<RAGGED>& a, hipStream_t s) {
  hmm_dispatch_k(
      a.K,
      [&](auto k) {
        hipLaunchKernelGGL((hmm_viterbi_row_kernel<k, RAGGED>), dim3((a.B + 3) / 4), dim3(64), 0, s, a);
        return 0;
      },
      [&](auto kp) {
        hipLaunchKernelGGL((hmm_viterbi_wide_kernel<kp, RAGGED>), dim3(a.B), dim3(64), 0, s, a);
        return 0;
      });
  return hipGetLastError() == hipSuccess ? 0 : -1000;
}

}  // namespace svae
