// hmm_sample_kernel.hpp -- the four kernel templates of HMM posterior sampling, forward filter + backward draw (see
// hmm_sample.hip for the definition of the arithmetic and the mappings), shared by
//   hmm_sample.hip          RAGGED = false: one T per launch (2 x (16 row kernels + 2 wide kernels))
//   hmm_sample_ragged.hip   RAGGED = true:  per-sequence lengths (the same 36 shapes)
// The filter kernels are the forward half of the one-directional E-step kernels (hmm_estep.hip: hmm_estep_kernel;
// hmm_estep_wide.hip), restated here: they store the filtered distribution alone, KP doubles per step, and nothing the
// backward pass of the E-step needs.  No code is shared with those units.
// Range (hmm_args.hpp, HMM_LOW; the E-step's contract): the filter kernels flag a sequence when a live component of a
// step's unnormalised message (sum_j a_{t-1}[j] P[j][k]) e_t[k] -- at t = 0 of exp(init + node_0 - max) -- falls below
// 1e-250, or a normaliser below 1e-200: one compare and one OR per step beside the dependent chain, no branch.  A
// flagged sequence's step-0 record is overwritten with -1 in every live lane; the log-space launch of
// hmm_sample_log.hip recognises it there (a scaled record sums to 1: it has a positive entry and none below 0),
// recomputes ALL of the sequence and leaves log a_t (normalised, <= 0, padding lanes -inf) in every record.  The draw
// kernels tell the two kinds of record apart by the first one they read, step L-1: no live entry > 0 = a log record.
// RAGGED: sequence b occupies steps 0 .. L-1 of its (T, K) block, L = lengths[b] clamped to [1, T] (a value outside
// raises the status word, in the filter launch).  The filter freezes at L-1, loads are clamped to L-1 -- nothing stored
// at t >= L is read --, the draw starts at the chain's own L-1 and labels at t >= L are stored as -1.  Every RAGGED
// difference is an `if constexpr`.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <type_traits>

#include "dpp.hpp"
#include "hmm_units.hpp"

namespace svae {

struct SampleArgs {
  int B, T, K, S;
  long pair_stride;           // doubles between sequences' pair params (0 = shared)
  const double* init_params;  // (K)
  const double* pair_params;  // (K,K) or (B,K,K)   [j][k] = j -> k
  const double* node_params;  // (B,T,K)
  const double* u;            // (B,S,T) uniforms
  int32_t* states;            // (B,S,T)
  double* logZ;               // (B) or nullptr
  double* ws;                 // (B,T,KP) filtered distributions a_t, padding lanes 0; a sequence redone in log space:
                              // log a_t <= 0, padding lanes -inf
};
struct SampleRaggedArgs : SampleArgs {
  const int32_t* lengths;     // (B)
  int32_t* info;              // status word: bit 0 = a length outside 1..T
};
template <bool RAGGED>
using SampleArgsT = std::conditional_t<RAGGED, SampleRaggedArgs, SampleArgs>;

constexpr double SMP_TINY = 1e-200;   // a normaliser below it (filter): the sequence is redone in log space; a weight
                                      // total below it (draw): that draw's weights in log space
constexpr int SMP_AHEAD = 8;          // filter: node potentials in flight, steps

// Maximum over the 16 lanes of a DPP row, in every lane (row_ror:8/4/2/1 on the two halves of the double)
template <int R>
__device__ __forceinline__ double smp_row_ror(double x) {
  const int lo = __builtin_amdgcn_update_dpp(0, __double2loint(x), 0x120 + R, 0xf, 0xf, false);
  const int hi = __builtin_amdgcn_update_dpp(0, __double2hiint(x), 0x120 + R, 0xf, 0xf, false);
  return __hiloint2double(hi, lo);
}
__device__ __forceinline__ double smp_row_max16(double x) {
  x = __builtin_fmax(x, smp_row_ror<8>(x));
  x = __builtin_fmax(x, smp_row_ror<4>(x));
  x = __builtin_fmax(x, smp_row_ror<2>(x));
  x = __builtin_fmax(x, smp_row_ror<1>(x));
  return x;
}
__device__ __forceinline__ double smp_wave_sum(double x) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) x += __shfl_xor(x, o, 64);
  return x;
}
__device__ __forceinline__ double smp_wave_max(double x) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) x = __builtin_fmax(x, __shfl_xor(x, o, 64));
  return x;
}
__device__ __forceinline__ void smp_lds_sync() {
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}
// lane `l` (wave-uniform) of a double
__device__ __forceinline__ double smp_readlane(double x, int l) {
  const int lo = __builtin_amdgcn_readlane(__double2loint(x), l);
  const int hi = __builtin_amdgcn_readlane(__double2hiint(x), l);
  return __hiloint2double(hi, lo);
}
__device__ __forceinline__ double smp_clamp01(double u) {
  u = u > 0.0 ? u : 0.0;                // (a NaN counts as 0)
  return u > 1.0 ? 1.0 : u;
}

// ---- filter, K <= 16: one DPP row per sequence ------------------------------------------------------------------------
template <int K, bool RAGGED>
__global__ __launch_bounds__(64) void hmm_filter_row_kernel(const SampleArgsT<RAGGED> a) {
  const int lane = threadIdx.x;
  const int c = lane & 15;
  const int brow = blockIdx.x * 4 + (lane >> 4);
  const bool valid = brow < a.B;                      // idle rows repeat the last sequence and store nothing
  const long b = valid ? brow : a.B - 1;
  const bool col = c < K;
  const int cc = col ? c : 0;
  const int T = a.T;
  const double NEG_INF = -__builtin_inf();
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

  // column c of the transition matrix, shifted by the matrix' maximum (the shift goes into logZ)
  const double* pp = a.pair_params + b * a.pair_stride;
  double P[K];
  double pmax = NEG_INF;
  static_for<0, K>([&](auto j) {
    const double v = pp[j * K + cc];
    P[j] = col ? v : NEG_INF;
    pmax = __builtin_fmax(pmax, P[j]);
  });
  pmax = smp_row_max16(pmax);
  static_for<0, K>([&](auto j) { P[j] = col ? exp(P[j] - pmax) : 0.0; });

  const double* node = a.node_params + (b * T) * K + cc;
  double* wsb = a.ws + (b * T) * 16 + c;
  double one = 1.0;
  double lzM = 1.0;            // product of the normalisers (mantissa) ...
  long lzE = 0;                // ... exponent
  double lzS = 0.0;            // sum of the subtracted maxima
  double alpha = 0.0;
  bool low = false, tiny = false;   // a message component (padding lanes too, masked at the end) / a normaliser left the range

  auto step = [&](auto first, int t, double ndraw) __attribute__((always_inline)) {
    constexpr bool FIRST = decltype(first)::value;
    const bool live = !RAGGED || t < TL;    // (a row past its length computes on its last step's data and keeps nothing)
    double nd = col ? ndraw : NEG_INF;
    if constexpr (FIRST) nd += col ? a.init_params[cc] : 0.0;
    const double m = smp_row_max16(nd);
    const double e = col ? exp_nonpos(nd - m) : 0.0;
    double pred;
    if constexpr (FIRST) {
      pred = col ? 1.0 : 0.0;
    } else {
      pred = 0.0;
      dpp_fence(alpha);
      static_for<0, K>([&](auto j) { mac_bc<j>(pred, alpha, P[j]); });     // sum_j a_{t-1}[j] P[j][k]
    }
    double al = pred * e;                   // the unnormalised message component
    double cs = 0.0;
    dpp_fence(al);
    static_for<0, K>([&](auto k) { mac_bc<k>(cs, al, one); });
    const double rc = rcp_nr(cs);
    const double shift = m + (FIRST ? 0.0 : pmax);
    // the range criterion (a NaN fails both compares); steps past the length never flag
    low = low || (live && !(al >= HMM_LOW));
    tiny = tiny || (live && !(cs > SMP_TINY));
    if constexpr (RAGGED) {
      alpha = live ? al * rc : alpha;
      if (valid && live) wsb[(long)t * 16] = alpha;
      lzM = live ? lzM * __builtin_amdgcn_frexp_mant(cs) : lzM;
      lzE += live ? __builtin_amdgcn_frexp_exp(cs) : 0;
      lzS = live ? lzS + shift : lzS;
      if ((t & 15) == 15) {
        lzE += live ? __builtin_amdgcn_frexp_exp(lzM) : 0;
        lzM = live ? __builtin_amdgcn_frexp_mant(lzM) : lzM;
      }
    } else {
      alpha = al * rc;
      if (valid) wsb[(long)t * 16] = alpha;
      lzM *= __builtin_amdgcn_frexp_mant(cs);
      lzE += __builtin_amdgcn_frexp_exp(cs);
      lzS += shift;
      if ((t & 15) == 15) { lzE += __builtin_amdgcn_frexp_exp(lzM); lzM = __builtin_amdgcn_frexp_mant(lzM); }
    }
  };

  auto load = [&](int t) -> double { return node[(long)(t < TL ? t : TL - 1) * K]; };
  step(std::true_type{}, 0, node[0]);
  double cur[SMP_AHEAD], nxt[SMP_AHEAD];
  static_for<0, SMP_AHEAD>([&](auto u) { cur[u] = load(1 + u); });
  for (int t0 = 1; t0 < TW; t0 += SMP_AHEAD) {
    static_for<0, SMP_AHEAD>([&](auto u) { nxt[u] = load(t0 + SMP_AHEAD + u); });
    static_for<0, SMP_AHEAD>([&](auto u) {
      const int t = t0 + u;
      if (t < TW) step(std::false_type{}, t, cur[u]);   // (wave-uniform)
    });
    static_for<0, SMP_AHEAD>([&](auto u) { cur[u] = nxt[u]; });
  }
  if (valid && c == 0 && a.logZ) a.logZ[b] = lzS + ::log(lzM) + (double)lzE * 0.6931471805599453094;
  // a flagged row marks its step-0 record for the log-space launch (which also rewrites logZ)
  const bool redo = ((unsigned)(__ballot((low && col) || tiny) >> (lane & 48)) & 0xffffu) != 0;
  if (valid && redo && col) wsb[0] = -1.0;
}

// ---- filter, 17 <= K <= 64: one wavefront per sequence ----------------------------------------------------------------
template <int KP, bool RAGGED>
__global__ __launch_bounds__(64) void hmm_filter_wide_kernel(const SampleArgsT<RAGGED> a) {
  __shared__ double line[64];
  const int lane = threadIdx.x;
  const int K = a.K, T = a.T;
  const long b = blockIdx.x;
  const bool st = lane < K;
  const int cc = st ? lane : 0;
  const double NEG_INF = -__builtin_inf();
  int TL = T;
  if constexpr (RAGGED) {
    const int l = a.lengths[b];
    if ((l < 1 || l > T) && lane == 0) atomicOr(a.info, 1);
    TL = l < 1 ? 1 : (l > T ? T : l);
  }
  const double* pp = a.pair_params + b * a.pair_stride;
  const double* nd = a.node_params + (b * T) * K + cc;
  double* wsb = a.ws + (b * T) * KP + (lane < KP ? lane : 0);

  double pmax = NEG_INF;
  double Pc[KP];                                      // Pc[i] = exp(pair[i][lane] - max); padding: 0
#pragma unroll
  for (int i = 0; i < KP; ++i) {
    const double v = pp[(i < K ? i : 0) * K + cc];
    Pc[i] = (st && i < K) ? v : NEG_INF;
    pmax = __builtin_fmax(pmax, Pc[i]);
  }
  pmax = smp_wave_max(pmax);
#pragma unroll
  for (int i = 0; i < KP; ++i) Pc[i] = (st && i < K) ? exp(Pc[i] - pmax) : 0.0;

  double lzM, lzS, al;
  long lzE;
  bool flag;                                          // this lane saw the sequence leave the range of the scaled recursion
  {
    const double x = st ? a.init_params[cc] + nd[0] : NEG_INF;
    const double m = smp_wave_max(x);
    const double w = (st && m > NEG_INF) ? exp(x - m) : 0.0;
    const double s = smp_wave_sum(w);
    flag = (st && !(w >= HMM_LOW)) || !(s > SMP_TINY);
    al = w * rcp_nr(s);
    lzS = m;
    lzM = __builtin_amdgcn_frexp_mant(s);
    lzE = __builtin_amdgcn_frexp_exp(s);
    if (lane < KP) wsb[0] = al;
  }
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
        const double x = st ? cur[u] : NEG_INF;
        __builtin_amdgcn_wave_barrier();
        line[lane] = al;
        smp_lds_sync();
        const double m = smp_wave_max(x);
        const double e = st ? exp_nonpos(x - m) : 0.0;
        double v0 = 0.0, v1 = 0.0;
#pragma unroll
        for (int i = 0; i < KP; i += 2) {
          v0 = __builtin_fma(line[i], Pc[i], v0);
          v1 = __builtin_fma(line[i + 1], Pc[i + 1], v1);
        }
        const double w = (v0 + v1) * e;               // the unnormalised message component
        const double cs = smp_wave_sum(w);
        const double shift = m + pmax;
        flag = flag || (st && !(w >= HMM_LOW)) || !(cs > SMP_TINY);    // (a NaN fails both compares)
        al = w * rcp_nr(cs);
        lzM *= __builtin_amdgcn_frexp_mant(cs);
        lzE += __builtin_amdgcn_frexp_exp(cs);
        lzS += shift;
        if ((t & 15) == 15) { lzE += __builtin_amdgcn_frexp_exp(lzM); lzM = __builtin_amdgcn_frexp_mant(lzM); }
        if (lane < KP) wsb[(long)t * KP] = al;
      }
    }
#pragma unroll
    for (int u = 0; u < AHEAD; ++u) cur[u] = nxt[u];
  }
  if (lane == 0 && a.logZ) a.logZ[b] = lzS + ::log(lzM) + (double)lzE * 0.6931471805599453094;
  // a flagged sequence marks its step-0 record for the log-space launch (which also rewrites logZ)
  if (__any(flag) && st) wsb[0] = -1.0;
}

// ---- draw, K <= 16: one DPP row per (sequence, sample) ----------------------------------------------------------------
// Lane k holds row k of exp(pair - M); z_{t+1} lives as a one-hot row vector `oh`, so the column of the matrix the weights
// need is K broadcast multiply-accumulates, and the index-ordered cumulative sum K masked broadcast adds.  No memory
// access on the serial chain depends on z: a_t and u_t of the next 16 steps are in flight during the current 16.
template <int K, bool RAGGED>
__global__ __launch_bounds__(64) void hmm_draw_row_kernel(const SampleArgsT<RAGGED> a) {
  const int lane = threadIdx.x;
  const int c = lane & 15;
  const long R = (long)a.B * a.S;
  const long rrow = (long)blockIdx.x * 4 + (lane >> 4);
  const bool valid = rrow < R;                        // idle rows repeat the last chain and store nothing
  const long r = valid ? rrow : R - 1;
  const long b = r / a.S;                             // (a wavefront's rows mostly share a sequence and a length)
  const bool col = c < K;
  const int cc = col ? c : 0;
  const int T = a.T;
  const double NEG_INF = -__builtin_inf();
  int TL = T, TW = T;
  if constexpr (RAGGED) {
    const int l = a.lengths[b];
    TL = l < 1 ? 1 : (l > T ? T : l);
    int m = TL;
    const int m1 = __shfl_xor(m, 16, 64);
    m = m1 > m ? m1 : m;
    const int m2 = __shfl_xor(m, 32, 64);
    m = m2 > m ? m2 : m;
    TW = __builtin_amdgcn_readfirstlane(m);
  }

  const double* pp = a.pair_params + b * a.pair_stride;
  double E[K];                                        // E[j] = exp(pair[c][j] - M)
  double ge[K];                                       // ge[j] = 1 if c >= j: lane c's cumulative sum takes w[j]
  double pmax = NEG_INF;
  static_for<0, K>([&](auto j) {
    const double v = pp[cc * K + j];
    E[j] = col ? v : NEG_INF;
    pmax = __builtin_fmax(pmax, E[j]);
    ge[j] = c >= (int)j ? 1.0 : 0.0;
  });
  pmax = smp_row_max16(pmax);
  static_for<0, K>([&](auto j) { E[j] = col ? exp(E[j] - pmax) : 0.0; });

  const double* af = a.ws + (b * T) * 16 + c;
  const double* ur = a.u + r * T;
  int32_t* out = a.states + r * T;
  const int rsh = lane & 48;                          // this row's bits of a ballot

  auto load_a = [&](int blk, double (&A)[16]) {
    static_for<0, 16>([&](auto i) {
      const int t = blk * 16 + (int)i;
      A[i] = af[(long)(t < TL ? t : TL - 1) * 16];
    });
  };
  auto load_u = [&](int blk) -> double {
    const int t = blk * 16 + c;
    return ur[t < TL ? t : TL - 1];
  };

  double oh = 0.0;                                    // one-hot z_{t+1} (unused at the chain's last step)
  int z = 0;
  int blk = (TW - 1) >> 4;
  double A[16], An[16];
  load_a(blk, A);
  double uv = load_u(blk);
  // the kind of this row's record, from the first one the draw reads: a scaled a_t sums to 1, log a_t is <= 0 throughout
  // (step blk 16 + 15 is at or past the row's last one: A[15] is the record of step TL-1)
  const bool islog = ((unsigned)(__ballot(col && A[15] > 0.0) >> rsh) & 0xffffu) == 0;
  for (; blk >= 0; --blk) {
    const int bn = blk > 0 ? blk - 1 : 0;
    load_a(bn, An);
    const double uvn = load_u(bn);
    int lab = 0;
    static_for<0, 16>([&](auto ii) {
      constexpr int i = 15 - (int)ii;
      const int t = blk * 16 + i;
      if (t < TW) {                                   // (wave-uniform)
        const bool live = !RAGGED || t < TL;
        const bool last = t == TL - 1;                // the chain's last step: the weights are a_t alone
        double colv = 0.0;
        dpp_fence(oh);
        static_for<0, K>([&](auto j) { mac_bc<j>(colv, oh, E[j]); });      // exp(pair[c][z_{t+1}] - M)
        colv = last ? 1.0 : colv;
        double w = col ? A[i] * colv : 0.0;
        double C = 0.0;
        dpp_fence(w);
        static_for<0, K>([&](auto j) { mac_bc<j>(C, w, ge[j]); });         // C[c] = w[0] + .. + w[c], in index order
        double tot = bcast_fenced<K - 1>(C);
        // (a row whose record is log a_t has no positive weight here: its total is <= 0 or NaN at every step, the last
        //  one included, where a scaled row's total is 1 -- the one compare of the chain serves both)
        const bool under = live && !(tot >= SMP_TINY);
        if (__any(under)) {
          // the weights of this draw in log space (wave-uniform branch; every step of a row whose record is log a_t,
          // else rare); the matrix entry is read again
          const int zc = (z & 15) < K ? (z & 15) : K - 1;
          const double la = islog ? A[i] : (A[i] > 0.0 ? ::log(A[i]) : NEG_INF);
          const double x = col ? la + (last ? 0.0 : pp[cc * K + zc]) : NEG_INF;
          const double mx = smp_row_max16(x);
          const double w2 = (col && mx > NEG_INF) ? exp(x - mx) : 0.0;
          double C2 = 0.0;
          static_for<0, K>([&](auto j) { C2 = __builtin_fma(bcast<j>(w2), ge[j], C2); });
          const double tot2 = bcast<K - 1>(C2);
          C = under ? C2 : C;
          tot = under ? tot2 : tot;
        }
        const double thr = smp_clamp01(bcast<i>(uv)) * tot;
        // (C <= thr) is a prefix of the row; (C < tot) keeps lane K-1 out, so the count is at most K-1 and, when the
        // product rounded up to the total, the lowest state that reaches the total is taken
        const int ind = (col && C <= thr && C < tot) ? 1 : 0;
        const int indp = __builtin_amdgcn_update_dpp(1, ind, 0x111, 0xf, 0xf, false);   // row_shr:1, lane 0 keeps 1
        const double ohn = (double)(indp - ind);
        const unsigned long long bm = __ballot(ind);
        const int zn = __popc((unsigned)(bm >> rsh) & 0xffffu) & 15;
        if constexpr (RAGGED) {
          oh = live ? ohn : oh;
          z = live ? zn : z;
        } else {
          oh = ohn;
          z = zn;
        }
        lab = c == i ? z : lab;
      }
    });
    const int t = blk * 16 + c;
    if (valid && t < TL) out[t] = lab;
    static_for<0, 16>([&](auto i) { A[i] = An[i]; });
    uv = uvn;
  }
  if constexpr (RAGGED) {
    // labels from the chain's length on (after the last cross-lane operation)
    if (valid)
      for (int t = TL + c; t < T; t += 16) out[t] = -1;
  }
}

// ---- draw, 17 <= K <= 64: one wavefront per (sequence, sample) ----------------------------------------------------------
// AT[z][k] = exp(pair[k][z] - M) in LDS: lane k reads its entry of the wave-uniform row z without bank conflicts.  The
// index-ordered cumulative sum goes through an LDS line with KP zeros in front of the weights: lane k adds the KP entries
// that end at its own, i.e. zeros and then w[0], w[1], .., w[k] in that order (unit stride across lanes, no masks).
template <int KP, bool RAGGED>
__global__ __launch_bounds__(64) void hmm_draw_wide_kernel(const SampleArgsT<RAGGED> a) {
  __shared__ double AT[KP * KP];
  __shared__ double line[128];
  const int lane = threadIdx.x;
  const int K = a.K, T = a.T;
  const long r = blockIdx.x;
  const long b = r / a.S;
  const bool st = lane < K;
  const int cc = st ? lane : 0;
  const int lk = lane & (KP - 1);
  const double NEG_INF = -__builtin_inf();
  int TL = T;
  if constexpr (RAGGED) {
    const int l = a.lengths[b];
    TL = l < 1 ? 1 : (l > T ? T : l);
  }
  const double* pp = a.pair_params + b * a.pair_stride;
  // lane = destination state z, loop over source states k: coalesced reads of row k
  double pmax = NEG_INF;
  for (int k = 0; k < K; ++k) pmax = __builtin_fmax(pmax, st ? pp[k * K + cc] : NEG_INF);
  pmax = smp_wave_max(pmax);
  for (int k = 0; k < KP; ++k) {
    const double v = (st && k < K) ? exp(pp[k * K + cc] - pmax) : 0.0;
    if (lane < KP) AT[lane * KP + k] = v;
  }
  line[lane] = 0.0;
  line[64 + lane] = 0.0;
  smp_lds_sync();

  const double* af = a.ws + (b * T) * KP + lk;
  const double* ur = a.u + r * T;
  int32_t* out = a.states + r * T;

  auto cumsum = [&](double w) -> double {
    __builtin_amdgcn_wave_barrier();
    line[KP + lane] = w;                              // (lanes >= K write 0)
    smp_lds_sync();
    double C = 0.0;
#pragma unroll
    for (int m = 0; m < KP; ++m) C += line[lane + 1 + m];
    return C;
  };
  auto load_a = [&](int t) -> double { return af[(long)(t < 0 ? 0 : (t < TL ? t : TL - 1)) * KP]; };
  constexpr int AHEAD = 8;
  int z = 0;
  bool islog = false;                                 // (wave-uniform) the chain's record is log a_t
  const int tfirst = ((TL - 1) >> 6) << 6;
  for (int t0 = tfirst; t0 >= 0; t0 -= 64) {
    const int tu = t0 + lane;
    const double uv = ur[tu < TL ? tu : TL - 1];
    int lab = 0;
    double cur[AHEAD], nxt[AHEAD];
#pragma unroll
    for (int q = 0; q < AHEAD; ++q) cur[q] = load_a(t0 + 56 + q);
    // the kind of this chain's record, from the first one the draw reads: a scaled a_t sums to 1, log a_t is <= 0
    // throughout (step tfirst + 63 is at or past the chain's last one: the load is the record of step TL-1)
    if (t0 == tfirst) islog = !__any(st && cur[AHEAD - 1] > 0.0);
    for (int i0 = 56; i0 >= 0; i0 -= AHEAD) {
#pragma unroll
      for (int q = 0; q < AHEAD; ++q) nxt[q] = load_a(t0 + i0 - AHEAD + q);
#pragma unroll
      for (int qq = 0; qq < AHEAD; ++qq) {
        const int q = AHEAD - 1 - qq;
        const int l = i0 + q;
        const int t = t0 + l;
        if (t < TL) {                                 // (wave-uniform)
          const bool last = t == TL - 1;
          const double colv = last ? 1.0 : AT[(z & (KP - 1)) * KP + lk];
          double w = st ? cur[q] * colv : 0.0;
          double C = cumsum(w);
          double tot = smp_readlane(C, K - 1);
          // (a chain whose record is log a_t has no positive weight here: its total is <= 0 or NaN at every step, the
          //  last one included, where a scaled chain's total is 1 -- the one compare of the chain serves both)
          if (!(tot >= SMP_TINY)) {
            // the weights of this draw in log space (wave-uniform branch; every step of a chain whose record is log a_t,
            // else rare); the matrix entry is read again
            const int zc = z < K ? z : K - 1;
            const double la = islog ? cur[q] : (cur[q] > 0.0 ? ::log(cur[q]) : NEG_INF);
            const double x = st ? la + (last ? 0.0 : pp[cc * K + zc]) : NEG_INF;
            const double mx = smp_wave_max(x);
            w = (st && mx > NEG_INF) ? exp(x - mx) : 0.0;
            C = cumsum(w);
            tot = smp_readlane(C, K - 1);
          }
          const double thr = smp_clamp01(smp_readlane(uv, l)) * tot;
          const unsigned long long bm = __ballot(st && C <= thr && C < tot);
          z = __builtin_amdgcn_readfirstlane(__popcll(bm)) & (KP - 1);
          lab = lane == l ? z : lab;
        }
      }
#pragma unroll
      for (int q = 0; q < AHEAD; ++q) cur[q] = nxt[q];
    }
    if (tu < TL) out[tu] = lab;
  }
  if constexpr (RAGGED) {
    for (int t = TL + lane; t < T; t += 64) out[t] = -1;
  }
}

}  // namespace svae

// hmm_sample_log.hip: the log-space filter, at work on the sequences the scaled filter flagged
extern "C" int svae_hmm_sample_log_launch(const svae::SampleArgs* a, void* stream);
extern "C" int svae_hmm_sample_log_ragged_launch(const svae::SampleRaggedArgs* a, void* stream);

namespace svae {

// ---- host: the three launches behind svae_hmm_sample_f64 (RAGGED = false) and svae_hmm_ragged_sample_f64 (RAGGED = true):
// the scaled filter, the log-space filter over what it flagged, the draw
template <bool RAGGED>
static int launch_sample(const SampleArgsT<RAGGED>& a, hipStream_t s) {
  auto log_filter = [&] {
    if constexpr (RAGGED) svae_hmm_sample_log_ragged_launch(&a, s);
    else svae_hmm_sample_log_launch(&a, s);
  };
  const long R = (long)a.B * a.S;
  hmm_dispatch_k(
      a.K,
      [&](auto k) {
        hipLaunchKernelGGL((hmm_filter_row_kernel<k, RAGGED>), dim3((a.B + 3) / 4), dim3(64), 0, s, a);
        log_filter();
        hipLaunchKernelGGL((hmm_draw_row_kernel<k, RAGGED>), dim3((unsigned)((R + 3) / 4)), dim3(64), 0, s, a);
        return 0;
      },
      [&](auto kp) {
        hipLaunchKernelGGL((hmm_filter_wide_kernel<kp, RAGGED>), dim3(a.B), dim3(64), 0, s, a);
        log_filter();
        hipLaunchKernelGGL((hmm_draw_wide_kernel<kp, RAGGED>), dim3((unsigned)R), dim3(64), 0, s, a);
        return 0;
      });
  return hipGetLastError() == hipSuccess ? 0 : -1000;
}

}  // namespace svae
