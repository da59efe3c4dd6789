// hmm_estep_vjp_kernel.hpp -- the kernel templates of the reverse-mode derivative of the HMM E-step (see hmm_estep_vjp.hip
// for the arithmetic), shared by
//   hmm_estep_vjp.hip          RAGGED = false: one T per launch
//   hmm_estep_vjp_ragged.hip   RAGGED = true:  per-sequence lengths
// Two mappings, both one-directional (a forward sweep, then a backward sweep, in ONE launch):
//   hmm_vjp_row_kernel<K>       K <= 16: one 16-lane DPP row per sequence, four per wavefront, scaled recursions; the
//                               matrix products are broadcast multiply-adds (dpp.hpp: mac_bc)
//   hmm_vjp_wide_kernel<KP, LOGSPACE>   one wavefront per sequence, lane = state.  KP = 32 / 64: the scaled kernels of
//                               17 <= K <= 64 and their log-space redo; KP = 16, LOGSPACE: the redo behind the row kernels
// The forward sweep stores a_t and r_t, 2 KP doubles per step (padding lanes 0); the backward sweep carries b_t and s_t,
// emits g_node per step and accumulates g_pair in registers (row) or in LDS (wide, next to V).  Every address is a
// function of the step alone.  The backward message is renormalised so that sum_k a_t[k] b_t[k] = 1: the marginals are
// a_t o b_t and no normaliser of the forward sweep is kept.  (On the log-space route the records hold log a_t, padding
// lanes -1e300.)
// Range (hmm_args.hpp, HMM_LOW): the scaled kernels raise a sequence's route flag when a live component of an
// unnormalised message falls below 1e-250 or a normaliser below 1e-200, in either sweep; the LOGSPACE launch behind them
// recomputes exactly the flagged sequences, all of each, with every weight a log-space softmax.
// RAGGED: sequence b occupies steps 0 .. L-1, L = lengths[b] clamped to [1, T] (a value outside raises the status word, in
// the scaled launch); loads are clamped to L-1, g_node[b, t >= L] is stored as 0.  Every RAGGED difference is an
// `if constexpr`.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <type_traits>

#include "dpp.hpp"
#include "hmm_units.hpp"
#include "hmm_sample_kernel.hpp"      // smp_row_max16, smp_wave_sum, smp_wave_max, smp_lds_sync

namespace svae {

struct VjpArgs {
  int B, T, K;
  long pair_stride;           // doubles between sequences' pair params (0 = shared)
  const double* init_params;  // (K)
  const double* pair_params;  // (K,K) or (B,K,K)   [i][j] = i -> j
  const double* node_params;  // (B,T,K)
  const double* g_logZ;       // (B)      cotangent of logZ, or nullptr (= 0)
  const double* g_init;       // (B,K)    cotangent of E_init   (u0), or nullptr
  const double* g_trans;      // (B,K,K)  cotangent of E_trans  (V), or nullptr
  const double* g_states;     // (B,T,K)  cotangent of E_states (W), or nullptr
  double* d_init;             // (B,K)
  double* d_pair;             // (B,K,K)
  double* d_node;             // (B,T,K)
  double* ws;                 // (B,T,2 KP) records [a_t | r_t], then (B) route flags
};
struct VjpRaggedArgs : VjpArgs {
  const int32_t* lengths;     // (B)
  int32_t* info;              // status word: bit 0 = a length outside 1..T
};
template <bool RAGGED>
using VjpArgsT = std::conditional_t<RAGGED, VjpRaggedArgs, VjpArgs>;

constexpr size_t vjp_ws_doubles(long B, long T, int K) { return (size_t)(B * T * 2 * hmm_kp(K) + B); }

// Between two walks over the same line: the second reads LDS again instead of keeping the first one's KP values (or the
// KP sums made of them) in registers
__device__ __forceinline__ void vjp_reread() { asm volatile("" ::: "memory"); }

// ---- K <= 16: one DPP row per sequence, scaled ------------------------------------------------------------------------
template <int K, bool RAGGED>
__global__ __launch_bounds__(64) void hmm_vjp_row_kernel(const VjpArgsT<RAGGED> a) {
  const int lane = threadIdx.x;
  const int c = lane & 15;
  const int brow = blockIdx.x * 4 + (lane >> 4);
  const bool valid = brow < a.B;                      // idle rows repeat the last sequence and store nothing
  const long b = valid ? brow : a.B - 1;
  const bool col = c < K;
  const int cc = col ? c : 0;
  const int T = a.T;
  const int rsh = lane & 48;                          // this row's bits of a ballot
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

  const double* pp = a.pair_params + b * a.pair_stride;
  const double* Vp = a.g_trans ? a.g_trans + b * K * K : nullptr;
  const double* node = a.node_params + (b * T) * K + cc;
  const double* Wp = a.g_states ? a.g_states + (b * T) * K + cc : nullptr;
  double* wsb = a.ws + (b * T) * 32 + c;
  const double gl = a.g_logZ ? a.g_logZ[b] : 0.0;
  double one = 1.0;
  bool flag = false;

  // ---- forward sweep: column c of exp(pair - max) and of its product with V ------------------------------------------
  double alpha = 0.0, r = 0.0;
  {
    double P[K], PV[K];
    double pmax = NEG_INF;
    static_for<0, K>([&](auto j) {
      P[j] = col ? pp[j * K + cc] : NEG_INF;
      pmax = __builtin_fmax(pmax, P[j]);
    });
    pmax = smp_row_max16(pmax);
    static_for<0, K>([&](auto j) {
      P[j] = col ? exp(P[j] - pmax) : 0.0;
      PV[j] = P[j] * (Vp ? Vp[j * K + cc] : 0.0);
    });

    auto load_n = [&](int t) -> double { return node[(long)(t < TL ? t : TL - 1) * K]; };
    auto load_w = [&](int t) -> double { return Wp ? Wp[(long)(t < TL ? t : TL - 1) * K] : 0.0; };
    auto step = [&](auto first, int t, double ndraw, double wraw) __attribute__((always_inline)) {
      constexpr bool FIRST = decltype(first)::value;
      const bool live = !RAGGED || t < TL;
      double nd = col ? ndraw : NEG_INF;
      if constexpr (FIRST) nd += col ? a.init_params[cc] : 0.0;
      const double m = smp_row_max16(nd);
      const double e = col ? exp_nonpos(nd - m) : 0.0;
      double pred, n1;
      if constexpr (FIRST) {
        pred = col ? 1.0 : 0.0;
        n1 = (col && a.g_init) ? a.g_init[b * K + cc] : 0.0;
      } else {
        pred = 0.0;
        n1 = 0.0;
        double ar = alpha * r;
        dpp_fence(alpha);
        dpp_fence(ar);
        static_for<0, K>([&](auto j) {
          mac_bc<j>(pred, alpha, P[j]);               // sum_i a_{t-1}[i] P[i][c]
          mac_bc<j>(n1, ar, P[j]);                    // sum_i a_{t-1}[i] P[i][c] (r_{t-1}[i] + V[i][c])
          mac_bc<j>(n1, alpha, PV[j]);
        });
      }
      double al = pred * e;
      double cs = 0.0;
      dpp_fence(al);
      static_for<0, K>([&](auto k) { mac_bc<k>(cs, al, one); });
      const double rc = rcp_nr(cs);
      flag = flag || (live && ((col && !(al >= HMM_LOW)) || !(cs > HMM_WIDE_TINY)));
      const double rn = col ? (pred > 0.0 ? n1 * rcp_nr(pred) : 0.0) + wraw : 0.0;
      alpha = live ? al * rc : alpha;
      r = live ? rn : r;
      if (valid && live) {
        wsb[(long)t * 32] = alpha;
        wsb[(long)t * 32 + 16] = r;
      }
    };
    double nn = load_n(1), wn = load_w(1);
    step(std::true_type{}, 0, node[0], Wp ? Wp[0] : 0.0);
    for (int t = 1; t < TW; ++t) {
      const double nc = nn, wc = wn;
      nn = load_n(t + 1);
      wn = load_w(t + 1);
      step(std::false_type{}, t, nc, wc);
    }
  }
  double Ephi = 0.0;                                  // E[phi] = sum_k a_{L-1}[k] r_{L-1}[k]
  {
    double arl = alpha * r;
    dpp_fence(arl);
    static_for<0, K>([&](auto k) { mac_bc<k>(Ephi, arl, one); });
  }
  const double gE = gl - Ephi;

  // ---- backward sweep: row c of the same two matrices; row c of g_pair -----------------------------------------------
  double Pr[K], PVr[K], acc[K];
  {
    double pmax = NEG_INF;
    static_for<0, K>([&](auto j) {
      Pr[j] = col ? pp[cc * K + j] : NEG_INF;
      pmax = __builtin_fmax(pmax, Pr[j]);
    });
    pmax = smp_row_max16(pmax);
    static_for<0, K>([&](auto j) {
      Pr[j] = col ? exp(Pr[j] - pmax) : 0.0;
      PVr[j] = Pr[j] * (Vp ? Vp[cc * K + j] : 0.0);
      acc[j] = 0.0;
    });
  }
  double* dn = a.d_node + (b * T) * K + cc;
  auto clampt = [&](int t) -> long { return t < TL ? t : TL - 1; };
  auto load_n1 = [&](int t) -> double { return node[clampt(t + 1) * K]; };
  auto load_w1 = [&](int t) -> double { return Wp ? Wp[clampt(t + 1) * K] : 0.0; };
  auto load_a = [&](int t) -> double { return wsb[clampt(t < 0 ? 0 : t) * 32]; };
  auto load_r = [&](int t) -> double { return wsb[clampt(t < 0 ? 0 : t) * 32 + 16]; };
  double bt = col ? 1.0 : 0.0, s = 0.0;               // b_{t+1}, s_{t+1}
  double pn = load_n1(TW - 1), pw = load_w1(TW - 1), pa = load_a(TW - 1), pr = load_r(TW - 1);
  for (int t = TW - 1; t >= 0; --t) {
    const double ndn = pn, wn1 = col ? pw : 0.0, at = pa, rt = pr;
    pn = load_n1(t > 0 ? t - 1 : 0);
    pw = load_w1(t > 0 ? t - 1 : 0);
    pa = load_a(t - 1);
    pr = load_r(t - 1);
    const bool live = t < TL;
    const bool inner = t < TL - 1;                    // (t = L-1: b = 1, s = 0, no transition out of it)
    const double nd = col ? ndn : NEG_INF;
    const double m = smp_row_max16(nd);
    const double e = col ? exp_nonpos(nd - m) : 0.0;
    double u = inner ? e * bt : 0.0;                  // (e o b)_{t+1}
    double y = inner ? u * (wn1 + s) : 0.0;
    double braw = 0.0, num = 0.0;
    dpp_fence(u);
    dpp_fence(y);
    static_for<0, K>([&](auto j) {
      mac_bc<j>(braw, u, Pr[j]);                      // sum_j P[c][j] u[j]
      mac_bc<j>(num, y, Pr[j]);                       // sum_j P[c][j] u[j] (V[c][j] + W[t+1][j] + s_{t+1}[j])
      mac_bc<j>(num, u, PVr[j]);
    });
    flag = flag || (inner && col && !(braw >= HMM_LOW));
    braw = inner ? braw : (col ? 1.0 : 0.0);
    double ab = at * braw;
    double Z = 0.0;
    dpp_fence(ab);
    static_for<0, K>([&](auto k) { mac_bc<k>(Z, ab, one); });
    flag = flag || (live && !(Z > HMM_WIDE_TINY));
    const double rz = rcp_nr(Z);
    const double sn = braw > 0.0 ? num * rcp_nr(braw) : 0.0;
    const double bn = braw * rz;
    const double gn = (at * bn) * (gE + rt + sn);     // gamma_t (g + E[phi | z_t] - E[phi])
    if (valid && live && col) {
      dn[(long)t * K] = gn;
      if (t == 0) a.d_init[b * K + cc] = gn;
    }
    const double a0 = inner ? at * rz : 0.0;
    const double cA = a0 * (gE + rt);
    static_for<0, K>([&](auto j) {
      const double c1 = __builtin_fma(cA, Pr[j], a0 * PVr[j]);
      const double c2 = a0 * Pr[j];
      mac_bc<j>(acc[j], u, c1);                       // xi_t[c][j] (g - E[phi] + r_t[c] + V[c][j] + W[t+1][j] + s_{t+1}[j])
      mac_bc<j>(acc[j], y, c2);
    });
    bt = live ? bn : bt;
    s = live ? sn : s;
  }
  if (valid && col) {
    double* dp = a.d_pair + (b * K + cc) * K;
    static_for<0, K>([&](auto j) { dp[j] = acc[j]; });
  }
  if constexpr (RAGGED) {
    if (valid && col)
      for (int t = TL; t < T; ++t) dn[(long)t * K] = 0.0;
  }
  const unsigned long long fm = __ballot(flag);
  if (valid && c == 0) a.ws[(long)a.B * T * 32 + b] = ((fm >> rsh) & 0xffffull) ? 1.0 : 0.0;
}

// ---- one wavefront per sequence, lane = state --------------------------------------------------------------------------
// Registers hold the transition matrix alone -- its column `lane` in the forward sweep, its row `lane` in the backward one
// (KP doubles per lane) -- up to KP = 32; at KP = 64 those 128 registers, half of them reached through copies, leave the
// unrolled walks short (hipcc spills), so the matrix goes to LDS as well and the walks are unrolled by 8.  V and g_pair
// live in LDS as KP x 64 arrays indexed [other state][lane]: a lane only ever touches its own column of them, without
// bank conflicts, without a barrier and (every lane has a column) without a branch.  The vectors that multiply the
// matrix are published through two 64-double lines and read back as broadcasts.
template <int KP, bool LOGSPACE, bool RAGGED>
__global__ __launch_bounds__(64) void hmm_vjp_wide_kernel(const VjpArgsT<RAGGED> a) {
  static_assert(KP == 32 || KP == 64 || (KP == 16 && LOGSPACE), "KP = 16: the log-space pass behind the row kernels");
  constexpr int REC = 2 * KP;
  constexpr double NEG_BIG = -1.0e300;
  __shared__ double lineA[64], lineB[64];
  __shared__ double Vs[KP * 64];                      // forward: V[i][lane] at [i]; backward: V[lane][j] at [j]  (scaled: P o V)
  constexpr bool PREG = KP <= 32;                     // the transition matrix in registers
  constexpr int UNR = PREG ? KP : 8;                  // (register arrays need their walks unrolled in full)
  __shared__ double Ps[PREG ? 1 : KP * 64];           // else here, laid out as V
  __shared__ double accT[KP * 64];                    // g_pair[lane][j] at [j]
  const int lane = threadIdx.x;
  const int K = a.K, T = a.T;
  const long b = blockIdx.x;
  const bool st = lane < K;
  const bool lp = lane < KP;
  const int cc = st ? lane : 0;
  const int lk = lp ? lane : 0;
  double* flagp = a.ws + (long)a.B * T * REC + b;
  int TL = T;
  if constexpr (RAGGED) {
    const int l = a.lengths[b];
    TL = l < 1 ? 1 : (l > T ? T : l);
    if constexpr (!LOGSPACE) {
      if ((l < 1 || l > T) && lane == 0) atomicOr(a.info, 1);
      double* tail = a.d_node + b * T * K;
      for (long q = (long)TL * K + lane; q < (long)T * K; q += 64) tail[q] = 0.0;
    }
  }
  if constexpr (LOGSPACE) {
    if (*flagp == 0.0) return;                        // not flagged by the scaled pass
  }
  const double* pp = a.pair_params + b * a.pair_stride;
  const bool hasV = a.g_trans != nullptr;
  const double* Vq = hasV ? a.g_trans + b * K * K : pp;            // (no cotangent: a readable address, selected away)
  const double* nd = a.node_params + (b * T) * K + cc;
  const double* Wp = a.g_states ? a.g_states + (b * T) * K + cc : nullptr;
  double* wsb = a.ws + (b * T) * REC + lk;
  double* Vl = Vs + lane;
  double* accl = accT + lane;
  double* Pl = PREG ? accl : Ps + lane;               // where `stage` leaves the matrix
  double Pq[PREG ? KP : 1];
  auto PM = [&](int o) -> double {
    if constexpr (PREG) return Pq[o];
    else return Pl[o * 64];
  };
  const double gl = a.g_logZ ? a.g_logZ[b] : 0.0;

  auto publish2 = [&](double x, double y) {
    __builtin_amdgcn_wave_barrier();
    lineA[lane] = x;
    lineB[lane] = y;
    smp_lds_sync();
  };

  // Entry [o][lane] of the transition matrix -- pair[o sr + lane sl], scaled: exp(. - max) -- goes to this lane's column of
  // Pl (PREG: the accumulator array, on its way into registers), the same entry of V (scaled: of P o V) into its own array.
  // Rolled loops: the 2 KP loads of an unrolled one are issued together and do not fit the register file.
  auto stage = [&](int sr, int sl) {
    double pmax = NEG_BIG;
#pragma unroll 4
    for (int o = 0; o < K; ++o) {
      const long q = (long)o * sr + (long)cc * sl;
      const double v = pp[q], vv = Vq[q];
      const double pv = st ? v : NEG_BIG;
      Pl[o * 64] = pv;
      Vl[o * 64] = (st && hasV) ? vv : 0.0;
      pmax = __builtin_fmax(pmax, pv);
    }
    for (int o = K; o < KP; ++o) {
      Pl[o * 64] = NEG_BIG;
      Vl[o * 64] = 0.0;
    }
    if constexpr (!LOGSPACE) {
      pmax = smp_wave_max(pmax);
#pragma unroll 4
      for (int o = 0; o < KP; ++o) {
        const double pe = exp(Pl[o * 64] - pmax);     // (padding: exp(-1e300) = 0)
        Pl[o * 64] = pe;
        Vl[o * 64] *= pe;
      }
    }
  };

  // ---- forward sweep ----------------------------------------------------------------------------------------------------
  double al, r;                                       // a_t[lane] (scaled) or log a_t[lane], normalised; r_t[lane]
  bool flagged = false;
  {
    stage(K, 1);                                      // pair[i][lane], V[i][lane]
    if constexpr (PREG) {
#pragma unroll
      for (int i = 0; i < KP; ++i) Pq[i] = accl[i * 64];
    }
    {
      const double x = st ? a.init_params[cc] + nd[0] : NEG_BIG;
      const double m = smp_wave_max(x);
      const double u = st ? exp(x - m) : 0.0;
      const double ssum = smp_wave_sum(u);
      if constexpr (LOGSPACE) {
        al = st ? x - (m + ::log(ssum)) : NEG_BIG;
      } else {
        flagged = st && !(u >= HMM_LOW);
        al = u / ssum;
      }
      r = st ? (a.g_init ? a.g_init[b * K + cc] : 0.0) + (Wp ? Wp[0] : 0.0) : 0.0;
      if (lp) { wsb[0] = al; wsb[KP] = r; }
    }
    for (int t = 1; t < TL; ++t) {
      const double x = st ? nd[(long)t * K] : NEG_BIG;
      const double w = (st && Wp) ? Wp[(long)t * K] : 0.0;
      if constexpr (LOGSPACE) {
        publish2(al, r);
        double m = NEG_BIG;
#pragma unroll UNR
        for (int i = 0; i < KP; ++i) {
          m = __builtin_fmax(m, lineA[i] + PM(i));
        }
        vjp_reread();
        double ssum = 0.0, n1 = 0.0;
#pragma unroll UNR
        for (int i = 0; i < KP; ++i) {
          const double wgt = exp(lineA[i] + PM(i) - m);           // softmax_i(log a_{t-1}[i] + pair[i][lane]), unnormalised
          ssum += wgt;
          n1 = __builtin_fma(wgt, lineB[i] + Vl[i * 64], n1);
        }
        const double lal = st ? m + ::log(ssum) + x : NEG_BIG;
        const double M = smp_wave_max(lal);
        const double tot = smp_wave_sum(st ? exp(lal - M) : 0.0);
        al = st ? lal - (M + ::log(tot)) : NEG_BIG;
        r = st ? (ssum > 0.0 ? n1 / ssum : 0.0) + w : 0.0;
      } else {
        publish2(al, al * r);
        const double m = smp_wave_max(x);
        const double e = st ? exp(x - m) : 0.0;
        double pred = 0.0, n1 = 0.0;
#pragma unroll UNR
        for (int i = 0; i < KP; ++i) {
          pred = __builtin_fma(lineA[i], PM(i), pred);
          n1 = __builtin_fma(lineB[i], PM(i), n1);
          n1 = __builtin_fma(lineA[i], Vl[i * 64], n1);
        }
        const double u = pred * e;
        const double cs = smp_wave_sum(u);
        flagged = flagged || (st && !(u >= HMM_LOW)) || !(cs > HMM_WIDE_TINY);
        al = u / cs;
        r = st ? (pred > 0.0 ? n1 / pred : 0.0) + w : 0.0;
      }
      if (lp) { wsb[(long)t * REC] = al; wsb[(long)t * REC + KP] = r; }
    }
  }
  if constexpr (!LOGSPACE) {
    if (__any(flagged)) {                             // (wave-uniform) the log-space launch takes it
      if (lane == 0) *flagp = 1.0;
      return;
    }
  }
  const double aL = LOGSPACE ? (st ? exp(al) : 0.0) : al;
  const double gE = gl - smp_wave_sum(st ? aL * r : 0.0);         // g - E[phi]

  // ---- backward sweep ---------------------------------------------------------------------------------------------------
  stage(1, K);                                        // pair[lane][j], V[lane][j]
#pragma unroll UNR
  for (int j = 0; j < KP; ++j) {
    if constexpr (PREG) Pq[j] = accl[j * 64];
    accl[j * 64] = 0.0;
  }
  double* dn = a.d_node + (b * T) * K + cc;
  {
    const double gn = aL * (gE + r);
    if (st) {
      dn[(long)(TL - 1) * K] = gn;
      if (TL == 1) a.d_init[b * K + cc] = gn;
    }
  }
  double bt = LOGSPACE ? (st ? 0.0 : NEG_BIG) : (st ? 1.0 : 0.0);  // b_{t+1} or its logarithm
  double s = 0.0;
  for (int t = TL - 2; t >= 0; --t) {
    const double x = st ? nd[(long)(t + 1) * K] : NEG_BIG;
    const double w1 = (st && Wp) ? Wp[(long)(t + 1) * K] : 0.0;
    const double at = wsb[(long)t * REC];
    const double rt = wsb[(long)t * REC + KP];
    double gam, sn;
    if constexpr (LOGSPACE) {
      publish2(st ? x + bt : NEG_BIG, st ? w1 + s : 0.0);          // log (e o b)_{t+1};  W[t+1] + s_{t+1}
      double m = NEG_BIG;
#pragma unroll UNR
      for (int j = 0; j < KP; ++j) {
          m = __builtin_fmax(m, PM(j) + lineA[j]);
        }
      vjp_reread();
      double ssum = 0.0, num = 0.0;
#pragma unroll UNR
      for (int j = 0; j < KP; ++j) {
        const double wgt = exp(PM(j) + lineA[j] - m);              // softmax_j(pair[lane][j] + node[t+1][j] + log b_{t+1}[j])
        ssum += wgt;
        num = __builtin_fma(wgt, Vl[j * 64] + lineB[j], num);
      }
      const double lbr = st ? m + ::log(ssum) : NEG_BIG;
      sn = (st && ssum > 0.0) ? num / ssum : 0.0;
      const double lg = st ? at + lbr : NEG_BIG;
      const double M = smp_wave_max(lg);
      const double eg = st ? exp(lg - M) : 0.0;
      const double tot = smp_wave_sum(eg);
      const double lZ = M + ::log(tot);
      gam = eg / tot;
      bt = st ? lbr - lZ : NEG_BIG;
      const double base = at - lZ;                                 // xi_t[lane][j] = exp(log a_t + pair + log (e o b) - log Z_t)
      const double cq = gE + rt;
      vjp_reread();
#pragma unroll UNR
      for (int j = 0; j < KP; ++j) {
        const double xi = exp(base + (PM(j) + lineA[j]));          // (lanes past K: pair = -1e300)
        accl[j * 64] = __builtin_fma(xi, cq + (Vl[j * 64] + lineB[j]), accl[j * 64]);
      }
    } else {
      const double m = smp_wave_max(x);
      const double e = st ? exp(x - m) : 0.0;
      const double u = e * bt;
      publish2(u, u * (w1 + s));
      double braw = 0.0, num = 0.0;
#pragma unroll UNR
      for (int j = 0; j < KP; ++j) {
        braw = __builtin_fma(PM(j), lineA[j], braw);
        num = __builtin_fma(PM(j), lineB[j], num);
        num = __builtin_fma(Vl[j * 64], lineA[j], num);
      }
      flagged = flagged || (st && !(braw >= HMM_LOW));
      const double Z = smp_wave_sum(at * braw);
      flagged = flagged || !(Z > HMM_WIDE_TINY);
      const double rz = 1.0 / Z;
      sn = braw > 0.0 ? num / braw : 0.0;
      bt = braw * rz;
      gam = at * bt;
      const double a0 = at * rz;
      const double cA = a0 * (gE + rt);
      vjp_reread();
#pragma unroll UNR
      for (int j = 0; j < KP; ++j) {
        const double p0 = PM(j) * lineA[j];
        const double p1 = __builtin_fma(PM(j), lineB[j], Vl[j * 64] * lineA[j]);
        accl[j * 64] += __builtin_fma(cA, p0, a0 * p1);
      }
    }
    s = sn;
    const double gn = gam * (gE + rt + sn);
    if (st) {
      dn[(long)t * K] = gn;
      if (t == 0) a.d_init[b * K + cc] = gn;
    }
  }
  if (st) {
    double* dp = a.d_pair + (b * K + cc) * K;
#pragma unroll
    for (int j = 0; j < KP; ++j)
      if (j < K) dp[j] = accl[j * 64];
  }
  if constexpr (!LOGSPACE) {
    flagged = __any(flagged);
    if (lane == 0) *flagp = flagged ? 1.0 : 0.0;
  }
}

// ---- host: the two launches behind svae_hmm_estep_vjp_f64 (RAGGED = false) and svae_hmm_ragged_estep_vjp_f64 (RAGGED =
// true): the scaled kernel, then the log-space kernel of its width over the sequences it flagged (KP = 16 behind a row kernel)
template <bool RAGGED>
static int launch_vjp(const VjpArgsT<RAGGED>& a, hipStream_t s) {
  auto redo = [&](auto kp) { hipLaunchKernelGGL((hmm_vjp_wide_kernel<kp, true, RAGGED>), dim3(a.B), dim3(64), 0, s, a); };
  hmm_dispatch_k(
      a.K,
      [&](auto k) {
        hipLaunchKernelGGL((hmm_vjp_row_kernel<k, RAGGED>), dim3((a.B + 3) / 4), dim3(64), 0, s, a);
        redo(std::integral_constant<int, 16>{});
        return 0;
      },
      [&](auto kp) {
        hipLaunchKernelGGL((hmm_vjp_wide_kernel<kp, false, RAGGED>), dim3(a.B), dim3(64), 0, s, a);
        redo(kp);
        return 0;
      });
  return hipGetLastError() == hipSuccess ? 0 : -1000;
}

}  // namespace svae
