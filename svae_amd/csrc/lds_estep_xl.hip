// lds_estep_xl.hip -- LDS E-step for latent dimension 65 <= n <= 128 on MI355X (gfx950).
//
// What it replaces (reference = mattjj/svae): natural_filter_forward_general svae/lds/cython_lds_inference.pyx:28-90,
// natural_smoother_general :149-195 and _compute_stats :197-210 (wired at svae/lds/lds_inference.py:232-237), at
// latent sizes where the tile path's per-sequence LDS panel [P | R | c] (lds_estep_tile.hip: 156 KB at n = 96,
// 272 KB at n = 128) no longer fits the 160 KiB of a CU.
//
// Mapping: one workgroup of NB = ceil(n / 16) wavefronts per sequence, one workgroup per CU (NB = 8: two wavefronts per
// SIMD, 256 registers each).  NP = 16 NB; padding rows / columns carry an identity diagonal as in the tile path.
//   forward   wavefront i OWNS tile row i of the step's panel [P | R] (P = pivot block, R = J12) in registers, 2 NB
//             tiles in the MFMA C layout (NB = 8: 16 tiles x 4 doubles = 128 VGPRs).  Block Gauss-Jordan with
//             16x16 block pivots k = 0 .. NB-1, two barriers per pivot:
//               (a) the owner of row k writes it to a pivot-row buffer in LDS and factors the pivot tile
//                   A_kk = L D L' with the tile path's DPP elimination (factor_pivot_tile: U = L^-1, D^-1, log det);
//                   every other wavefront i parks its tile A_ik in a private LDS tile (C layout -> A operand);
//               (b) all wavefronts scale the pivot row, two tiles each: A_kj <- U' D^-1 U A_kj, A_kk <- A_kk^-1;
//               (c) wavefront i != k:  A_ij -= A_ik (A_kk^-1 A_kj),  A_ik <- -A_ik A_kk^-1;  the owner reloads row k.
//             The two pivot-row buffers alternate, so that (a) of pivot k+1 never waits for (c) of pivot k.
//             Afterwards row i holds P^-1 and X = P^-1 J12; c = P^-1 h is a per-lane product with the row.  The
//             hand-off record goes to the workspace straight from the registers.  Schur step: X goes to LDS (the
//             pivot-row buffers' space), and wavefront i forms its own tile row of  P' = -2 (J22 + J11') - J12' X
//             and h' = node_h' + J12' c, with -J12' read in A-fragment order from the pre-packed pair parameters.
//   backward  moment form, the full NP x NP Sigma_{t+1} in LDS (NB = 8: 133 KB).  Wavefront i reads its tile row of
//             X_t from the record (A-fragment layout: the same registers are the B operand of X_t'), then
//               (1) W = Sigma_{t+1} X_t', tile column i, in registers; m_t = c_t + X_t m_{t+1}, rows of tile row i;
//               (2) W replaces Sigma_{t+1} in LDS;  Sigma_t = P_t^-1 + X_t W, tile row i;  Sigma_t replaces W.
//             Four barriers per step.  The statistics come from the same registers; the homogeneous sums over t are
//             accumulated in their output slots (each element belongs to one lane: fixed order, deterministic).
// LDS: max(NP (NP + 2) | 2 pivot-row buffers of 16 x (2 NP + 2) + NB transposition tiles) + the pivot factor + 4 NP:
// 137 KB at NB = 8.
//
// Hand-off record per step: the tile path's (TileCfg::WSTEP): X, P^-1 (row-major NP x NP), c (NP) -- 2 NP^2 + NP
// doubles, 263 KB at n = 128 (B = 512, T = 200: 26.9 GB of workspace).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/svae_hip.h"
#include "dpp.hpp"
#include "lds_units.hpp"
#include "lds_tile_mfma.hpp"
#include "per_device.hpp"

namespace svae {

template <int NB>
struct XlCfg {
  static constexpr int NP = 16 * NB;
  static constexpr int NT = 64 * NB;                        // threads per workgroup
  static constexpr int WSTEP = 2 * NP * NP + NP;            // hand-off per step: X, P^-1 (row-major NP x NP), c
  static constexpr int LDR = 2 * NP + 2;                    // pivot-row buffer [P_k | R_k], row stride == 2 (mod 32)
  static constexpr int LDX = 32 * ((NP + 31) / 32) + 2;     // one NP x NP matrix (X_t, Sigma_t, W_t), == 2 (mod 32)
  static constexpr int LDU = 18;                            // 16x16 tiles: pivot factor U = L^-1, transposition tiles
  static constexpr int ROWBUF = 16 * LDR;
  static constexpr int GJ_DOUBLES = 2 * ROWBUF + NB * 16 * LDU;
  static constexpr int BIG = NP * LDX > GJ_DOUBLES ? NP * LDX : GJ_DOUBLES;
  static constexpr int LDS_DOUBLES = BIG + 16 * LDU + 16 + 4 * NP + 32;
};
static_assert(XlCfg<8>::LDS_DOUBLES * 8 <= 160 * 1024, "one workgroup per CU");

template <int NB, bool INHOMOG>
__global__ __launch_bounds__(64 * NB) void lds_estep_xl_kernel(const LdsArgs a, const int n,
                                                              const double* __restrict__ pk_base, const int pk_batched) {
  using Cfg = XlCfg<NB>;
  constexpr int NP = Cfg::NP, NT = Cfg::NT, WSTEP = Cfg::WSTEP, LDR = Cfg::LDR, LDX = Cfg::LDX, LDU = Cfg::LDU;
  extern __shared__ double smem[];
  double* big = smem;                      // forward: pivot-row buffers + transposition tiles, then X; backward: Sigma / W
  double* ubuf = big + Cfg::BIG;           // U = L^-1 of the current pivot tile (row stride LDU), then D^-1
  double* dinv = ubuf + 16 * LDU;
  double* hvec = dinv + 16;                // forward: h of the step
  double* cvec = hvec + NP;                // forward: c = P^-1 h of the step
  double* mv0 = cvec + NP;                 // backward: smoothed means (double buffer)
  double* mv1 = mv0 + NP;
  double* red = mv1 + NP;                  // 32 doubles of reduction scratch

  const int tid = threadIdx.x;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int lane = tid & 63, r16 = lane & 15, kq = lane >> 4;
  const int i = wave;                      // the tile row this wavefront owns
  const int b = blockIdx.x;
  const int T = a.T;
  const long nn = (long)n * n;
  const double* J11 = a.J11 + (long)b * a.pair_seq_stride;
  const double* J12 = a.J12 + (long)b * a.pair_seq_stride;
  const double* nodeJ = a.node_J + (long)b * T * n;
  const double* nodeh = a.node_h + (long)b * T * n;
  double* wsb = a.ws + (long)b * T * WSTEP;
  // packed pair parameters: per set, (INHOMOG ? T-1 : 2) slots of [pA | pC | pR] (3 NP^2 doubles, xl_pack_pairs_kernel)
  const double* packed = pk_base + (pk_batched ? (long)b * (T - 1) * (3 * NP * NP) : 0);
  const d4 z4 = {0.0, 0.0, 0.0, 0.0};

  double ldM = 1.0, pmin = 1.0e300, qacc = 0.0;
  int ldE = 0;

  // ---- step 0: P = -2 (init_J + J11) + diag(-2 node_J[0]),  R = J12,  h = init_h + node_h[0] ------------------------
  d4 row[2 * NB];            // tile (i, j) of [P | R], C layout: lane holds [16 i + 4 qq + kq][16 j + r16]
  static_for<0, 2 * NB>([&](auto jc) {
    constexpr int j = jc;
#pragma unroll
    for (int qq = 0; qq < 4; ++qq) {
      const int r = 16 * i + 4 * qq + kq, c = 16 * (j % NB) + r16;
      const bool in = r < n && c < n;
      double v;
      if constexpr (j < NB) {
        v = (r == c) ? 1.0 : 0.0;
        if (in) {
          v = -2.0 * a.init_J[r * n + c];
          if (T > 1) v -= 2.0 * J11[r * n + c];
          if (r == c) v -= 2.0 * nodeJ[r];
        }
      } else {
        v = (in && T > 1) ? J12[r * n + c] : 0.0;
      }
      row[j][qq] = v;
    }
  });
  if (tid < NP) hvec[tid] = tid < n ? a.init_h[tid] + nodeh[tid] : 0.0;

  for (int t = 0; t < T; ++t) {
    const bool last = (t == T - 1);
    // (opaque copy of the lane index: the lane-dependent LDS / global addresses of the step are recomputed every step
    //  instead of being hoisted out of the time loop, where ~40 of them cost more registers than the budget has left)
    int lx = lane;
    asm volatile("" : "+v"(lx));
    const int lane = lx, r16 = lx & 15, kq = lx >> 4;
    double* stg = big + 2 * Cfg::ROWBUF + i * 16 * LDU;   // this wavefront's transposition tile
    // ---- block Gauss-Jordan on [P | R] ---------------------------------------------------------------------------
    static_for<0, NB>([&](auto kc) {
      constexpr int k = kc;
      double* rb = big + (k & 1) * Cfg::ROWBUF;
      // (a) pivot row to LDS and its pivot tile factored by the owner; the others park A_ik
      if (i == k) {
        // (the owner's row is rebuilt from the buffer in (c): zeroed here, so that its 16 NB registers are free for the
        //  factorisation -- otherwise the compiler keeps them live through it and spills)
        static_for<0, 2 * NB>([&](auto jc) { store_c(rb, LDR, 0, 16 * jc, r16, kq, row[jc]); row[jc] = z4; });
        factor_pivot_tile(rb + 16 * k, LDR, ubuf, LDU, dinv, r16, kq, pmin, ldM, ldE);
      } else {
        store_c(stg, LDU, 0, 0, r16, kq, row[k]);
      }
      __syncthreads();
      // (b) pivot row <- A_kk^-1 (pivot row): tiles i and i + NB of the buffer
      {
        const d4 fu = frag_a(ubuf, LDU, 0, 0, r16, kq), fut = frag_b(ubuf, LDU, 0, 0, r16, kq);
        d4 dq;
#pragma unroll
        for (int qq = 0; qq < 4; ++qq) dq[qq] = dinv[4 * qq + kq];
#pragma unroll
        for (int s = 0; s < 2; ++s) {
          const int j = i + s * NB;
          d4 v = (j == k) ? fut : mma16(fu, frag_b(rb, LDR, 0, 16 * j, r16, kq), z4);   // U A_kj  (tile k: U)
#pragma unroll
          for (int qq = 0; qq < 4; ++qq) v[qq] *= dq[qq];
          store_c(rb, LDR, 0, 16 * j, r16, kq, mma16(fut, v, z4));
        }
      }
      __syncthreads();
      // (c) elimination of tile column k from the other rows:  row_j <- row_j - A_ik (scaled pivot row)_j  (tile k: 0 - ..);
      //     the owner takes the scaled row back through the same products, as  0 + I (scaled pivot row)_j  (exact)
      {
        d4 nfa;
        if (i == k) {
#pragma unroll
          for (int kb = 0; kb < 4; ++kb) nfa[kb] = (r16 == 4 * kb + kq) ? 1.0 : 0.0;
        } else {
          nfa = -frag_a(stg, LDU, 0, 0, r16, kq);
        }
        // (software pipeline: the fragment of tile j+1 is requested before the MFMAs of tile j; the scheduling barrier
        //  keeps the compiler from hoisting all 2 NB fragment reads to the top, which costs 8 NB registers it does not have)
        d4 fb = frag_b(rb, LDR, 0, 0, r16, kq);
        static_for<0, 2 * NB>([&](auto jc) {
          constexpr int j = jc;
          const d4 cur = fb;
          if constexpr (j + 1 < 2 * NB) fb = frag_b(rb, LDR, 0, 16 * (j + 1), r16, kq);
          row[j] = mma16(nfa, cur, j == k ? z4 : row[j]);
          __builtin_amdgcn_sched_barrier(0);
        });
      }
    });

    // ---- hand-off record: X, P^-1 (row-major NP x NP), c --------------------------------------------------------
    double* w = wsb + (long)t * WSTEP;
    static_for<0, NB>([&](auto jc) {
      store_c(w, NP, 16 * i, 16 * jc, r16, kq, row[NB + jc]);
      store_c(w + NP * NP, NP, 16 * i, 16 * jc, r16, kq, row[jc]);
    });
    {  // c = P^-1 h for the rows of this tile row: lanes hold columns, summed over the 16 lanes of a DPP row
      d4 s = z4;
      static_for<0, NB>([&](auto jc) {
        const double hv = hvec[16 * jc + r16];
#pragma unroll
        for (int qq = 0; qq < 4; ++qq) s[qq] = __builtin_fma(row[jc][qq], hv, s[qq]);
      });
#pragma unroll
      for (int qq = 0; qq < 4; ++qq) s[qq] = group_sum<16>(s[qq]);
      if (r16 == 0) {
#pragma unroll
        for (int qq = 0; qq < 4; ++qq) {
          const int r = 16 * i + 4 * qq + kq;
          cvec[r] = s[qq];
          w[2 * NP * NP + r] = s[qq];
          qacc = __builtin_fma(hvec[r], s[qq], qacc);      // h' P^-1 h
        }
      }
    }
    __syncthreads();           // (pivot-row buffers free, c complete)

    if (!last) {
      // ---- Schur step:  P' = -2 (J22 + J11') + diag(-2 node_J') - J12' X,  h' = node_h' + J12' c -----------------
      double* Xs = big;
      static_for<0, NB>([&](auto jc) { store_c(Xs, LDX, 16 * i, 16 * jc, r16, kq, row[NB + jc]); });
      const double* pk = packed + (long)(INHOMOG ? t : (t + 1 == T - 1 ? 1 : 0)) * (3 * NP * NP);
      static_for<0, NB>([&](auto jc) { row[jc] = *(const d4*)(pk + NP * NP + ((i * NB + jc) * 64 + lane) * 4); });
      const long tn = (long)(t + 1) * n;
      const int myrow = 16 * i + r16;
      const double njd = nodeJ[tn + (myrow < n ? myrow : n - 1)];
      const double nhn = nodeh[tn + (myrow < n ? myrow : n - 1)];
      __syncthreads();         // (X complete)
      double s0 = 0.0, s1 = 0.0;
      static_for<0, NB>([&](auto kc) {
        constexpr int kk = kc;
        const d4 fa = *(const d4*)(pk + ((i * NB + kk) * 64 + lane) * 4);      // (-J12') tile (i, kk), A operand
        d4 fb = frag_b(Xs, LDX, 16 * kk, 0, r16, kq);
        static_for<0, NB>([&](auto jc) {
          constexpr int j = jc;
          const d4 cur = fb;
          if constexpr (j + 1 < NB) fb = frag_b(Xs, LDX, 16 * kk, 16 * (j + 1), r16, kq);
          row[j] = mma16(fa, cur, row[j]);
          __builtin_amdgcn_sched_barrier(0);
        });
        const double* cp = cvec + 16 * kk + kq;
        s0 = __builtin_fma(fa[0], cp[0], s0);
        s1 = __builtin_fma(fa[1], cp[4], s1);
        s0 = __builtin_fma(fa[2], cp[8], s0);
        s1 = __builtin_fma(fa[3], cp[12], s1);
      });
      // node diagonal on the diagonal tile (i, i): lane (r16, kq) holds rows 16 i + 4 qq + kq, column 16 i + r16
      const double njd2 = myrow < n ? 2.0 * njd : 0.0;
      static_for<0, NB>([&](auto jc) {
        if (jc == i) {
#pragma unroll
          for (int qq = 0; qq < 4; ++qq) row[jc][qq] -= (4 * qq + kq == r16) ? njd2 : 0.0;
        }
      });
      double sh = s0 + s1;                                   // -(J12' c)[myrow], a quarter per DPP row
      sh += __shfl_xor(sh, 16, 64);
      sh += __shfl_xor(sh, 32, 64);
      if (kq == 0) hvec[myrow] = myrow < n ? nhn - sh : 0.0;
      static_for<0, NB>([&](auto jc) {                     // next right-hand sides (zero ahead of the last step)
        row[NB + jc] = *(const d4*)(pk + 2 * NP * NP + ((i * NB + jc) * 64 + lane) * 4);
      });
      __syncthreads();         // (X read by all before the next pivot-row buffers overwrite it)
    }
  }

  // ---- log-normaliser ----------------------------------------------------------------------------------------------
  {
    double z = qacc * 0.5;
    if (a.node_logZ) { for (int t = tid; t < T; t += NT) z += a.node_logZ[(long)b * T + t]; }
    if (INHOMOG) {
      const double* lz = a.logZ_pair + (a.pair_seq_stride ? (long)b * (T - 1) : 0);
      for (int t = tid; t < T - 1; t += NT) z += lz[t];
    }
#pragma unroll
    for (int s = 1; s < 64; s <<= 1) z += __shfl_xor(z, s, 64);
    if (lane == 0) {
      red[wave] = z;
      red[8 + wave] = ::log(ldM) + (double)ldE * 0.6931471805599453094;   // log det of the pivots this wavefront factored
      red[16 + wave] = pmin;
    }
    __syncthreads();
    if (tid == 0) {
      double total = 0.0, logdet = 0.0, pm = 1.0e300;
      for (int q = 0; q < NB; ++q) { total += red[q]; logdet += red[8 + q]; pm = fmin(pm, red[16 + q]); }
      total += a.init_logZ[0];
      if (!INHOMOG && T > 1) total += (double)(T - 1) * a.logZ_pair[0];
      total -= 0.5 * logdet;
      a.lognorm[b] = total;
      const bool bad = !(pm > 0.0) || !(total == total);
      if (bad) {
        int old = *(volatile int32_t*)a.info;
        while (old == 0 || old > b + 1) {
          const int seen = atomicCAS(a.info, old, b + 1);
          if (seen == old) break;
          old = seen;
        }
      }
    }
  }
  __syncthreads();

  // ---- backward pass (moment form) ----------------------------------------------------------------------------------
  double* S = big;                         // Sigma_{t+1}, then W_t
  for (int idx = tid; idx < NP * NP; idx += NT) S[(idx / NP) * LDX + (idx % NP)] = 0.0;   // Sigma_T := 0
  if (tid < NP) { mv0[tid] = 0.0; mv1[tid] = 0.0; }
  double* mold = mv0;
  double* mnew = mv1;
  double* oEx = a.E_node_x + (long)b * T * n;
  double* oExx = a.E_node_diagxx + (long)b * T * n;
  double* oI = a.E_init + (long)b * (nn + n);
  double* oPh = a.E_pair + (long)b * 3 * nn;             // homogeneous: the three sums
  __syncthreads();
  for (int t = T - 1; t >= 0; --t) {
    int lx = lane;                         // (as in the forward loop)
    asm volatile("" : "+v"(lx));
    const int r16 = lx & 15, kq = lx >> 4;
    const double* w = wsb + (long)t * WSTEP;
    d4 bx[NB];              // X_t tile (i, l) as A operand (lane: X[16 i + r16][16 l + 4 kb + kq]) == B operand of X_t'
    static_for<0, NB>([&](auto lc) {
      const double* p = w + (16 * i + r16) * NP + 16 * lc + kq;
      bx[lc] = d4{p[0], p[4], p[8], p[12]};
    });
    if (t + 1 < T && tid < n) {            // node statistics of step t+1 (S holds Sigma_{t+1})
      const double mm = mold[tid];
      oEx[(long)(t + 1) * n + tid] = mm;
      oExx[(long)(t + 1) * n + tid] = __builtin_fma(mm, mm, S[tid * LDX + tid]);
    }
    {  // m_t = c_t + X_t m_{t+1}, rows 16 i + r16
      double s = 0.0;
      static_for<0, NB>([&](auto lc) {
#pragma unroll
        for (int kb = 0; kb < 4; ++kb) s = __builtin_fma(bx[lc][kb], mold[16 * lc + 4 * kb + kq], s);
      });
      s += __shfl_xor(s, 16, 64);
      s += __shfl_xor(s, 32, 64);
      if (kq == 0) mnew[16 * i + r16] = w[2 * NP * NP + 16 * i + r16] + s;
    }
    // (1) W = Sigma_{t+1} X_t', tile column i:  W[m][i] = sum_l Sigma[m][l] X[i][l]'   (= Cov(x_{t+1}, x_t))
    d4 wt[NB];
    static_for<0, NB>([&](auto mc) {
      d4 c = z4;
      static_for<0, NB>([&](auto lc) { c = mma16(frag_a(S, LDX, 16 * mc, 16 * lc, r16, kq), bx[lc], c); });
      wt[mc] = c;
      __builtin_amdgcn_sched_barrier(0);      // (one tile's fragments in flight at a time: see the elimination)
    });
    __syncthreads();           // (Sigma_{t+1} read by all; m_t complete)
    // (opaque copies of the lane coordinates: the 8 NB output addresses below are recomputed every step instead of being
    //  hoisted out of the time loop as 64-bit loop invariants -- registers the 256-register budget does not have)
    int r16x = r16, kqx = kq;
    asm volatile("" : "+v"(r16x), "+v"(kqx));
    const int col = 16 * i + r16x;
    const double mcol = mnew[col];
    // cross moments E[x_{t+1} x_t'](row, col) = W + m_{t+1} m_t', stored transposed: slot 1 = E[x_t x_{t+1}']
    // (homogeneous: at t = T-1 the term is exactly 0 and initialises the sum)
    if (INHOMOG ? t < T - 1 : true) {
      double* o1 = INHOMOG ? a.E_pair + ((long)b * (T - 1) + t) * 3 * nn + nn : oPh + nn;
      static_for<0, NB>([&](auto mc) {
#pragma unroll
        for (int qq = 0; qq < 4; ++qq) {
          const int r = 16 * mc + 4 * qq + kqx;
          if (r < n && col < n) {
            const double v = __builtin_fma(mold[r], mcol, wt[mc][qq]);
            double* p = o1 + (long)col * n + r;
            *p = (INHOMOG || t == T - 1) ? v : *p + v;
          }
        }
      });
    }
    static_for<0, NB>([&](auto mc) { store_c(S, LDX, 16 * mc, 16 * i, r16, kq, wt[mc]); });
    __syncthreads();           // (W complete)
    // (2) Sigma_t = P_t^-1 + X_t W, tile row i
    d4 sg[NB];
    static_for<0, NB>([&](auto bc) {
      const double* pp = w + NP * NP + (16 * i + kq) * NP + 16 * bc + r16;
      d4 c = d4{pp[0], pp[4 * NP], pp[8 * NP], pp[12 * NP]};
      static_for<0, NB>([&](auto mc) { c = mma16(bx[mc], frag_b(S, LDX, 16 * mc, 16 * bc, r16, kq), c); });
      sg[bc] = c;
      __builtin_amdgcn_sched_barrier(0);
    });
    // E[x_t x_t'](row, c) = Sigma_t + m_t m_t',  row = 16 i + 4 qq + kq,  c = 16 bc + r16
    static_for<0, NB>([&](auto bc) {
      const int c = 16 * bc + r16x;
#pragma unroll
      for (int qq = 0; qq < 4; ++qq) {
        const int r = 16 * i + 4 * qq + kqx;
        if (r < n && c < n) {
          const double v = __builtin_fma(mnew[r], mnew[c], sg[bc][qq]);
          const long e = (long)r * n + c;
          if (INHOMOG) {
            if (t < T - 1) a.E_pair[((long)b * (T - 1) + t) * 3 * nn + e] = v;                 // E[x_t x_t']
            if (t > 0) a.E_pair[((long)b * (T - 1) + t - 1) * 3 * nn + 2 * nn + e] = v;        // E[x_{t+1} x_{t+1}'] of t-1
          } else {
            // slot 0: sum_{t<=T-2} E[x_t x_t'], slot 2: sum_{t>=1}, each summed on its own (the tile path's
            // "slot 0 + last - first" cancels on ill-conditioned models)
            if (t == T - 1) {
              oPh[e] = 0.0;
              oPh[2 * nn + e] = T > 1 ? v : 0.0;
            } else {
              oPh[e] += v;
              if (t > 0) oPh[2 * nn + e] += v;
            }
          }
          if (t == 0) oI[e] = v;
        }
      }
    });
    __syncthreads();           // (W read by all)
    static_for<0, NB>([&](auto bc) { store_c(S, LDX, 16 * i, 16 * bc, r16, kq, sg[bc]); });
    double* tmp = mold; mold = mnew; mnew = tmp;
    __syncthreads();
  }
  if (tid < n) {                           // node statistics of step 0, E[x_0]
    const double mm = mold[tid];
    oEx[tid] = mm;
    oExx[tid] = __builtin_fma(mm, mm, S[tid * LDX + tid]);
    oI[nn + tid] = mm;
  }
}

// Pair parameters of one step (slot) re-packed in the register order of the main kernel:
//   pA[((i NB + kk) 64 + lane) 4 + kb] = -J12[16 kk + 4 kb + kq][16 i + r16]        (A operand of -(J12'))
//   pC[((i NB + j) 64 + lane) 4 + qq]  = -2 (J22 + w J11n)[16 i + 4 qq + kq][16 j + r16], identity on the padding
//   pR[((i NB + j) 64 + lane) 4 + qq]  = J12n[16 i + 4 qq + kq][16 j + r16] (zero-padded; zero ahead of the last step)
// Homogeneous parameters: slot 0 = regular step, slot 1 = the step before the last one (no J11 term, zero right-hand
// side).  Per-step parameters: slot t = transition t -> t+1 (t = 0 .. T-2).
template <int NB>
__global__ __launch_bounds__(256) void xl_pack_pairs_kernel(const double* __restrict__ J11, const double* __restrict__ J12,
                                                            const double* __restrict__ J22, int n, int T, int inhomog,
                                                            long set_stride, double* __restrict__ out) {
  constexpr int NP = 16 * NB;
  const int slot = blockIdx.x, set = blockIdx.y;
  const int nslots = inhomog ? T - 1 : 2;
  const long nn = (long)n * n;
  const int t = inhomog ? slot : 0;
  const bool next_last = inhomog ? (t + 1 == T - 1) : (slot == 1);
  const double* j12 = J12 + set * set_stride + (long)t * nn;
  const double* j22 = J22 + set * set_stride + (long)t * nn;
  const double* j11n = J11 + set * set_stride + (long)(inhomog && !next_last ? t + 1 : t) * nn;
  const double* j12n = J12 + set * set_stride + (long)(inhomog && !next_last ? t + 1 : t) * nn;
  double* o = out + ((long)set * nslots + slot) * (3 * NP * NP);
  for (int e = threadIdx.x; e < NP * NP; e += 256) {
    const int qq = e & 3, lane = (e >> 2) & 63, tile = e >> 8;
    const int r16 = lane & 15, kq = lane >> 4, ti = tile / NB, tj = tile % NB;
    {  // pA: tile (i = ti, kk = tj), kb = qq
      const int row = 16 * tj + 4 * qq + kq, col = 16 * ti + r16;
      o[e] = (row < n && col < n) ? -j12[row * n + col] : 0.0;
    }
    const int row = 16 * ti + 4 * qq + kq, col = 16 * tj + r16;
    {  // pC: tile (i = ti, j = tj)
      double v = (row == col) ? 1.0 : 0.0;
      if (row < n && col < n) v = -2.0 * j22[row * n + col] - (next_last ? 0.0 : 2.0 * j11n[row * n + col]);
      o[NP * NP + e] = v;
    }
    o[2 * NP * NP + e] = (!next_last && row < n && col < n) ? j12n[row * n + col] : 0.0;   // pR
  }
}

template <int NB>
static int launch_xl(const LdsArgs& a, int n, int inhomog, hipStream_t s) {
  using Cfg = XlCfg<NB>;
  const size_t lds = Cfg::LDS_DOUBLES * sizeof(double);
  const int T = a.T;
  double* pk = a.ws + (size_t)a.B * T * Cfg::WSTEP;     // workspace: [hand-off: B T WSTEP][packed pair parameters]
  const int batched = a.pair_seq_stride != 0;
  if (T > 1) {
    const int nslots = inhomog ? T - 1 : 2;
    hipLaunchKernelGGL((xl_pack_pairs_kernel<NB>), dim3(nslots, batched ? a.B : 1), dim3(256), 0, s,
                       a.J11, a.J12, a.J22, n, T, inhomog, (long)a.pair_seq_stride, pk);
    if (hipGetLastError() != hipSuccess) return -1000;
  }
  static LdsGrant grants[2];
  auto go = [&](auto kern, int which) {
    if (!grants[which].ensure((const void*)kern, (long)lds)) return -1001;
    hipLaunchKernelGGL(kern, dim3(a.B), dim3(Cfg::NT), lds, s, a, n, (const double*)pk, batched);
    return hipGetLastError() == hipSuccess ? 0 : -1000;
  };
  return inhomog ? go(lds_estep_xl_kernel<NB, true>, 0) : go(lds_estep_xl_kernel<NB, false>, 1);
}

}  // namespace svae

extern "C" size_t svae_lds_xl_workspace_bytes(int B, int T, int n, int inhomog, int pair_batched) {
  if (B <= 0 || T <= 0 || n <= SVAE_LDS_TILE_MAX_N || n > SVAE_LDS_XL_MAX_N) return 0;
  const size_t NP = 16 * (size_t)((n + 15) / 16);
  const size_t packed = T < 2 ? 0 : (pair_batched ? (size_t)B : 1) * (inhomog ? (size_t)(T - 1) : 2) * 3 * NP * NP;
  return ((size_t)B * T * (2 * NP * NP + NP) + packed) * sizeof(double);
}

extern "C" int svae_lds_xl_estep_f64(int B, int T, int n, int inhomog, int pair_batched, int keep, unsigned options,
                                     const double* init_J, const double* init_h, const double* init_logZ,
                                     const double* J11, const double* J12, const double* J22,
                                     const double* logZ_pair,
                                     const double* node_J, const double* node_h, const double* node_logZ,
                                     double* lognorm, double* E_init, double* E_pair,
                                     double* E_node_diagxx, double* E_node_x,
                                     int32_t* info, void* workspace, size_t ws_bytes, void* stream) {
  if (B < 0) return -1;
  if (T < 1) return -2;
  if (n <= SVAE_LDS_TILE_MAX_N || n > SVAE_LDS_XL_MAX_N) return -3;
  if (keep != 0) return -23;
  if (pair_batched && !inhomog) return -5;
  svae::LdsArgs a{};
  svae::set_estep_args(a, B, T, n, pair_batched, init_J, init_h, init_logZ, J11, J12, J22, logZ_pair, node_J, node_h, node_logZ,
                       lognorm, E_init, E_pair, E_node_diagxx, E_node_x, info, workspace);
  if (const int rc = svae::check_model(a)) return rc;
  if (options != 0) return -24;
  if (B == 0) return 0;                  // (the per-sequence arrays of an empty batch may be NULL)
  if (const int rc = svae::check_arrays(a)) return rc;
  if (!workspace || ws_bytes < svae_lds_xl_workspace_bytes(B, T, n, inhomog, pair_batched)) return -22;
  hipStream_t s = (hipStream_t)stream;
  switch ((n + 15) / 16) {
    case 5: return svae::launch_xl<5>(a, n, inhomog, s);
    case 6: return svae::launch_xl<6>(a, n, inhomog, s);
    case 7: return svae::launch_xl<7>(a, n, inhomog, s);
    case 8: return svae::launch_xl<8>(a, n, inhomog, s);
  }
  return -3;
}
