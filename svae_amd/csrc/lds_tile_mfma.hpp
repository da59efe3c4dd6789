// lds_tile_mfma.hpp -- the 16x16 f64 tile primitives shared by the MFMA LDS E-step kernels (lds_estep_tile.hip,
// 16 <= n <= 64, and lds_estep_xl.hip, 65 <= n <= 128): fragment addressing of v_mfma_f64_16x16x4_f64 operands, the
// tile product, and the DPP factorisation of a 16x16 SPD pivot tile.
#pragma once
#include <hip/hip_runtime.h>

#include "dpp.hpp"

namespace svae {

typedef double d4 __attribute__((ext_vector_type(4)));

// D = A(16x16) * B(16x16) + C as four 16x16x4 MFMAs; a[kb]/b[kb] = k-chunk kb of the fragments.
__device__ __forceinline__ d4 mma16(const d4 a, const d4 b, d4 c) {
  c = __builtin_amdgcn_mfma_f64_16x16x4f64(a[0], b[0], c, 0, 0, 0);
  c = __builtin_amdgcn_mfma_f64_16x16x4f64(a[1], b[1], c, 0, 0, 0);
  c = __builtin_amdgcn_mfma_f64_16x16x4f64(a[2], b[2], c, 0, 0, 0);
  c = __builtin_amdgcn_mfma_f64_16x16x4f64(a[3], b[3], c, 0, 0, 0);
  return c;
}

// Two independent products sharing the A fragment, MFMAs interleaved (the second chain fills the
// result latency of the first).
__device__ __forceinline__ void mma16x2(const d4 a, const d4 b0, d4& c0, const d4 b1, d4& c1) {
#pragma unroll
  for (int kb = 0; kb < 4; ++kb) {
    c0 = __builtin_amdgcn_mfma_f64_16x16x4f64(a[kb], b0[kb], c0, 0, 0, 0);
    c1 = __builtin_amdgcn_mfma_f64_16x16x4f64(a[kb], b1[kb], c1, 0, 0, 0);
  }
}

// Fragment addressing (lane = 16 kq + r16).  For a row-major tile Tl at (row0, col0):
//   frag_a: A operand of Tl   (lane holds Tl[r16][4 kb + kq])   == B operand of Tl'
//   frag_b: B operand of Tl   (lane holds Tl[4 kb + kq][r16])   == A operand of Tl'  == C/D layout
__device__ __forceinline__ d4 frag_a(const double* M, int ld, int row0, int col0, int r16, int kq) {
  const double* p = M + (row0 + r16) * ld + col0 + kq;
  return d4{p[0], p[4], p[8], p[12]};
}
__device__ __forceinline__ d4 frag_b(const double* M, int ld, int row0, int col0, int r16, int kq) {
  const double* p = M + (row0 + kq) * ld + col0 + r16;
  return d4{p[0], p[4 * ld], p[8 * ld], p[12 * ld]};
}
__device__ __forceinline__ void store_c(double* M, int ld, int row0, int col0, int r16, int kq, const d4 v) {
  double* p = M + (row0 + kq) * ld + col0 + r16;
  p[0] = v[0]; p[4 * ld] = v[1]; p[8 * ld] = v[2]; p[12 * ld] = v[3];
}

// writes the TRANSPOSE of a C-layout tile at (row0, col0)  (same addressing as frag_a)
__device__ __forceinline__ void store_ct(double* M, int ld, int row0, int col0, int r16, int kq, const d4 v) {
  double* p = M + (row0 + r16) * ld + col0 + kq;
  p[0] = v[0]; p[4] = v[1]; p[8] = v[2]; p[12] = v[3];
}
// 16x16 SPD tile A = L D L'  ->  U = L^-1 (unit lower triangular) and D^-1, by the calling wavefront
// (lane r16 = column, one register per row, the four DPP rows work redundantly).  Forward
// elimination only: row i > p gets  row_i -= (A[i][p] / d_p) * row_p, with the multiplier written
// into lane p, so that lanes c < i of row i end as U[i][c].  Accumulates log det as mantissa/exponent.
__device__ __forceinline__ void factor_pivot_tile(const double* tile, int ld, double* U, int ldu,
                                                  double* dinv, int r16, int kq,
                                                  double& pmin, double& ldM, int& ldE) {
  double A[16];
  static_for<0, 16>([&](auto r) { A[r] = tile[r * ld + r16]; });
  dpp_fence(A);
  double dv = 0.0;
  double pv = bcast_fenced<0>(A[0]);
  double rinv = rcp_nr(pv);
  double pprod = 1.0;
  static_for<0, 16>([&](auto p) {
    const double Ep = (r16 == p) ? 1.0 : 0.0;       // per-lane selects done arithmetically (x * Ep, exact)
    pmin = fmin(pmin, pv);
    pprod *= pv;
    dv = __builtin_fma(Ep, rinv, dv);
    const double r = __builtin_fma(Ep, 1.0 - pv, A[p]) * rinv;       // lane p: 1/pivot
    // row updates in groups of four: the four lane-p clears first (independent), then the four DPP
    // multiply-accumulates, so that no instruction waits for its predecessor's 8-cycle latency
    // (the exact two-instruction form: the single-FMA form of the register path, gauss_jordan in
    // lds_estep_kernel.hpp, loses a factor 3 on ill-conditioned n = 64 models here and gains nothing)
    auto update4 = [&](auto i0, auto cnt) {
      constexpr int I0 = decltype(i0)::value, C = decltype(cnt)::value;
      double olds[C], accs[C];
      static_for<0, C>([&](auto j) { olds[j] = A[I0 + j]; accs[j] = __builtin_fma(-olds[j], Ep, olds[j]); });
      static_for<0, C>([&](auto j) { mac_bc<p, true, false>(accs[j], olds[j], r); A[I0 + j] = accs[j]; });
    };
    if constexpr (p + 1 < 16) {
      // software pipelining by hand: row p+1 first, broadcast its pivot, then the reciprocal chain of
      // the NEXT pivot between the remaining row updates (cf. gauss_jordan, lds_estep_kernel.hpp)
      update4(std::integral_constant<int, p + 1>{}, std::integral_constant<int, 1>{});
      const double pn = bcast_fenced<p + 1>(A[p + 1]);
      double t0 = 0.0, e0 = 0.0, t1 = 0.0, e1 = 0.0, rn = 0.0;
      constexpr int REM = 14 - p;                      // row updates still to come
      constexpr int NG = (REM + 3) / 4;                // ... in groups of four
      auto chain = [&](auto s) {
        if constexpr (s == 0) t0 = asm_rcp(pn);
        else if constexpr (s == 1) e0 = asm_fnma1(pn, t0);
        else if constexpr (s == 2) t1 = asm_fma(t0, e0, t0);
        else if constexpr (s == 3) e1 = asm_fnma1(pn, t1);
        else if constexpr (s == 4) rn = asm_fma(t1, e1, t1);
      };
      if constexpr (NG == 0) static_for<0, 5>(chain);
      static_for<0, NG>([&](auto g) {
        constexpr int i0 = p + 2 + 4 * g;
        constexpr int c = (16 - i0) < 4 ? (16 - i0) : 4;
        constexpr int lo = g * 5 / NG, hi = (g + 1) * 5 / NG;
        static_for<lo, hi>(chain);                     // chain steps ahead of the group they overlap with
        update4(std::integral_constant<int, i0>{}, std::integral_constant<int, c>{});
      });
      pv = pn;
      rinv = rn;
    }
    if constexpr (p == 7 || p == 15) {             // keep the running product of pivots in range
      ldE += __builtin_amdgcn_frexp_exp(pprod);
      ldM *= __builtin_amdgcn_frexp_mant(pprod);
      pprod = 1.0;
    }
  });
  ldE += __builtin_amdgcn_frexp_exp(ldM);
  ldM = __builtin_amdgcn_frexp_mant(ldM);
  if (kq == 0) {
    static_for<0, 16>([&](auto r) { U[r * ldu + r16] = r16 < r ? A[r] : (r16 == r ? 1.0 : 0.0); });
    dinv[r16] = dv;
  }
}

}  // namespace svae
