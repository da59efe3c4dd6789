// hmm_estep_chunked.hip -- the HMM E-step and log-normaliser PARTITIONED IN TIME, for long sequences (K <= 16), gfx950.
//
// The serial E-step (hmm_estep.hip) runs one dependent chain per sequence, T steps deep, whatever the batch: a recording
// of 10^4 .. 10^6 frames waits for as many serial steps on one wavefront.  Here the T steps are cut into C = ceil(T / L)
// chunks of L steps (the last may be as short as one) and the chain becomes three short ones:
//   stage 1  hmm_chunk_ops_kernel   parallel over (sequence, chunk, start state): chunk c >= 1's transfer operator
//            M_c = prod_{t in chunk} P diag(e_t) as K INDEPENDENTLY SCALED rows -- row j is the scaled forward filter
//            started from the one-hot delta_j, renormalised to sum 1, its log scale s_c[j] kept beside it (a common
//            scale for the matrix would underflow the rows of improbable start states against the best one).  Chunk 0
//            is the ordinary filter from `init`.                                      depth L
//   stage 2  hmm_chunk_scan_kernel  one DPP row per sequence, serial over the chunks: the filtered message a^_c at every
//            chunk's last step (u = (a^_{c-1} o exp(s_c - max s_c)) M^_c, normalised), log Z from the normalisers and
//            the maxima, then backward the messages b^_c at every chunk's last step.    depth 2 C
//   stage 3  hmm_chunk_estep_kernel parallel over (sequence, chunk): the scaled forward-backward of the serial
//            one-directional kernel on the chunk's own steps, entered with a^_{c-1} in place of the initial message
//            and left with b^_c in place of 1; the chunk adds the transition term of the step that enters it, so the
//            C - 1 boundary terms need no pass of their own.  E_states goes to the caller's array.   depth 2 L
//            hmm_chunk_combine_kernel sums the chunks' transition counts in chunk order (no floating-point atomics).
// Mapping (all stages): one 16-lane DPP row per chain, lane k = state k, four chains per wavefront, products by
// row_newbcast multiply-accumulates (dpp.hpp) -- stage 1 with ONE ROW PER START STATE rather than the K x K operator
// in one row's registers: K times the wavefronts, each with the serial kernel's K multiply-accumulates per step, so
// a lone long sequence fills the chip (B C K / 4 wavefronts) and a chunk's latency is L short steps, not L steps of K^2.
// Range: a sequence keeps this result only while every live component -- of every operator row
// from the chunk's second step on, of chunk 0's filter, of every weighted entry a^ o exp(s - max), forward product u and
// backward product of stage 2, of stage 3's forward messages -- stays >= HMM_LOW and every normaliser above 1e-200.
// Any other sequence raises its route word and is recomputed WHOLE by the serial route (an indexed launch over the flagged
// sequences only), whose own log-space redo stands behind it.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/svae_hip.h"

#include "dpp.hpp"
#include "hmm_units.hpp"

// hmm_estep.hip: the serial E-step's launches on filled arguments
extern "C" int svae_hmm_estep_args_launch(const svae::HmmArgs* a, void* stream);

namespace svae {

struct HmmChunkedArgs {
  int B, T, K, L, C;                      // L = steps per chunk (2 <= L < T), C = ceil(T / L) >= 2
  long pair_stride;
  const double* __restrict__ init_params;
  const double* __restrict__ pair_params;
  const double* __restrict__ node_params;
  double* __restrict__ logZ;
  double* __restrict__ E_init;            // the three statistics: all NULL (logZ only) or none
  double* __restrict__ E_trans;
  double* __restrict__ E_states;
  int32_t* __restrict__ route;            // (B) route words, zeroed before stage 1
  int32_t* __restrict__ index;            // (B) slots of the recompute launch
  double* __restrict__ rec;               // (B,T,HMM_CHUNK_REC)
  double* __restrict__ ops;               // (B,C,K,K)
  double* __restrict__ scale;             // (B,C,K)
  double* __restrict__ ahat;              // (B,C,K)
  double* __restrict__ bhat;              // (B,C,K)
  double* __restrict__ ctrans;            // (B,C,K,K)
};

constexpr double HMMC_TINY = 1e-200;
constexpr int HMMC_D = 8;                 // node potentials requested this many steps ahead (stage 1)
constexpr int HMMC_NORM = 4;              // stage 1 renormalises its message every HMMC_NORM-th step
static_assert(HMMC_D % HMMC_NORM == 0, "ring positions fix the renormalisation steps");
constexpr double HMMC_LN2 = 0.6931471805599453094;

// maximum / sum over the 16 lanes of a DPP row, in every lane (the serial kernels' rotate-and-max)
template <int R>
__device__ __forceinline__ double chunk_row_ror(double x) {
  const int lo = __builtin_amdgcn_update_dpp(0, __double2loint(x), 0x120 + R, 0xf, 0xf, false);
  const int hi = __builtin_amdgcn_update_dpp(0, __double2hiint(x), 0x120 + R, 0xf, 0xf, false);
  return __hiloint2double(hi, lo);
}
__device__ __forceinline__ double chunk_row_max(double x) {
  x = __builtin_fmax(x, chunk_row_ror<8>(x));
  x = __builtin_fmax(x, chunk_row_ror<4>(x));
  x = __builtin_fmax(x, chunk_row_ror<2>(x));
  x = __builtin_fmax(x, chunk_row_ror<1>(x));
  return x;
}
// sum over the K live lanes of the row (idle lanes hold 0), two accumulators: half the dependent chain
template <int K>
__device__ __forceinline__ double chunk_row_sum(double x) {
  double one = 1.0, s0 = 0.0, s1 = 0.0;
  dpp_fence(x);
  static_for<0, K>([&](auto k) { if constexpr (k % 2 == 0) mac_bc<k>(s0, x, one); else mac_bc<k>(s1, x, one); });
  return s0 + s1;
}

// this row's transition matrix in the register layout of the serial kernels: P[j] (lane c) = exp(pair[j][c] - max),
// PT[k] (lane c) = exp(pair[c][k] - max), 0 in idle lanes; returns the maximum
template <int K, bool WITH_T>
__device__ __forceinline__ double chunk_load_pair(const double* __restrict__ pp, bool col, int cc, double (&P)[K],
                                                  double (&PT)[K]) {
  const double NEG_BIG = -1.0e300;
  double lp[K];
  [[maybe_unused]] double lpT[K];
  static_for<0, K>([&](auto j) {
    const double v = pp[j * K + cc];
    lp[j] = col ? v : NEG_BIG;
    if constexpr (WITH_T) { const double vt = pp[cc * K + j]; lpT[j] = col ? vt : NEG_BIG; }
  });
  double pmax = NEG_BIG;
  static_for<0, K>([&](auto j) { pmax = fmax(pmax, lp[j]); });
  pmax = chunk_row_max(pmax);
  static_for<0, K>([&](auto j) {
    P[j] = col ? exp(lp[j] - pmax) : 0.0;
    if constexpr (WITH_T) PT[j] = col ? exp(lpT[j] - pmax) : 0.0;
  });
  return pmax;
}

// ---- stage 1: chunk operators --------------------------------------------------------------------------------------------
// row r = (b, chunk, j): j fastest, so the K rows of an operator share wavefronts and their node potentials' cache lines.
// Chunk 0 has the one row j = 0 (its other rows idle).  The trip count is the full chunk length L for every row of the
// wavefront; a row of the short last chunk runs its tail on its last step's data under a mask and keeps nothing of it.
template <int K>
__global__ __launch_bounds__(64) void hmm_chunk_ops_kernel(const HmmChunkedArgs a) {
  constexpr int D = HMMC_D;
  const int lane = threadIdx.x;
  const int c = lane & 15;
  const long rows = (long)a.B * a.C * K;
  const long r0 = (long)blockIdx.x * 4 + (lane >> 4);
  const long r = r0 < rows ? r0 : rows - 1;
  const int j = (int)(r % K);
  const long q = r / K;                               // (b, chunk)
  const int ch = (int)(q % a.C);
  const long b = q / a.C;
  const bool valid = r0 < rows && (ch > 0 || j == 0);
  if (!__any(valid)) return;
  const bool col = c < K;
  const int cc = col ? c : 0;
  const bool st = valid && col;
  const double NEG_BIG = -1.0e300;
  const int L = a.L;
  const int t0 = ch * L;
  const int n = a.T - t0 < L ? a.T - t0 : L;          // this chunk's steps (>= 1)

  double P[K], PT_unused[K];
  const double pmax = chunk_load_pair<K, false>(a.pair_params + b * a.pair_stride, col, cc, P, PT_unused);
  const double* nodep = a.node_params + ((long)b * a.T + t0) * K + cc;
  const bool head = ch == 0;                          // the filter from `init`
  const double init = head ? a.init_params[cc] : 0.0;
  const double colone = col ? 1.0 : 0.0;

  double alpha = head ? 0.0 : (c == j ? 1.0 : 0.0);   // delta_j (head: step 0 sets it)
  double lzM = 1.0, lzS = 0.0;
  long lzE = 0;
  bool bad = false;
  auto clampn = [&](int i) { return i < n ? i : n - 1; };
  auto step = [&](int i, double ndraw, auto norm, auto renorm) {
    const bool live = i < n;
    const bool first = head && i == 0;
    const double nd = col ? ndraw + (first ? init : 0.0) : NEG_BIG;
    const double m = chunk_row_max(nd);
    const double e = col ? exp_nonpos(nd - m) : 0.0;
    double p0 = 0.0, p1 = 0.0;
    dpp_fence(alpha);
    static_for<0, K>([&](auto jj) { if constexpr (jj % 2 == 0) mac_bc<jj>(p0, alpha, P[jj]); else mac_bc<jj>(p1, alpha, P[jj]); });
    const double pred = __builtin_fma(first ? 1.0 : 0.0, colone, p0 + p1);        // (head: alpha starts at 0)
    double al = pred * e;
    // (an operator row's first step is P[j][:] o e: its zeros are exact and what it drops is absolute -- checked from
    //  the second step on; chunk 0 is a message from its first step)
    bad = bad || (live && (head || i > 0) && col && !(al >= HMM_LOW));
    if constexpr (decltype(norm)::value) {
      const double cs = chunk_row_sum<K>(al);
      bad = bad || (live && !(cs > HMMC_TINY));
      al *= rcp_nr(cs);
      lzM = live ? lzM * __builtin_amdgcn_frexp_mant(cs) : lzM;
      lzE += live ? __builtin_amdgcn_frexp_exp(cs) : 0;
    }
    alpha = live ? al : alpha;
    lzS += live ? m + (first ? 0.0 : pmax) : 0.0;
    if constexpr (decltype(renorm)::value) { lzE += __builtin_amdgcn_frexp_exp(lzM); lzM = __builtin_amdgcn_frexp_mant(lzM); }
  };
  {
    double ring[D];
    static_for<0, D>([&](auto u) { ring[u] = nodep[(long)clampn(u) * K]; });
    int i = 0;
    for (; i + D <= L; i += D) {
      static_for<0, D>([&](auto u) {
        const double x = ring[u];
        ring[u] = nodep[(long)clampn(i + u + D) * K];
        step(i + u, x, std::integral_constant<bool, (u % HMMC_NORM) == HMMC_NORM - 1>{}, std::integral_constant<bool, u == D - 1>{});
      });
    }
    static_for<0, D>([&](auto u) {
      if (i + u < L) step(i + u, ring[u], std::integral_constant<bool, (u % HMMC_NORM) == HMMC_NORM - 1>{},
                          std::integral_constant<bool, u == D - 1>{});
    });
  }
  {
    // what the last renormalisation left unscaled
    const double fs = chunk_row_sum<K>(alpha);
    bad = bad || !(fs > HMMC_TINY);
    alpha *= rcp_nr(fs);
    lzM *= __builtin_amdgcn_frexp_mant(fs);
    lzE += __builtin_amdgcn_frexp_exp(fs);
  }
  if (st) a.ops[(q * K + j) * K + c] = alpha;
  if (valid && c == 0) a.scale[q * K + j] = lzS + ::log(lzM) + (double)lzE * HMMC_LN2;
  // (`bad` is per lane: the row's sixteen bits of the ballot; every writer of a route word writes the same 1)
  if (((__ballot(bad) >> (lane & 48)) & 0xffffull) != 0 && valid && c == 0) a.route[b] = 1;
}

// ---- stage 2: boundary scan ------------------------------------------------------------------------------------------------
// one DPP row per sequence; the next chunk's operator and scales are requested before the current one is used
template <int K>
__global__ __launch_bounds__(64) void hmm_chunk_scan_kernel(const HmmChunkedArgs a) {
  const int lane = threadIdx.x;
  const int c = lane & 15;
  const long b0 = (long)blockIdx.x * 4 + (lane >> 4);
  const bool valid = b0 < a.B;
  const long b = valid ? b0 : a.B - 1;
  const bool col = c < K;
  const int cc = col ? c : 0;
  const bool st = valid && col;
  const double NEG_BIG = -1.0e300;
  const int C = a.C;
  const double* ops = a.ops + b * C * K * K;
  const double* scale = a.scale + b * C * K;
  bool bad = false;

  // forward: a^_0 and its log scale are chunk 0's row 0
  double ah = col ? ops[cc] : 0.0;
  double lzS = scale[0], lzM = 1.0;
  long lzE = 0;
  if (st) a.ahat[b * C * K + c] = ah;
  {
    double Mn[K], sn;
    auto request = [&](int ch) {
      static_for<0, K>([&](auto jj) { Mn[jj] = ops[((long)ch * K + jj) * K + cc]; });      // lane k: M^[jj][k]
      sn = scale[(long)ch * K + cc];                                                       // lane j: s[j]
    };
    request(1);
    for (int ch = 1; ch < C; ++ch) {
      double M[K];
      static_for<0, K>([&](auto jj) { M[jj] = Mn[jj]; });
      const double s = col ? sn : NEG_BIG;
      request(ch + 1 < C ? ch + 1 : ch);
      const double smax = chunk_row_max(s);
      double w = col ? ah * exp_nonpos(s - smax) : 0.0;
      bad = bad || (col && !(w >= HMM_LOW));
      double u0 = 0.0, u1 = 0.0;
      dpp_fence(w);
      static_for<0, K>([&](auto jj) { if constexpr (jj % 2 == 0) mac_bc<jj>(u0, w, M[jj]); else mac_bc<jj>(u1, w, M[jj]); });
      double u = col ? u0 + u1 : 0.0;
      bad = bad || (col && !(u >= HMM_LOW));
      const double su = chunk_row_sum<K>(u);
      bad = bad || !(su > HMMC_TINY);
      ah = u * rcp_nr(su);
      if (st) a.ahat[(b * C + ch) * K + c] = ah;
      lzS += smax;
      lzM *= __builtin_amdgcn_frexp_mant(su);
      lzE += __builtin_amdgcn_frexp_exp(su);
      if ((ch & 15) == 15) { lzE += __builtin_amdgcn_frexp_exp(lzM); lzM = __builtin_amdgcn_frexp_mant(lzM); }
    }
  }
  if (valid && c == 0) a.logZ[b] = lzS + ::log(lzM) + (double)lzE * HMMC_LN2;

  // backward (not for logZ alone): b^_{C-1} = 1;  b_{c-1} = exp(s_c - max) o (M^_c b^_c), renormalised
  if (a.E_states) {
    double be = col ? 1.0 : 0.0;
    if (st) a.bhat[(b * C + (C - 1)) * K + c] = be;
    double Mn[K], sn;
    auto request = [&](int ch) {
      static_for<0, K>([&](auto k) { Mn[k] = ops[((long)ch * K + cc) * K + k]; });         // lane j: M^[j][k]
      sn = scale[(long)ch * K + cc];
    };
    request(C - 1);
    for (int ch = C - 1; ch >= 1; --ch) {
      double M[K];
      static_for<0, K>([&](auto k) { M[k] = Mn[k]; });
      const double s = col ? sn : NEG_BIG;
      request(ch > 1 ? ch - 1 : ch);
      const double smax = chunk_row_max(s);
      double q0 = 0.0, q1 = 0.0;
      dpp_fence(be);
      static_for<0, K>([&](auto k) { if constexpr (k % 2 == 0) mac_bc<k>(q0, be, M[k]); else mac_bc<k>(q1, be, M[k]); });
      double bw = col ? (q0 + q1) * exp_nonpos(s - smax) : 0.0;
      bad = bad || (col && !(bw >= HMM_LOW));
      const double sb = chunk_row_sum<K>(bw);
      bad = bad || !(sb > HMMC_TINY);
      be = bw * rcp_nr(sb);
      if (st) a.bhat[(b * C + (ch - 1)) * K + c] = be;
    }
  }
  if (((__ballot(bad) >> (lane & 48)) & 0xffffull) != 0 && valid && c == 0) a.route[b] = 1;
}

// ---- stage 3: the E-step of every chunk ------------------------------------------------------------------------------------
// The serial one-directional kernel (hmm_estep.hip) on the chunk's steps: forward from a^_{c-1} (chunk 0: from `init`),
// backward from b^_c scaled so that <alpha^, beta> = 1 at the chunk's last step -- the e_t / c_t scaling of the backward
// pass keeps that product 1 at every step, so gamma_t = alpha^_t o beta_t and the xi terms need no normaliser.  The
// transition INTO the chunk is the same xi term with alpha^ = a^_{c-1}: the chunk adds it to its own counts.
// Trip count L for every row of the wavefront; a row of the short last chunk runs under masks, as the ragged serial kernel.
template <int K>
__global__ __launch_bounds__(64) void hmm_chunk_estep_kernel(const HmmChunkedArgs a) {
  const int lane = threadIdx.x;
  const int c = lane & 15;
  const long rows = (long)a.B * a.C;
  const long q0 = (long)blockIdx.x * 4 + (lane >> 4);
  const bool valid = q0 < rows;
  const long q = valid ? q0 : rows - 1;
  const int ch = (int)(q % a.C);
  const long b = q / a.C;
  const bool col = c < K;
  const int cc = col ? c : 0;
  const bool st = valid && col;
  const double NEG_BIG = -1.0e300;
  const int L = a.L, T = a.T;
  const int t0 = ch * L;
  const int n = T - t0 < L ? T - t0 : L;
  const bool head = ch == 0;

  double P[K], PT[K];
  const double pmax = chunk_load_pair<K, true>(a.pair_params + b * a.pair_stride, col, cc, P, PT);
  (void)pmax;
  const double* nodep = a.node_params + ((long)b * T + t0) * K + cc;
  double* rec = a.rec + ((long)b * T + t0) * HMM_CHUNK_REC + c;
  double* oS = a.E_states + ((long)b * T + t0) * K + cc;
  const double init = head ? a.init_params[cc] : 0.0;
  const double aprev_ld = a.ahat[(head ? q : q - 1) * K + cc];               // (index inside the array for chunk 0 too)
  const double aprev = (col && !head) ? aprev_ld : 0.0;                      // a^_{c-1}
  const double bend = col ? a.bhat[q * K + cc] : 0.0;                        // b^_c
  bool bad = false;

  // ---- forward
  double alpha = aprev;
  double nd_n = nodep[0];
  for (int i = 0; i < L; ++i) {
    const bool live = i < n;
    const bool first = head && i == 0;
    const double nd = col ? nd_n + (first ? init : 0.0) : NEG_BIG;
    nd_n = nodep[(long)(i + 1 < n ? i + 1 : n - 1) * K];                     // next step's, unconditionally (clamped)
    const double m = chunk_row_max(nd);
    const double e = col ? exp_nonpos(nd - m) : 0.0;
    // (no branch on `first`: it differs between the rows of a wavefront; chunk 0's alpha starts at 0)
    double pred = (first && col) ? 1.0 : 0.0;
    dpp_fence(alpha);
    static_for<0, K>([&](auto jj) { mac_bc<jj>(pred, alpha, P[jj]); });
    const double al = pred * e;
    const double cs = chunk_row_sum<K>(al);
    const double rc = rcp_nr(cs);
    bad = bad || (live && ((col && !(al >= HMM_LOW)) || !(cs > HMMC_TINY)));
    alpha = live ? al * rc : alpha;
    if (valid && live) { rec[(long)i * HMM_CHUNK_REC] = alpha; rec[(long)i * HMM_CHUNK_REC + 16] = e * rc; }
  }

  // ---- backward + statistics
  double beta;
  {
    const double z = chunk_row_sum<K>(alpha * bend);
    bad = bad || !(z > HMMC_TINY);
    beta = bend * rcp_nr(z);
    const double gam = alpha * beta;                       // the chunk's last step
    if (st) oS[(long)(n - 1) * K] = gam;
    if (head && n == 1 && st) a.E_init[b * K + c] = gam;
  }
  double acc[K];
  static_for<0, K>([&](auto jj) { acc[jj] = 0.0; });
  // (u, alpha) one step ahead, record indices clamped into the chunk's own steps
  auto rec_hi = [&](int i) -> long { return (long)(i < n - 1 ? i : (n > 1 ? n - 1 : 0)); };
  auto rec_lo = [&](int i) -> long { return (long)(i < n - 2 ? i : (n > 2 ? n - 2 : 0)); };
  double u_n = rec[rec_hi(L - 1) * HMM_CHUNK_REC + 16], al_n = rec[rec_lo(L - 2 > 0 ? L - 2 : 0) * HMM_CHUNK_REC];
  for (int i = L - 2; i >= 0; --i) {
    const double u = u_n;                                  // e_{i+1} / c_{i+1}
    const double al = al_n;
    const bool act = i <= n - 2;
    {
      const int ip = i > 0 ? i - 1 : 0;
      u_n = rec[rec_hi(ip + 1) * HMM_CHUNK_REC + 16];
      al_n = rec[rec_lo(ip) * HMM_CHUNK_REC];
    }
    double w = act ? u * beta : 0.0;
    double al_f = act ? al : 0.0;
    dpp_fence(w);
    dpp_fence(al_f);
    double bn = 0.0;
    static_for<0, K>([&](auto k) { mac_bc<k>(bn, w, PT[k]); });             // beta_i[j] = sum_k P[j][k] w[k]
    static_for<0, K>([&](auto jj) { mac_bc<jj>(acc[jj], al_f, w); });       // xi sums (without P)
    beta = act ? bn : beta;
    const double gam = al * beta;
    if (st && act) oS[(long)i * K] = gam;
    if (head && i == 0 && st && act) a.E_init[b * K + c] = gam;
  }
  {
    // the transition into the chunk: alpha^ = a^_{c-1}, w of the chunk's first step (chunk 0: aprev = 0, adds nothing)
    double w = rec[16] * beta;
    w = (col && !head) ? w : 0.0;
    double ap = aprev;
    dpp_fence(w);
    dpp_fence(ap);
    static_for<0, K>([&](auto jj) { mac_bc<jj>(acc[jj], ap, w); });
  }
  if (st) static_for<0, K>([&](auto jj) { a.ctrans[(q * K + jj) * K + c] = acc[jj] * P[jj]; });
  if (((__ballot(bad) >> (lane & 48)) & 0xffffull) != 0 && valid && c == 0) a.route[b] = 1;
}

// E_trans[b] = the chunks' counts summed in chunk order: one thread per entry
__global__ __launch_bounds__(256) void hmm_chunk_combine_kernel(const HmmChunkedArgs a) {
  const long kk = (long)a.K * a.K;
  const long e = (long)blockIdx.x * 256 + threadIdx.x;
  if (e >= a.B * kk) return;
  const long b = e / kk, jk = e - b * kk;
  const double* ct = a.ctrans + b * a.C * kk + jk;
  double s = 0.0;
  for (int ch = 0; ch < a.C; ++ch) s += ct[(long)ch * kk];
  a.E_trans[e] = s;
}

// the flagged sequences as the compacted slot list of an indexed launch (stable order), the slots behind it -1: one wavefront
__global__ __launch_bounds__(64) void hmm_chunk_index_kernel(int B, const int32_t* __restrict__ route, int32_t* __restrict__ index) {
  const int lane = threadIdx.x;
  int count = 0;
  for (int base = 0; base < B; base += 64) {
    const int b = base + lane;
    const bool f = b < B && route[b] != 0;
    const unsigned long long mask = __ballot(f);
    if (f) index[count + __popcll(mask & ((1ull << lane) - 1ull))] = b;
    count += __popcll(mask);
  }
  for (int i = count + lane; i < B; i += 64) index[i] = -1;
}

template <int K>
static int launch_chunked(const HmmChunkedArgs& a, hipStream_t s) {
  const long op_rows = (long)a.B * a.C * K, seq_rows = (long)a.B * a.C;
  hipLaunchKernelGGL((hmm_chunk_ops_kernel<K>), dim3((unsigned)((op_rows + 3) / 4)), dim3(64), 0, s, a);
  hipLaunchKernelGGL((hmm_chunk_scan_kernel<K>), dim3((unsigned)((a.B + 3) / 4)), dim3(64), 0, s, a);
  if (a.E_states) {
    hipLaunchKernelGGL((hmm_chunk_estep_kernel<K>), dim3((unsigned)((seq_rows + 3) / 4)), dim3(64), 0, s, a);
    hipLaunchKernelGGL(hmm_chunk_combine_kernel, dim3((unsigned)(((long)a.B * K * K + 255) / 256)), dim3(256), 0, s, a);
  }
  hipLaunchKernelGGL(hmm_chunk_index_kernel, dim3(1), dim3(64), 0, s, a.B, a.route, a.index);
  return hipGetLastError() == hipSuccess ? 0 : -1000;
}

}  // namespace svae

// Stages 1 and 2 alone -- chunk operators and the forward boundary scan, the log-Z-only form -- on a caller's buffers
// (hmm_sample_chunked.hip): logZ, ahat and the route words as svae_hmm_chunked_estep_f64 leaves them at this chunk.  The
// route words are the caller's to zero; no recompute launch follows.  Host only: the kernels are the ones above.
extern "C" int svae_hmm_chunked_forward_launch(int B, int T, int K, int L, int C, long pair_stride,
                                               const double* init_params, const double* pair_params,
                                               const double* node_params, double* logZ, int32_t* route, double* ops,
                                               double* scale, double* ahat, void* stream) {
  svae::HmmChunkedArgs a;
  svae::hmm_set_model(a, B, T, K, pair_stride, init_params, pair_params, node_params);
  a.L = L; a.C = C;
  a.logZ = logZ; a.E_init = nullptr; a.E_trans = nullptr; a.E_states = nullptr;
  a.route = route; a.index = nullptr; a.rec = nullptr;
  a.ops = ops; a.scale = scale; a.ahat = ahat; a.bhat = nullptr; a.ctrans = nullptr;
  hipStream_t s = (hipStream_t)stream;
  return svae::hmm_dispatch_k(
      K,
      [&](auto k) {
        const long op_rows = (long)a.B * a.C * k;
        hipLaunchKernelGGL((svae::hmm_chunk_ops_kernel<k>), dim3((unsigned)((op_rows + 3) / 4)), dim3(64), 0, s, a);
        hipLaunchKernelGGL((svae::hmm_chunk_scan_kernel<k>), dim3((unsigned)((a.B + 3) / 4)), dim3(64), 0, s, a);
        return hipGetLastError() == hipSuccess ? 0 : -1000;
      },
      [&](auto) { return -3; });
}

// The chunk the library picks, from tools/bench_hmm_chunked.py on one MI355X (K = 8 and 16; DESIGN 4.5k has the table).
// Chunked beat the serial call, by far more than the windows' spread (<= 5 %), at every measured shape with T >= 500 and
// B <= 128 -- 1.3x - 1.8x at T = 500, 3x - 7x at T = 5000, 8x - 24x at T = 50000 -- and lost at 512 x 500 (and, at
// K = 16, at 512 x 5000): batches above 128 sequences and sequences shorter than 500 steps stay serial (return T).  The
// fastest chunk was 32 / 64 / 256 at T = 500 / 5000 / 50000 for both K, i.e. the power of two nearest 1.2 sqrt(T); at
// 32 and 128 sequences that pick is within 4 % of the best measured.
extern "C" int svae_hmm_chunked_default_chunk(int B, int T, int K) {
  if (B < 1 || T < 1 || K < 1 || K > svae::HMM_CHUNKED_MAX_K) return T;
  if (T < 500 || B > 128) return T;
  long L = 2;
  while (200 * L * L <= 144 * (long)T) L *= 2;          // 2^round(log2(1.2 sqrt(T)))
  return L < T ? (int)L : T;
}

extern "C" size_t svae_hmm_chunked_workspace_bytes(int B, int T, int K, int chunk) {
  if (B <= 0 || T <= 0 || K <= 0 || K > svae::HMM_CHUNKED_MAX_K || chunk < 2) return 0;
  return (size_t)svae::hmm_chunked_layout(B, T, K, chunk).total * sizeof(double);
}

extern "C" int svae_hmm_chunked_estep_f64(int B, int T, int K, int pair_batched, int chunk,
                                          const double* init_params, const double* pair_params,
                                          const double* node_params,
                                          double* logZ, double* E_init, double* E_trans, double* E_states,
                                          void* workspace, size_t ws_bytes, void* stream) {
  // hmm_check_model's -1 .. -6 with this unit's bound on K in its place: -3 comes before -4 .. -6
  const int rc_model = svae::hmm_check_model(B, T, K, pair_batched, init_params, pair_params);
  if (rc_model <= -1 && rc_model >= -3) return rc_model;
  if (K > svae::HMM_CHUNKED_MAX_K) return -3;
  if (rc_model) return rc_model;
  if (B == 0) return 0;
  if (chunk < 2) return -7;
  if (!node_params) return -8;
  if (!logZ) return -9;
  const int nstats = (E_init != nullptr) + (E_trans != nullptr) + (E_states != nullptr);
  if (nstats != 0 && nstats != 3) return -10;
  if (!workspace) return -11;
  if (ws_bytes < svae_hmm_chunked_workspace_bytes(B, T, K, chunk)) return -12;
  const svae::HmmChunkedLayout lay = svae::hmm_chunked_layout(B, T, K, chunk);
  double* ws = (double*)workspace;
  const long pair_stride = pair_batched ? (long)K * K : 0;
  hipStream_t s = (hipStream_t)stream;

  // the serial route's arguments: the whole call where one chunk holds the sequence, else the flagged sequences
  svae::HmmArgs h;
  svae::hmm_set_model(h, B, T, K, pair_stride, init_params, pair_params, node_params);
  h.logZ = logZ;
  h.E_states = nstats ? E_states : ws + lay.stats;
  h.E_trans = nstats ? E_trans : ws + lay.stats + (long)B * T * K;
  h.E_init = nstats ? E_init : ws + lay.stats + (long)B * T * K + (long)B * K * K;
  h.ws = ws + lay.serial;
  h.seq_index = nullptr; h.n = 0; h.pair_contr = nullptr; h.lds_E_init = nullptr; h.init_J = nullptr; h.init_h = nullptr;
  h.cinit = nullptr; h.lz = nullptr; h.node_out = nullptr;
  if (chunk >= T) return svae_hmm_estep_args_launch(&h, stream);

  svae::HmmChunkedArgs a;
  svae::hmm_set_model(a, B, T, K, pair_stride, init_params, pair_params, node_params);
  a.L = chunk; a.C = (int)lay.C;
  a.logZ = logZ; a.E_init = E_init; a.E_trans = E_trans; a.E_states = E_states;
  a.route = (int32_t*)(ws + lay.route);
  a.index = a.route + B;
  a.rec = ws + lay.serial;
  a.ops = ws + lay.ops; a.scale = ws + lay.scale; a.ahat = ws + lay.ahat; a.bhat = ws + lay.bhat; a.ctrans = ws + lay.ctrans;
  if (hipMemsetAsync(a.route, 0, sizeof(int32_t) * (size_t)B, s) != hipSuccess) return -1000;
  const int rc = svae::hmm_dispatch_k(
      K, [&](auto k) { return svae::launch_chunked<k>(a, s); }, [&](auto) { return -3; });
  if (rc) return rc;
  h.seq_index = a.index;
  return svae_hmm_estep_args_launch(&h, stream);
}
