// hmm_viterbi_chunked.hip -- HMM Viterbi decoding PARTITIONED IN TIME, for long sequences (K <= 16), gfx950.
//
// The serial decoder (hmm_viterbi.hip) runs one dependent chain of T max-plus steps and a backtrace of T look-ups per
// sequence, whatever the batch.  Here the T steps are cut into C = ceil(T / L) chunks of L steps (the last may be as
// short as one) and the two chains become five short ones and a flat pass.  step(d, t)[k] = (max_j (d[j] + pair[j][k]))
// + node[t][k] is the serial recursion's step: fp64 adds in that order, a running maximum with strict `>` (lowest j on ties).
//   stage 1  hmm_vchunk_ops_kernel     parallel over (sequence, chunk, start state): row j of chunk c >= 1's max-plus
//            operator M_c starts as pair[j][:] + node[t0][:] and takes `step` over t0+1 .. t1-1; chunk 0 is the ordinary
//            recursion from `init`, its end vector D_0.  Values only: no scaling, no back-pointers.        depth L
//   stage 2  hmm_vchunk_scan_kernel    one DPP row per sequence, serial over the chunks:
//            D_c[k] = max_j (D_{c-1}[j] + M_c[j][k]), running maximum in j order; the next operator is requested before
//            the current one is used.                                                                      depth C
//   stage 3  hmm_vchunk_decode_kernel  parallel over (sequence, chunk): enter with D_{c-1} (chunk 0: init + node[0]), run
//            `step` over the chunk's own steps (step t0 included for c >= 1) storing one back-pointer byte per step and
//            state; the last chunk yields z_{T-1} (lowest k attaining the maximum of its final delta) and the score.  Then
//            the chase INSIDE the chunk from all K end states at once: lane k starts at end state k and follows the
//            back-pointers down to t0 -- 16 steps at a time, each step's 16 bytes packed into a 64-bit word of nibbles
//            (vit_pack16), so the chain is a row broadcast, a shift and a mask per step --, storing its candidate label at
//            every step and f_c[k] = psi_{t0}[.], the end state of chunk c-1 it arrives at.                 depth L + L
//   stage 4  hmm_vchunk_resolve_kernel one thread per sequence: e_{C-1} = z_{T-1}, e_{c-1} = f_c[e_c]; the 16-byte rows
//            of f are requested ahead of the chain, which stays in registers.                               depth C
//   stage 5  hmm_vchunk_gather_kernel  flat over (sequence, step): states[b,t] = candidate[b, t, e_{c(t)}].
// Mapping (stages 1 - 3): one 16-lane DPP row per chain, lane k = state k, four chains per wavefront, delta[j] by
// row_newbcast (dpp.hpp bcast<j>), as hmm_viterbi_row_kernel; stage 1 with ONE ROW PER START STATE, j fastest, so the K rows
// of an operator share wavefronts and their node potentials' cache lines.  A wavefront's trip count is the full chunk
// length L; a row of the short last chunk runs its tail under a mask on its last step's data and keeps nothing of it.
// No atomics anywhere: labels and score are reproducible bit for bit, and a NumPy restatement of the five stages
// reproduces them (tests/_hmm_viterbi_chunked_numpy.py).  Against the serial decoder (include/svae_hip.h): equal bit for
// bit wherever every add of the recursion is exact (max-plus is then associative, D_{c-1} IS the serial delta); otherwise
// the boundary deltas differ from the serial ones in rounding and the path is optimal to that rounding.  NaN inputs lose
// every compare: every back-pointer, map entry and end state is an index below 16 (below K along the resolved path),
// every look-up is masked to its row -- unspecified labels in 0..K-1, no fault.  Built without fast-math.
// Candidates do NOT alias the back-pointers: a buffer of their own, B T 16 bytes.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/svae_hip.h"

#include "dpp.hpp"
#include "hmm_units.hpp"
#include "hmm_viterbi_kernel.hpp"         // vit_pack16, vit_bcast_u64, VIT_AHEAD (no kernel of it is instantiated here)

namespace svae {

struct ViterbiChunkedArgs {
  int B, T, K, L, C;                      // L = steps per chunk (2 <= L < T), C = ceil(T / L) >= 2
  long pair_stride;
  const double* __restrict__ init_params;
  const double* __restrict__ pair_params;
  const double* __restrict__ node_params;
  int32_t* __restrict__ states;           // (B,T)
  double* __restrict__ score;             // (B) or nullptr
  uint8_t* psi;                           // (B,T,16) back-pointers
  uint8_t* cand;                          // (B,T,16) candidate labels: [b][t][k] = the label at t of the path that ends
                                          //          t's chunk in state k
  uint8_t* fmap;                          // (B,C,16) f_c[k]
  uint8_t* ends;                          // (B,C)    e_c
  double* ops;                            // (B,C,K,K) (chunk 0's block is not used)
  double* delta;                          // (B,C,K)  D_c
};

// max_j (d[j] + P[j]) as the serial kernel's running maximum; the _arg form also gives the lowest j attaining it
template <int K>
__device__ __forceinline__ double vchunk_maxplus(double d, const double (&P)[K]) {
  double best = bcast<0>(d) + P[0];
  static_for<1, K>([&](auto j) {
    const double v = bcast<j>(d) + P[j];
    best = v > best ? v : best;
  });
  return best;
}
template <int K>
__device__ __forceinline__ double vchunk_maxplus_arg(double d, const double (&P)[K], int& arg) {
  double best = bcast<0>(d) + P[0];
  arg = 0;
  static_for<1, K>([&](auto j) {
    const double v = bcast<j>(d) + P[j];
    const bool w = v > best;                          // strict: the first (lowest) j keeps a tie
    best = w ? v : best;
    arg = w ? (int)j : arg;
  });
  return best;
}

// ---- stage 1: chunk operators --------------------------------------------------------------------------------------------
// row r = (b, chunk, j), j fastest.  Chunk 0 has the one row j = 0 (its other rows idle).
template <int K>
__global__ __launch_bounds__(64) void hmm_vchunk_ops_kernel(const ViterbiChunkedArgs a) {
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
  const double NEG_INF = -__builtin_inf();
  const int L = a.L;
  const int t0 = ch * L;
  const int n = a.T - t0 < L ? a.T - t0 : L;          // this chunk's steps (>= 1)
  const bool head = ch == 0;

  const double* pp = a.pair_params + b * a.pair_stride;
  double P[K];                                        // P[jj] = pair[jj][c]
  static_for<0, K>([&](auto jj) { P[jj] = pp[jj * K + cc]; });
  const double* node = a.node_params + (b * a.T + t0) * K + cc;
  const double start = head ? a.init_params[cc] : pp[j * K + cc];

  double d = col ? start + node[0] : NEG_INF;
  auto load = [&](int i) -> double { return node[(long)(i < n ? i : n - 1) * K]; };
  double cur[VIT_AHEAD], nxt[VIT_AHEAD];
  static_for<0, VIT_AHEAD>([&](auto u) { cur[u] = load(1 + u); });
  for (int i0 = 1; i0 < L; i0 += VIT_AHEAD) {
    static_for<0, VIT_AHEAD>([&](auto u) { nxt[u] = load(i0 + VIT_AHEAD + u); });
    static_for<0, VIT_AHEAD>([&](auto u) {
      const int i = i0 + u;
      if (i < L) {                                    // (wave-uniform)
        const double best = vchunk_maxplus<K>(d, P);
        const double dn = col ? best + cur[u] : NEG_INF;
        d = i < n ? dn : d;
      }
    });
    static_for<0, VIT_AHEAD>([&](auto u) { cur[u] = nxt[u]; });
  }
  if (valid && col) {
    if (head) a.delta[q * K + c] = d;
    else a.ops[(q * K + j) * K + c] = d;
  }
}

// ---- stage 2: boundary scan ------------------------------------------------------------------------------------------------
template <int K>
__global__ __launch_bounds__(64) void hmm_vchunk_scan_kernel(const ViterbiChunkedArgs a) {
  const int lane = threadIdx.x;
  const int c = lane & 15;
  const long b0 = (long)blockIdx.x * 4 + (lane >> 4);
  const bool valid = b0 < a.B;
  const long b = valid ? b0 : a.B - 1;
  const bool col = c < K;
  const int cc = col ? c : 0;
  const double NEG_INF = -__builtin_inf();
  const int C = a.C;
  const double* ops = a.ops + b * C * K * K;
  double* dl = a.delta + b * C * K;

  const double d0 = dl[cc];                           // D_0: chunk 0's recursion (stage 1)
  double D = col ? d0 : NEG_INF;
  double Mn[K];
  auto request = [&](int ch) { static_for<0, K>([&](auto jj) { Mn[jj] = ops[((long)ch * K + jj) * K + cc]; }); };  // lane k: M[jj][k]
  request(1);
  for (int ch = 1; ch < C; ++ch) {
    double M[K];
    static_for<0, K>([&](auto jj) { M[jj] = Mn[jj]; });
    request(ch + 1 < C ? ch + 1 : ch);
    const double best = vchunk_maxplus<K>(D, M);
    D = col ? best : NEG_INF;
    if (valid && col) dl[(long)ch * K + c] = D;
  }
}

// ---- stage 3: decode every chunk -------------------------------------------------------------------------------------------
template <int K>
__global__ __launch_bounds__(64) void hmm_vchunk_decode_kernel(const ViterbiChunkedArgs a) {
  const int lane = threadIdx.x;
  const int c = lane & 15;
  const long rows = (long)a.B * a.C;
  const long q0 = (long)blockIdx.x * 4 + (lane >> 4);
  const bool valid = q0 < rows;                       // idle rows repeat the last chunk and store nothing
  const long q = valid ? q0 : rows - 1;
  const int ch = (int)(q % a.C);
  const long b = q / a.C;
  const bool col = c < K;
  const int cc = col ? c : 0;
  const double NEG_INF = -__builtin_inf();
  const int L = a.L, T = a.T;
  const int t0 = ch * L;
  const int n = T - t0 < L ? T - t0 : L;
  const bool head = ch == 0;

  const double* pp = a.pair_params + b * a.pair_stride;
  double P[K];
  static_for<0, K>([&](auto jj) { P[jj] = pp[jj * K + cc]; });
  const double* node = a.node_params + (b * T + t0) * K + cc;
  uint8_t* psi = a.psi + (b * T + t0) * 16 + c;
  const double enter = a.delta[(head ? q : q - 1) * K + cc];        // D_{c-1} (chunk 0: an index inside the array, not used)
  const double first = a.init_params[cc] + node[0];
  double d = col ? (head ? first : enter) : NEG_INF;

  auto load = [&](int i) -> double { return node[(long)(i < n ? i : n - 1) * K]; };
  double cur[VIT_AHEAD], nxt[VIT_AHEAD];
  static_for<0, VIT_AHEAD>([&](auto u) { cur[u] = load(u); });
  for (int i0 = 0; i0 < L; i0 += VIT_AHEAD) {
    static_for<0, VIT_AHEAD>([&](auto u) { nxt[u] = load(i0 + VIT_AHEAD + u); });
    static_for<0, VIT_AHEAD>([&](auto u) {
      const int i = i0 + u;
      if (i < L) {                                    // (wave-uniform)
        int arg;
        const double best = vchunk_maxplus_arg<K>(d, P, arg);
        // step 0 of the sequence has no step into it: delta_0 stands, psi_0 = 0 (never followed; every byte read is defined)
        const bool act = i < n && !(head && i == 0);
        const double dn = col ? best + cur[u] : NEG_INF;
        d = act ? dn : d;
        if (valid && i < n) psi[(long)i * 16] = (uint8_t)(act ? arg : 0);
      }
    });
    static_for<0, VIT_AHEAD>([&](auto u) { cur[u] = nxt[u]; });
  }

  {
    double best = bcast<0>(d);
    int z = 0;
    static_for<1, K>([&](auto k) {
      const double v = bcast<k>(d);
      const bool w = v > best;
      best = w ? v : best;
      z = w ? (int)k : z;
    });
    if (valid && ch == a.C - 1 && c == 0) {
      if (a.score) a.score[b] = best;
      a.ends[q] = (uint8_t)z;                         // e_{C-1} = z_{T-1}
    }
  }

  // ---- chase: the back-pointers written above by OTHER lanes of this wavefront are read back below -------------------
  __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "agent");
  const uint4* prow = reinterpret_cast<const uint4*>(a.psi + (b * T + t0) * 16);
  uint8_t* cand = a.cand + (b * T + t0) * 16 + c;
  auto load_row = [&](int blk) -> uint4 {
    const int i = blk * 16 + c;
    return prow[i < n ? i : n - 1];
  };
  int z = c;                                          // lane k: the path that ends the chunk in state k
  int blk = (L - 1) >> 4;
  uint4 qv = load_row(blk);
  for (; blk >= 0; --blk) {
    const uint4 qn = load_row(blk > 0 ? blk - 1 : 0);
    const int ic = blk * 16 + c;
    // steps beyond the chunk: the identity map (z passes through)
    const unsigned long long map = ic < n ? vit_pack16(qv) : 0xFEDCBA9876543210ull;
    static_for<0, 16>([&](auto s) {
      constexpr int l = 15 - (int)s;
      const int i = blk * 16 + l;
      if (valid && i < n) cand[(long)i * 16] = (uint8_t)z;       // z = the candidate label of step t0 + i ...
      const unsigned long long m = vit_bcast_u64<l>(map);
      z = (int)((unsigned)(m >> (4 * z)) & 15u);                 // ... and psi of that step leads to the step before
    });
    qv = qn;
  }
  if (valid) a.fmap[q * 16 + c] = (uint8_t)z;         // f_c[k] (chunk 0: psi_0 = 0, not used)
}

// ---- stage 4: resolve the chunks' end states -------------------------------------------------------------------------------
__global__ __launch_bounds__(64) void hmm_vchunk_resolve_kernel(const ViterbiChunkedArgs a) {
  constexpr int D = 8;                                // rows of f requested ahead of the chain
  const long b = (long)blockIdx.x * 64 + threadIdx.x;
  if (b >= a.B) return;
  const int C = a.C;
  uint8_t* e = a.ends + b * C;
  const uint4* f = reinterpret_cast<const uint4*>(a.fmap + b * C * 16);
  auto row = [&](int ch) -> uint4 { return f[ch >= 1 ? ch : 1]; };
  int z = e[C - 1] & 15;
  uint4 ring[D];
  static_for<0, D>([&](auto u) { ring[u] = row(C - 1 - (int)u); });
  for (int ch0 = C - 1; ch0 >= 1; ch0 -= D) {
    static_for<0, D>([&](auto u) {
      const int ch = ch0 - (int)u;
      const uint4 r = ring[u];
      ring[u] = row(ch - D);
      if (ch >= 1) {
        z = (int)((unsigned)(vit_pack16(r) >> (4 * z)) & 15u);   // e_{c-1} = f_c[e_c]
        e[ch - 1] = (uint8_t)z;
      }
    });
  }
}

// ---- stage 5: gather -------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void hmm_vchunk_gather_kernel(const ViterbiChunkedArgs a) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= (long)a.B * a.T) return;
  const long b = i / a.T;
  const int t = (int)(i - b * a.T);
  const int e = a.ends[b * a.C + t / a.L] & 15;
  a.states[i] = a.cand[i * 16 + e];
}

template <int K>
static int launch_viterbi_chunked(const ViterbiChunkedArgs& a, hipStream_t s) {
  const long op_rows = (long)a.B * a.C * K, seq_rows = (long)a.B * a.C, steps = (long)a.B * a.T;
  hipLaunchKernelGGL((hmm_vchunk_ops_kernel<K>), dim3((unsigned)((op_rows + 3) / 4)), dim3(64), 0, s, a);
  hipLaunchKernelGGL((hmm_vchunk_scan_kernel<K>), dim3((unsigned)((a.B + 3) / 4)), dim3(64), 0, s, a);
  hipLaunchKernelGGL((hmm_vchunk_decode_kernel<K>), dim3((unsigned)((seq_rows + 3) / 4)), dim3(64), 0, s, a);
  hipLaunchKernelGGL(hmm_vchunk_resolve_kernel, dim3((unsigned)((a.B + 63) / 64)), dim3(64), 0, s, a);
  hipLaunchKernelGGL(hmm_vchunk_gather_kernel, dim3((unsigned)((steps + 255) / 256)), dim3(256), 0, s, a);
  return hipGetLastError() == hipSuccess ? 0 : -1000;
}

}  // namespace svae

// Stages 4 and 5 alone -- resolve and gather -- on R chains of T steps whose candidates, chunk maps and last end states
// (ends[r][C-1]) the caller has filled (hmm_sample_chunked.hip: R = B S).  Host only: the kernels are the ones above.
extern "C" int svae_hmm_vchunk_resolve_gather_launch(int R, int T, int L, int C, int32_t* states, uint8_t* cand,
                                                     uint8_t* fmap, uint8_t* ends, void* stream) {
  svae::ViterbiChunkedArgs a{};
  a.B = R; a.T = T; a.L = L; a.C = C;
  a.states = states; a.cand = cand; a.fmap = fmap; a.ends = ends;
  hipStream_t s = (hipStream_t)stream;
  const long steps = (long)R * T;
  hipLaunchKernelGGL(svae::hmm_vchunk_resolve_kernel, dim3((unsigned)((R + 63) / 64)), dim3(64), 0, s, a);
  hipLaunchKernelGGL(svae::hmm_vchunk_gather_kernel, dim3((unsigned)((steps + 255) / 256)), dim3(256), 0, s, a);
  return hipGetLastError() == hipSuccess ? 0 : -1000;
}

// The chunk the library picks, from tools/bench_hmm_viterbi_chunked.py on one MI355X (K = 8 and 16; DESIGN 4.5l has the
// table).  It started as the chunked E-step's rule (the stage structure is the same) and the measurement kept its core:
// the fastest chunk was 32 / 64 / 256 at T = 500 / 5000 / 50000 for both K up to 32 sequences (at 32 x 5000 chunk 128 was
// 2 - 4 % ahead of 64), i.e. the power of two nearest 1.2 sqrt(T); at 128 and 256 sequences the minimum sat one power of
// two higher (64 at T = 500, 128 at T = 5000; at 256 x 5000 and K = 8 chunk 256 was another 7 % ahead).  Chunked beat the
// serial call, by far more than the windows' spread (<= 4 %), at every measured shape with T >= 500 and B <= 256 --
// 1.2x - 4x at T = 500, 1.6x - 17x at T = 5000, 11x - 59x at T = 50000 -- and lost or tied at 512 x 500: batches above
// 256 sequences and sequences shorter than 500 steps (not measured) stay serial (return T).
extern "C" int svae_hmm_chunked_viterbi_default_chunk(int B, int T, int K) {
  if (B < 1 || T < 1 || K < 1 || K > svae::HMM_CHUNKED_MAX_K) return T;
  if (T < 500 || B > 256) return T;
  long L = 2;
  while (200 * L * L <= 144 * (long)T) L *= 2;          // 2^round(log2(1.2 sqrt(T)))
  if (B >= 128) L *= 2;
  return L < T ? (int)L : T;
}

extern "C" size_t svae_hmm_chunked_viterbi_workspace_bytes(int B, int T, int K, int chunk) {
  if (B <= 0 || T <= 0 || K <= 0 || K > svae::HMM_CHUNKED_MAX_K || chunk < 2) return 0;
  return (size_t)svae::hmm_chunked_viterbi_layout(B, T, K, chunk).total;
}

extern "C" int svae_hmm_chunked_viterbi_f64(int B, int T, int K, int pair_batched, int chunk,
                                            const double* init_params, const double* pair_params,
                                            const double* node_params, int32_t* states, double* score,
                                            void* workspace, size_t ws_bytes, void* stream) {
  // hmm_check_model's -1 .. -6 with this unit's bound on K in its place: -3 comes before -4 .. -6
  const int rc_model = svae::hmm_check_model(B, T, K, pair_batched, init_params, pair_params);
  if (rc_model <= -1 && rc_model >= -3) return rc_model;
  if (K > svae::HMM_CHUNKED_MAX_K) return -3;
  if (rc_model) return rc_model;
  if (B == 0) return 0;
  if (chunk < 2) return -7;
  if (!node_params) return -8;
  if (!states) return -9;
  if (!workspace) return -10;
  if (ws_bytes < svae_hmm_chunked_viterbi_workspace_bytes(B, T, K, chunk)) return -11;
  if (((uintptr_t)workspace & 15) != 0) return -12;   // back-pointer and map rows are read back 16 bytes at a time
  // one chunk holds the sequence: the serial decoder's launch on the head of the workspace (its back-pointers), nothing else
  if (chunk >= T)
    return svae_hmm_viterbi_f64(B, T, K, pair_batched, init_params, pair_params, node_params, states, score, workspace,
                                ws_bytes, stream);

  const svae::HmmChunkedViterbiLayout lay = svae::hmm_chunked_viterbi_layout(B, T, K, chunk);
  uint8_t* ws = (uint8_t*)workspace;
  svae::ViterbiChunkedArgs a;
  svae::hmm_set_model(a, B, T, K, pair_batched ? (long)K * K : 0, init_params, pair_params, node_params);
  a.L = chunk; a.C = (int)lay.C;
  a.states = states; a.score = score;
  a.psi = ws + lay.psi; a.cand = ws + lay.cand; a.fmap = ws + lay.fmap; a.ends = ws + lay.ends;
  a.ops = (double*)(ws + lay.ops); a.delta = (double*)(ws + lay.delta);
  return svae::hmm_dispatch_k(
      K, [&](auto k) { return svae::launch_viterbi_chunked<k>(a, (hipStream_t)stream); }, [&](auto) { return -3; });
}
