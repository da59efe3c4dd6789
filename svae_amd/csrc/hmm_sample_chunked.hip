// hmm_sample_chunked.hip -- HMM posterior sampling PARTITIONED IN TIME, for long sequences (K <= 16), gfx950.
//
// The serial sampler (hmm_sample.hip) runs a forward filter of T dependent steps and a backward draw of T dependent steps
// per chain, whatever the batch.  Here the T steps are cut into C = ceil(T / L) chunks of L steps (the last may be as
// short as one).  With the uniforms fixed, the backward draw at step t is a MAP from z_{t+1} to z_t -- like a Viterbi
// back-pointer --, so the chain becomes five short ones and two flat passes:
//   stage 1, 2  the chunk operators and the forward boundary scan of the chunked E-step in its log-Z-only form: the
//            kernels of hmm_estep_chunked.hip, through its host launcher svae_hmm_chunked_forward_launch.  They give the
//            filtered message a^_c at every chunk's last step, log Z and the range flags.            depth L, C
//   stage 3  hmm_smpc_filter_kernel   parallel over (sequence, chunk): hmm_filter_row_kernel's scaled step on the chunk's
//            own steps, entered with a^_{c-1} in place of the initial message (chunk 0: `init`); stores the serial
//            sampler's records a_t, 16 doubles per step, padding lanes 0, with the same range test per step.   depth L
//            hmm_smpc_mark_kernel writes -1 into the live lanes of a flagged sequence's step-0 record; the log-space
//            filter launch of hmm_sample_log.hip then replaces all of that sequence's records and its log Z.
//   stage 4  hmm_smpc_maps_kernel     flat over (sequence, sample, step), no dependent chain: psi_t[k] = the state drawn at
//            t-1 given z_t = k, for all k, from record a_{t-1}, column k of the matrix and u[b,s,t-1]; z_{T-1} from
//            a_{T-1} and u[b,s,T-1].  Weights and selection are svae_hmm_sample_f64's (include/svae_hip.h): rounded
//            products a[j] exp(pair[j][k] - M), summed in index order, thr = clamp(u) C[K-1], z = #{j : C[j] <= thr and
//            C[j] < C[K-1]}; a total below 1e-200, and every step of a sequence whose record is log a_t, in log space.
//            Lane k is the conditioning state: column k in K registers, a[j] by row_newbcast.  One byte per state.
//   stage 5  hmm_smpc_chase_kernel    parallel over (chain, chunk): from all K end states at once, down the chunk's maps,
//            16 steps at a time, each step's 16 bytes packed into a word of nibbles (vit_pack16): candidate labels
//            cand[t][k] and f_c[k], the end state of chunk c-1 the path arrives at.                              depth L
//   stage 6, 7  resolve (e_{C-1} = z_{T-1}, e_{c-1} = f_c[e_c]) and gather (states[b,s,t] = cand[t][e_{c(t)}]): the
//            kernels of hmm_viterbi_chunked.hip on B S chains, through svae_hmm_vchunk_resolve_gather_launch.  depth C
// One uniform serves all K conditioning states of a step: a valid coupling, and only the entry on the realised path reaches
// the output -- the labels are those of svae_hmm_sample_f64's draw run on the same records.
// Every data-dependent index is a count below K or a nibble, masked before it addresses memory: NaN potentials give
// unspecified labels in 0..K-1, no fault, and touch no other sequence.  No atomics, no allocation, no host read-back.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/svae_hip.h"

#include "dpp.hpp"
#include "hmm_units.hpp"
#include "hmm_sample_kernel.hpp"          // SampleArgs, smp_row_max16, smp_clamp01, the log-space launch (no kernel of it
                                          // is instantiated here)
#include "hmm_viterbi_kernel.hpp"         // vit_pack16, vit_bcast_u64 (likewise)

// hmm_estep_chunked.hip: stages 1 and 2 (chunk operators, forward boundary scan) on a caller's buffers
extern "C" int svae_hmm_chunked_forward_launch(int B, int T, int K, int L, int C, long pair_stride,
                                               const double* init_params, const double* pair_params,
                                               const double* node_params, double* logZ, int32_t* route, double* ops,
                                               double* scale, double* ahat, void* stream);
// hmm_viterbi_chunked.hip: resolve and gather on R chains of T steps
extern "C" int svae_hmm_vchunk_resolve_gather_launch(int R, int T, int L, int C, int32_t* states, uint8_t* cand,
                                                     uint8_t* fmap, uint8_t* ends, void* stream);

namespace svae {

struct SampleChunkedArgs {
  int B, T, K, S, L, C;                   // L = steps per chunk (2 <= L < T), C = ceil(T / L) >= 2
  long pair_stride;
  const double* __restrict__ init_params;
  const double* __restrict__ pair_params;
  const double* __restrict__ node_params;
  const double* __restrict__ u;           // (B,S,T)
  int32_t* __restrict__ route;            // (B) route words, zeroed before stage 1
  double* rec;                            // (B,T,16) a_t (a flagged sequence: log a_t)
  const double* __restrict__ ahat;        // (B,C,K)
  uint8_t* psi;                           // (B S,T,16) state maps
  uint8_t* cand;                          // (B S,T,16) candidate labels
  uint8_t* fmap;                          // (B S,C,16)
  uint8_t* ends;                          // (B S,C)
};

// ---- stage 3: the filter of every chunk ------------------------------------------------------------------------------------
// Trip count L for every row of the wavefront; a row of the short last chunk runs its tail on its last step's data under
// selects and keeps nothing of it.
template <int K>
__global__ __launch_bounds__(64) void hmm_smpc_filter_kernel(const SampleChunkedArgs a) {
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
  const int n = T - t0 < L ? T - t0 : L;              // this chunk's steps (>= 1)
  const bool head = ch == 0;

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

  const double* node = a.node_params + (b * T + t0) * K + cc;
  double* rec = a.rec + (b * T + t0) * 16 + c;
  const double init = a.init_params[cc];
  const double aprev_ld = a.ahat[(head ? q : q - 1) * K + cc];               // (index inside the array for chunk 0 too)
  double alpha = (col && !head) ? aprev_ld : 0.0;                            // a^_{c-1}
  double one = 1.0;
  bool bad = false;

  auto step = [&](int i, double ndraw) __attribute__((always_inline)) {
    const bool live = i < n;
    const bool first = head && i == 0;
    const double nd = col ? ndraw + (first ? init : 0.0) : NEG_INF;
    const double m = smp_row_max16(nd);
    const double e = col ? exp_nonpos(nd - m) : 0.0;
    // (no branch on `first`: it differs between the rows of a wavefront; chunk 0's alpha starts at 0)
    double pred = (first && col) ? 1.0 : 0.0;
    dpp_fence(alpha);
    static_for<0, K>([&](auto j) { mac_bc<j>(pred, alpha, P[j]); });         // sum_j a_{t-1}[j] P[j][k]
    double al = pred * e;                                                    // the unnormalised message component
    double cs = 0.0;
    dpp_fence(al);
    static_for<0, K>([&](auto k) { mac_bc<k>(cs, al, one); });
    const double rc = rcp_nr(cs);
    // the range criterion of hmm_filter_row_kernel (a NaN fails both compares); steps past the chunk never flag
    bad = bad || (live && ((col && !(al >= HMM_LOW)) || !(cs > SMP_TINY)));
    alpha = live ? al * rc : alpha;
    if (valid && live) rec[(long)i * 16] = alpha;
  };
  auto load = [&](int i) -> double { return node[(long)(i < n ? i : n - 1) * K]; };
  double cur[SMP_AHEAD], nxt[SMP_AHEAD];
  static_for<0, SMP_AHEAD>([&](auto v) { cur[v] = load(v); });
  for (int i0 = 0; i0 < L; i0 += SMP_AHEAD) {
    static_for<0, SMP_AHEAD>([&](auto v) { nxt[v] = load(i0 + SMP_AHEAD + v); });
    static_for<0, SMP_AHEAD>([&](auto v) {
      const int i = i0 + v;
      if (i < L) step(i, cur[v]);                     // (wave-uniform)
    });
    static_for<0, SMP_AHEAD>([&](auto v) { cur[v] = nxt[v]; });
  }
  // (`bad` is per lane: the row's sixteen bits of the ballot; every writer of a route word writes the same 1)
  if (((__ballot(bad) >> (lane & 48)) & 0xffffull) != 0 && valid && c == 0) a.route[b] = 1;
}

// a flagged sequence's step-0 record: -1 in every live lane, where the log-space launch looks for it
__global__ __launch_bounds__(256) void hmm_smpc_mark_kernel(const SampleChunkedArgs a) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  const long b = i >> 4;
  const int c = (int)(i & 15);
  if (b >= a.B || c >= a.K) return;
  if (a.route[b] != 0) a.rec[b * a.T * 16 + c] = -1.0;
}

// ---- stage 4: state maps ---------------------------------------------------------------------------------------------------
// row = (chain r = b S + s, block of 16 steps): step t of the block draws from record a_t with u[r][t] -- for t < T-1 the
// map psi_{t+1} (lane k: given z_{t+1} = k), for t = T-1 the chain's last state (every lane the same; lane 0 stores it as
// e_{C-1}).  The block amortises the K exponentials of the matrix column.
template <int K>
__global__ __launch_bounds__(64) void hmm_smpc_maps_kernel(const SampleChunkedArgs a) {
  const int lane = threadIdx.x;
  const int c = lane & 15;
  const int T = a.T;
  const long NB = ((long)T + 15) >> 4;
  const long rows = (long)a.B * a.S * NB;
  const long r0 = (long)blockIdx.x * 4 + (lane >> 4);
  const bool valid = r0 < rows;                       // idle rows repeat the last block and store nothing
  const long row = valid ? r0 : rows - 1;
  const int blk = (int)(row % NB);
  const long r = row / NB;
  const long b = r / a.S;
  const bool col = c < K;
  const int cc = col ? c : 0;
  const double NEG_INF = -__builtin_inf();
  const int rsh = lane & 48;

  const double* pp = a.pair_params + b * a.pair_stride;
  double E[K];                                        // E[j] = exp(pair[j][c] - M): column c
  double pmax = NEG_INF;
  static_for<0, K>([&](auto j) {
    const double v = pp[j * K + cc];
    E[j] = col ? v : NEG_INF;
    pmax = __builtin_fmax(pmax, E[j]);
  });
  pmax = smp_row_max16(pmax);
  static_for<0, K>([&](auto j) { E[j] = col ? exp(E[j] - pmax) : 0.0; });

  const double* af = a.rec + (b * T) * 16 + c;
  // the kind of this sequence's records, as the serial draw tells it: a scaled a_{T-1} has a positive entry, log a_t none
  const bool islog = ((unsigned)(__ballot(col && af[(long)(T - 1) * 16] > 0.0) >> rsh) & 0xffffu) == 0;
  auto load_a = [&](int i) -> double {
    const int t = blk * 16 + i;
    return af[(long)(t < T ? t : T - 1) * 16];
  };
  const double uv = a.u[r * T + (blk * 16 + c < T ? blk * 16 + c : T - 1)];
  uint8_t* psi = a.psi + (r * T) * 16 + c;
  if (valid && blk == 0) psi[0] = 0;                  // psi_0 is never followed; every byte read later is defined

  double av_n = load_a(0);
#pragma unroll 1
  for (int i = 0; i < 16; ++i) {
#pragma clang fp contract(off)
    const int t = blk * 16 + i;
    const bool last = t >= T - 1;                     // the chain's last step: the weights are a_t alone
    const double av = av_n;
    av_n = load_a(i + 1);                             // next step's record, unconditionally (clamped)
    const double uc = smp_clamp01(__shfl(uv, i, 16));
    // w[j] = a[j] E[j] is a rounded product, C their sum in index order: one pass for the total, one for the count
    double w[K];
    double tot = 0.0;
    static_for<0, K>([&](auto j) {
      w[j] = __dmul_rn(bcast<j>(av), last ? 1.0 : E[j]);
      tot = __dadd_rn(tot, w[j]);
    });
    const double thr = uc * tot;
    double C = 0.0;
    int cnt = 0;
    static_for<0, K>([&](auto j) {
      C = __dadd_rn(C, w[j]);
      cnt += (C <= thr && C < tot) ? 1 : 0;
    });
    const bool under = col && !(tot >= SMP_TINY);
    if (__any(under)) {
      // the weights of this draw in log space (wave-uniform branch; every step of a sequence whose record is log a_t,
      // else rare); the matrix column is read again
      const double la = islog ? av : (av > 0.0 ? ::log(av) : NEG_INF);
      double mx = NEG_INF;
      static_for<0, K>([&](auto j) {
        w[j] = bcast<j>(la) + (last ? 0.0 : pp[j * K + cc]);
        mx = __builtin_fmax(mx, w[j]);
      });
      double tot2 = 0.0;
      static_for<0, K>([&](auto j) {
        w[j] = mx > NEG_INF ? exp(w[j] - mx) : 0.0;
        tot2 = __dadd_rn(tot2, w[j]);
      });
      const double thr2 = uc * tot2;
      double C2 = 0.0;
      int cnt2 = 0;
      static_for<0, K>([&](auto j) {
        C2 = __dadd_rn(C2, w[j]);
        cnt2 += (C2 <= thr2 && C2 < tot2) ? 1 : 0;
      });
      cnt = under ? cnt2 : cnt;
    }
    // (cnt <= K - 1: the entry that reaches the total is never counted; a NaN counts nothing)
    if (valid && t < T - 1) psi[(long)(t + 1) * 16] = (uint8_t)cnt;
    if (valid && t == T - 1 && c == 0) a.ends[r * a.C + (a.C - 1)] = (uint8_t)cnt;       // e_{C-1} = z_{T-1}
  }
}

// ---- stage 5: the chase inside every chunk ---------------------------------------------------------------------------------
// hmm_vchunk_decode_kernel's second half on the maps of stage 4: lane k starts at end state k of the chunk.
__global__ __launch_bounds__(64) void hmm_smpc_chase_kernel(const SampleChunkedArgs a) {
  const int lane = threadIdx.x;
  const int c = lane & 15;
  const long rows = (long)a.B * a.S * a.C;
  const long q0 = (long)blockIdx.x * 4 + (lane >> 4);
  const bool valid = q0 < rows;                       // idle rows repeat the last chunk and store nothing
  const long q = valid ? q0 : rows - 1;
  const int ch = (int)(q % a.C);
  const long r = q / a.C;
  const int L = a.L, T = a.T;
  const int t0 = ch * L;
  const int n = T - t0 < L ? T - t0 : L;

  const uint4* prow = reinterpret_cast<const uint4*>(a.psi + (r * T + t0) * 16);
  uint8_t* cand = a.cand + (r * T + t0) * 16 + c;
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
      z = (int)((unsigned)(m >> (4 * z)) & 15u);                 // ... and that step's map leads to the step before
    });
    qv = qn;
  }
  if (valid) a.fmap[q * 16 + c] = (uint8_t)z;         // f_c[k] (chunk 0: psi_0 = 0, not used)
}

template <int K>
static int launch_sample_chunked(const SampleChunkedArgs& a, const SampleArgs& lg, hipStream_t s) {
  const long seq_rows = (long)a.B * a.C, R = (long)a.B * a.S;
  const long map_rows = R * (((long)a.T + 15) >> 4), chase_rows = R * a.C;
  hipLaunchKernelGGL((hmm_smpc_filter_kernel<K>), dim3((unsigned)((seq_rows + 3) / 4)), dim3(64), 0, s, a);
  hipLaunchKernelGGL(hmm_smpc_mark_kernel, dim3((unsigned)(((long)a.B * 16 + 255) / 256)), dim3(256), 0, s, a);
  if (hipGetLastError() != hipSuccess) return -1000;
  if (const int rc = svae_hmm_sample_log_launch(&lg, s)) return rc;
  hipLaunchKernelGGL((hmm_smpc_maps_kernel<K>), dim3((unsigned)((map_rows + 3) / 4)), dim3(64), 0, s, a);
  hipLaunchKernelGGL(hmm_smpc_chase_kernel, dim3((unsigned)((chase_rows + 3) / 4)), dim3(64), 0, s, a);
  return hipGetLastError() == hipSuccess ? 0 : -1000;
}

}  // namespace svae

// The chunk the library picks, from tools/bench_hmm_sample_chunked.py on one MI355X (K = 8 and 16, S = 1 and 8; DESIGN
// 4.5m has the table).  It started as the chunked E-step's rule applied to B (the front end is that unit's) and the
// measurement kept it: chunked beat the serial call, by far more than the windows' spread (<= 5.4 %), at every measured
// shape with T >= 500 and B <= 128 -- 1.9x - 5x at T = 500, 2.7x - 25x at T = 5000, 10x - 93x at T = 50000 --, the pick
// within 3.2 % of the best measured chunk; at 512 x 500 it lost at K = 16 (and won at K = 8, S = 1): batches above 128
// sequences and sequences shorter than 500 steps (not measured) stay serial (return T).
extern "C" int svae_hmm_chunked_sample_default_chunk(int B, int T, int K, int S) {
  if (B < 1 || T < 1 || K < 1 || K > svae::HMM_CHUNKED_MAX_K || S < 1) return T;
  if ((long)B * S * T >= (1l << 31)) return T;
  if (T < 500 || B > 128) return T;
  long L = 2;
  while (200 * L * L <= 144 * (long)T) L *= 2;          // 2^round(log2(1.2 sqrt(T)))
  return L < T ? (int)L : T;
}

extern "C" size_t svae_hmm_chunked_sample_workspace_bytes(int B, int T, int K, int S, int chunk) {
  if (B <= 0 || T <= 0 || K <= 0 || K > svae::HMM_CHUNKED_MAX_K || S <= 0 || chunk < 2) return 0;
  return (size_t)svae::hmm_chunked_sample_layout(B, T, K, S, chunk).total;
}

extern "C" int svae_hmm_chunked_sample_f64(int B, int T, int K, int S, int pair_batched, int chunk,
                                           const double* init_params, const double* pair_params,
                                           const double* node_params, const double* u,
                                           int32_t* states, double* logZ,
                                           void* workspace, size_t ws_bytes, void* stream) {
  // hmm_check_model's -1 .. -6 with this unit's bound on K in its place: -3 comes before -4 .. -6
  const int rc_model = svae::hmm_check_model(B, T, K, pair_batched, init_params, pair_params);
  if (rc_model <= -1 && rc_model >= -3) return rc_model;
  if (K > svae::HMM_CHUNKED_MAX_K) return -3;
  if (rc_model) return rc_model;
  if (B == 0) return 0;
  if (chunk < 2) return -7;
  if (!node_params) return -8;
  if (S < 1) return -9;
  if ((long)B * S * T >= (1l << 31)) return -10;
  if (!u) return -11;
  if (!states) return -12;
  if (!workspace) return -13;
  if (ws_bytes < svae_hmm_chunked_sample_workspace_bytes(B, T, K, S, chunk)) return -14;
  if (((uintptr_t)workspace & 15) != 0) return -15;   // map rows are read back 16 bytes at a time
  // one chunk holds the sequence: the serial sampler's launches on the head of the workspace (its records), nothing else
  if (chunk >= T)
    return svae_hmm_sample_f64(B, T, K, S, pair_batched, init_params, pair_params, node_params, u, states, logZ,
                               workspace, ws_bytes, stream);

  const svae::HmmChunkedSampleLayout lay = svae::hmm_chunked_sample_layout(B, T, K, S, chunk);
  uint8_t* ws = (uint8_t*)workspace;
  hipStream_t s = (hipStream_t)stream;
  const long pair_stride = pair_batched ? (long)K * K : 0;
  double* lz = logZ ? logZ : (double*)(ws + lay.lz);
  svae::SampleChunkedArgs a;
  svae::hmm_set_model(a, B, T, K, pair_stride, init_params, pair_params, node_params);
  a.S = S; a.L = chunk; a.C = (int)lay.C;
  a.u = u;
  a.route = (int32_t*)(ws + lay.route);
  a.rec = (double*)(ws + lay.rec);
  a.ahat = (double*)(ws + lay.ahat);
  a.psi = ws + lay.maps; a.cand = ws + lay.cand; a.fmap = ws + lay.fmap; a.ends = ws + lay.ends;
  // the log-space launch works on the serial sampler's arguments
  svae::SampleArgs lg;
  svae::hmm_set_model(lg, B, T, K, pair_stride, init_params, pair_params, node_params);
  lg.S = S; lg.u = u; lg.states = states; lg.logZ = lz; lg.ws = a.rec;

  if (hipMemsetAsync(a.route, 0, sizeof(int32_t) * (size_t)B, s) != hipSuccess) return -1000;
  if (const int rc = svae_hmm_chunked_forward_launch(B, T, K, a.L, a.C, pair_stride, init_params, pair_params, node_params,
                                                     lz, a.route, (double*)(ws + lay.ops), (double*)(ws + lay.scale),
                                                     (double*)(ws + lay.ahat), stream))
    return rc;
  if (const int rc = svae::hmm_dispatch_k(
          K, [&](auto k) { return svae::launch_sample_chunked<k>(a, lg, s); }, [&](auto) { return -3; }))
    return rc;
  return svae_hmm_vchunk_resolve_gather_launch(B * S, T, a.L, a.C, states, a.cand, a.fmap, a.ends, stream);
}
