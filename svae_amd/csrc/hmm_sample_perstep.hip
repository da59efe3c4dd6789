// hmm_sample_perstep.hip -- HMM posterior sampling (forward filter, backward draw) with PER-STEP transition potentials for
// MI355X (gfx950), K <= 64: svae_hmm_perstep_sample_f64 (include/svae_hip.h).
//
// ONE ROUTE, log space throughout, as the per-step E-step (hmm_estep_perstep.hip): no range flags, no second filter launch.
//   filter   the E-step's forward sweep ITSELF: hmm_perstep_kernel<G, W, FILTER = true> (hmm_perstep_kernel.hpp) leaves the
//            unnormalised la_t, (B,T,K) doubles, in the workspace, stores logZ = logsumexp_k la_{L-1}[k] and returns.
//   draw     t = L-1:  lw[k] = la_{L-1}[k];   t < L-1:  lw[k] = la_t[k] + pair[t][k][z_{t+1}]
//            m = max_k lw[k] (0 if that is -inf),  w[k] = exp(lw[k] - m),  C[k] = w[0] + .. + w[k] in index order,
//            thr = clamp(u,0,1) C[K-1] (a NaN u counts as 0),  z_t = #{k : C[k] <= thr and C[k] < C[K-1]}
//            -- the selection rule of svae_hmm_sample_f64 word for word.
// The draw differs from the uniform one (hmm_sample_kernel.hpp) in what it can keep: the column pair[t][.][z_{t+1}] is new
// at every step and its address depends on the path, so it must not be a global load on the serial chain.
//   workgroup  one sequence, 4 wavefronts; a chain (one sample) is a group of G = 8, 16, 32 or 64 lanes (the E-step's
//              grouping), lane = state k: 256 / G samples per pass share every staged P_t; more samples take further
//              passes (grid y, then a loop).
//   staging    a block of NSB consecutive steps at a time (NSB = G for K <= 16, 4 for K <= 32, 1 above: what LDS holds):
//              all 256 threads copy the block's matrices (coalesced: the steps are contiguous in memory; 2 or 16 entries
//              each) and records into registers BEFORE the draws of the block above it and into LDS after them, between
//              two workgroup barriers: the loads are in flight during up to NSB draws, and the barriers are paid once per
//              block.  A tile keeps the E-step's odd row stride KS = K | 1: lane k reads [k][z] free of bank conflicts,
//              and that LDS read is the only z-dependent access of the chain.  Only the top block of a chain is clipped
//              to its length; a thread without an entry copies to one spare slot (no branch per entry); a wavefront
//              without a sample only stages.
//   u, labels  blocks of G steps: lane l of a chain holds u of step t0 + l (the next block's loaded a block ahead) and
//              keeps the label of that step: consecutive lanes load and store consecutive addresses.
//   C          the zero-padded LDS line of the uniform wide draw: lane k adds the G entries that end at its own, i.e.
//              zeros and then w[0], .., w[k] in that order.
// z is a count of at most K-1 lanes and is masked into range again before it addresses LDS.
// Lengths: L = lengths[b] clamped to [1,T] (the filter launch raises the status word); the draw starts at L-1, loads
// nothing at pair steps >= L-1 or u steps >= L, and stores -1 from L on.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "../../include/svae_hip.h"
#include "hmm_perstep_kernel.hpp"     // HmmPerstepArgs, the grouping and the kernel template: FILTER = true is instantiated here
#include "hmm_sample_kernel.hpp"      // smp_lds_sync, smp_clamp01 (no kernel of that header is instantiated here)

namespace svae {

struct PerstepDrawArgs {
  int B, T, K, S;
  long pair_stride;                        // doubles between sequences' (T-1,K,K) blocks (0 = shared)
  const double* __restrict__ pair_params;  // (T-1,K,K) or (B,T-1,K,K)
  const int32_t* __restrict__ lengths;     // (B) or nullptr
  const double* __restrict__ u;            // (B,S,T)
  int32_t* __restrict__ states;            // (B,S,T)
  const double* __restrict__ la;           // (B,T,K) the filter's records
};

constexpr int PSD_WAVES = 4;
// steps staged per block: all G of a label block where that fits in LDS beside the line (K <= 16), 4 at K <= 32, 1 above
constexpr int perstep_draw_block(int G) { return G <= 16 ? G : G == 32 ? 4 : 1; }
// the tiles and records of a block, the wavefronts' lines, and one slot for the stores of threads without an entry
constexpr int perstep_draw_lds_doubles(int K, int G) { return perstep_draw_block(G) * (K * (K | 1) + K) + PSD_WAVES * 128 + 1; }

template <int G>
__global__ __launch_bounds__(64 * PSD_WAVES) void hmm_perstep_draw_kernel(const PerstepDrawArgs a) {
  constexpr int NT = 64 * PSD_WAVES;
  constexpr int CPW = 64 / G;                    // chains per wavefront
  constexpr int CPB = PSD_WAVES * CPW;           // ... per pass of the workgroup
  constexpr int NSB = perstep_draw_block(G);
  constexpr int NE = NSB * G * G > NT ? NSB * G * G / NT : 1;   // entries of a block of matrices a thread stages: 2 or 16
  extern __shared__ double smem[];
  const int K = a.K, T = a.T, S = a.S, KS = K | 1, TS = K * KS;
  const int tid = threadIdx.x, wv = tid >> 6, tl = tid & 63;
  const int lane = tl & (G - 1), grp = tl / G;
  const long b = blockIdx.x;
  const bool live = lane < K;
  const int lk = live ? lane : 0;
  double* tile = smem;                           // [NSB][K][KS] P_t of the block's steps
  double* lav = tile + NSB * TS;                 // [NSB][K] la_t
  double* line = lav + NSB * K + wv * 128 + grp * 2 * G;   // [2 G] G zeros, then this chain's weights
  const double NINF = -__builtin_inf();

  int L = T;
  if (a.lengths) L = min(max(a.lengths[b], 1), T);

  const int KK = K * K;
  const double* pair = a.pair_params + b * a.pair_stride;
  const double* la = a.la + b * T * K;
  const int NONE = NSB * (TS + K) + PSD_WAVES * 128;   // the spare slot: no branch per entry in the copies
  int off[NE], est[NE];                          // this thread's entries of a block: tile offsets (NONE: none), step in the block
#pragma unroll
  for (int i = 0; i < NE; ++i) {
    const int e = tid + NT * i;
    const int s = e / KK, r = e - s * KK;
    const int j = r / K;
    off[i] = e < NSB * KK ? s * TS + j * KS + (r - j * K) : NONE;
    est[i] = s;
  }
  const int las = tid / K;                       // the step in the block of this thread's entry of la (tid < NSB K)
  line[lane] = 0.0;
  const unsigned long long gmask = G == 64 ? ~0ull : ((1ull << (G & 63)) - 1ull);
  const int gsh = grp * G;

  // the matrices and records of block `blk` (steps blk NSB ..).  Only the top block of a chain can reach past its length:
  // TOP clips it (nothing at pair steps >= L-1 or record steps >= L is loaded); every block below it is whole
  double pr[NE], lar;
  auto load_block = [&](int blk, auto top) {
    constexpr bool TOP = decltype(top)::value;
    const int tb0 = blk * NSB;
    const double* P = pair + (long)tb0 * KK;
    if constexpr (TOP) {
#pragma unroll
      for (int e = 0; e < NE; ++e) pr[e] = (off[e] != NONE && tb0 + est[e] < L - 1) ? P[tid + NT * e] : 0.0;
      lar = (tid < NSB * K && tb0 + las < L) ? la[(long)tb0 * K + tid] : 0.0;
    } else {                                     // no branch per entry: a thread without an entry loads the block's first
#pragma unroll
      for (int e = 0; e < NE; ++e) pr[e] = P[off[e] != NONE ? tid + NT * e : 0];
      lar = la[(long)tb0 * K + (tid < NSB * K ? tid : 0)];
    }
  };
  auto store_block = [&]() {
#pragma unroll
    for (int e = 0; e < NE; ++e) tile[off[e]] = pr[e];
    lav[tid < NSB * K ? tid : NONE - NSB * TS] = lar;
  };

  const long NCH = ((long)S + CPB - 1) / CPB;
  for (long ch = blockIdx.y; ch < NCH; ch += gridDim.y) {
    const long sr = ch * CPB + wv * CPW + grp;
    const bool cvalid = sr < S;                  // an idle chain shadows the last sample and stores nothing
    const bool wact = ch * CPB + wv * CPW < S;   // a wavefront without a chain only stages: it leaves the SIMD to the others
    const long r = b * S + (cvalid ? sr : S - 1);
    const double* ur = a.u + r * T;
    int32_t* out = a.states + r * T;

    int blk = (L - 1) / NSB;
    load_block(blk, std::true_type{});
    __syncthreads();                             // (the pass before has left the tile)
    store_block();
    __syncthreads();
    auto load_u = [&](int ub) -> double { return ur[min((ub > 0 ? ub : 0) * G + lane, L - 1)]; };
    double uv = 0.0, uvn = 0.0;
    if (wact) {
      uv = load_u((L - 1) / G);
      uvn = load_u((L - 1) / G - 1);
    }
    int z = 0, lab = 0;
    for (; blk >= 0; --blk) {                    // (workgroup-uniform: one sequence)
      const int tb0 = blk * NSB;
      if (blk > 0) load_block(blk - 1, std::false_type{});   // the next block: in flight during this block's draws
      for (int t = wact ? min(tb0 + NSB, L) - 1 : tb0 - 1; t >= tb0; --t) {
        const int i = t & (G - 1);
        const double* tl_t = tile + (t - tb0) * TS;
        const bool last = t == L - 1;
        const int zc = min(z, K - 1);            // (z counts at most K-1 lanes; masked again before it addresses LDS)
        const double lat = lav[(t - tb0) * K + lk], pz = tl_t[lk * KS + zc];
        const double lw = live ? (last ? lat : lat + pz) : NINF;
        double m = lw;
#pragma unroll
        for (int o = G / 2; o > 0; o >>= 1) m = __builtin_fmax(m, __shfl_xor(m, o));
        const double ms = m == NINF ? 0.0 : m;
        const double w = live ? exp(lw - ms) : 0.0;
        __builtin_amdgcn_wave_barrier();
        line[G + lane] = w;
        smp_lds_sync();
        double C = 0.0;
#pragma unroll
        for (int q = 0; q < G; ++q) C += line[lane + 1 + q];
        const double tot = __shfl(C, K - 1, G);
        const double thr = smp_clamp01(__shfl(uv, i, G)) * tot;
        const unsigned long long bm = __ballot(live && C <= thr && C < tot);
        z = __popcll((bm >> gsh) & gmask);
        lab = lane == i ? z : lab;
        if (i == 0) {                            // the label block leaves; the next block's uniforms arrive
          if (cvalid && t + lane < L) out[t + lane] = lab;
          uv = uvn;
          uvn = load_u(t / G - 2);
        }
      }
      __syncthreads();
      if (blk > 0) store_block();
      __syncthreads();
    }
    if (cvalid)
      for (int t = L + lane; t < T; t += G) out[t] = -1;
  }
}

template <int G, int W>
static void launch_perstep_filter(const HmmPerstepArgs& a, hipStream_t s) {
  constexpr int SPB = 64 / G;
  const size_t lds = (size_t)SPB * hmm_perstep_lds_doubles(a.K, W) * sizeof(double);
  hipLaunchKernelGGL((hmm_perstep_kernel<G, W, true>), dim3((unsigned)((a.B + SPB - 1) / SPB)), dim3(64 * W), lds, s, a);
}

template <int G>
static void launch_perstep_draw(const PerstepDrawArgs& a, hipStream_t s) {
  constexpr int CPB = PSD_WAVES * (64 / G);
  const long nch = ((long)a.S + CPB - 1) / CPB;
  const size_t lds = (size_t)perstep_draw_lds_doubles(a.K, G) * sizeof(double);
  hipLaunchKernelGGL((hmm_perstep_draw_kernel<G>), dim3((unsigned)a.B, (unsigned)(nch < 65535 ? nch : 65535)),
                     dim3(64 * PSD_WAVES), lds, s, a);
}

}  // namespace svae

extern "C" int svae_hmm_perstep_sample_f64(int B, int T, int K, int S, int pair_batched,
                                           const double* init_params, const double* pair_params,
                                           const double* node_params, const int32_t* lengths, const double* u,
                                           int32_t* states, double* logZ,
                                           int32_t* info, void* workspace, size_t ws_bytes, void* stream) {
  if (const int rc = svae::hmm_check_model(B, T, K, pair_batched, init_params, pair_params, true)) return rc;
  if (B == 0) return 0;
  if (!node_params) return -7;
  if (S < 1) return -8;
  if (!u) return -9;
  if (!states) return -10;
  if (lengths && !info) return -11;
  if (!workspace) return -12;
  if (ws_bytes < svae_hmm_perstep_workspace_bytes(B, T, K)) return -13;
  if (((uintptr_t)workspace & 15) != 0) return -14;
  const long stride = pair_batched ? (long)(T - 1) * K * K : 0;
  svae::HmmPerstepArgs f;
  svae::hmm_set_model(f, B, T, K, stride, init_params, pair_params, node_params);
  f.lengths = lengths;
  f.logZ = logZ; f.E_init = nullptr; f.E_trans = nullptr; f.E_states = nullptr; f.info = info;
  f.ws = (double*)workspace;
  svae::PerstepDrawArgs d;
  d.B = B; d.T = T; d.K = K; d.S = S; d.pair_stride = stride;
  d.pair_params = pair_params; d.lengths = lengths; d.u = u; d.states = states; d.la = (const double*)workspace;
  hipStream_t s = (hipStream_t)stream;
  svae::hmm_dispatch_group(K, [&](auto g, auto w) {
    svae::launch_perstep_filter<g, w>(f, s);
    svae::launch_perstep_draw<g>(d, s);
  });
  return hipGetLastError() == hipSuccess ? 0 : -1000;
}
