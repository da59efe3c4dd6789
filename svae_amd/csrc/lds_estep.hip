// lds_estep.hip -- host side of the register-path LDS C ABI (include/svae_hip.h, 1 <= n <= 15): argument checks, kernel
// selection and workspace layout of the uniform entry points (E-step, filter, sampler, fused inference, SLDS mean-field
// step, VJPs) and of the per-sequence-length ones (svae_lds_ragged_*).  Every launch goes through the per-n unit tables
// (lds_units.hpp; defined by lds_estep_n.hip and lds_vjp_n.hip); svae_lds_estep_f64 hands 16 <= n <= 64 to the tiled
// path (lds_estep_tile.hip).  Device code here: the deterministic batch reduction of the global statistics and the
// one-workgroup table / count kernels of the ragged entry points.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdlib.h>

#include "../../include/svae_hip.h"
#include "lds_units.hpp"
#include "per_device.hpp"

// the per-n units: units[n] for 1 <= n <= SVAE_LDS_MAX_N (every entry point checks n before it looks one up)
#define SVAE_DECL(NN) extern "C" const svae::EstepUnit svae_lds_estep_unit_n##NN; \
                      extern "C" const svae::VjpUnit svae_lds_vjp_unit_n##NN;
SVAE_LDS_NS(SVAE_DECL)
#undef SVAE_DECL
#define SVAE_ESTEP(NN) &svae_lds_estep_unit_n##NN,
#define SVAE_VJP(NN) &svae_lds_vjp_unit_n##NN,
static const svae::EstepUnit* const estep_units[SVAE_LDS_MAX_N + 1] = {nullptr, SVAE_LDS_NS(SVAE_ESTEP)};
static const svae::VjpUnit* const vjp_units[SVAE_LDS_MAX_N + 1] = {nullptr, SVAE_LDS_NS(SVAE_VJP)};
#undef SVAE_ESTEP
#undef SVAE_VJP

extern "C" {
/* 16 <= n <= SVAE_LDS_TILE_MAX_N: LDS-tiled MFMA path (lds_estep_tile.hip) */
int svae_lds_launch_tile(const svae::LdsArgs*, int n, int inhomog, void* stream);
size_t svae_lds_tile_step_doubles(int n);
size_t svae_lds_tile_packed_doubles(int B, int T, int n, int inhomog, int pair_batched);
}

namespace svae {

// ---- deterministic batch reduction of the global statistics ------------------------------------
// out = [sum_b E_init (n^2+n) | sum_b E_pair (3 n^2) | sum_b lognorm | B].  Fixed summation order => bit-reproducible.
// A workgroup takes 8 consecutive statistics: thread (jj, ch) = (tid & 7, tid >> 3) sums the sequences b = ch, ch + 32,
// ... of statistic j0 + jj in four interleaved partial sums, sixteen requests in flight (the 8 lanes of a chunk read one
// 64-byte sector of a sequence's block: the first version read one statistic with a stride of n^2 + n doubles across
// the lanes -- every lane its own sector, 13 MB of traffic for 1.7 MB of data at 512 sequences), then the 32 chunks
// meet in LDS.
__global__ __launch_bounds__(256) void lds_reduce_stats_kernel(int B, int n, const double* __restrict__ E_init,
                                                               const double* __restrict__ E_pair,
                                                               const double* __restrict__ lognorm, double* out) {
  const int ni = n * n + n, np = 3 * n * n, tot = ni + np + 1;
  __shared__ double red[256], red2[64];
  const int jj = threadIdx.x & 7, ch = threadIdx.x >> 3;
  const int j = blockIdx.x * 8 + jj;
  const double* src;
  long stride;
  if (j < ni) { src = E_init + j; stride = ni; }
  else if (j < ni + np) { src = E_pair + (j - ni); stride = np; }
  else { src = lognorm; stride = 1; }
  double acc[4] = {0.0, 0.0, 0.0, 0.0};
  if (j < tot) {
    int b = ch;
    for (; b + 31 * 32 < B; b += 32 * 32) {       // (large batches: 32 requests in flight)
      double v[32];
#pragma unroll
      for (int u = 0; u < 32; ++u) v[u] = src[(long)(b + 32 * u) * stride];
#pragma unroll
      for (int u = 0; u < 32; ++u) acc[u & 3] += v[u];
    }
    for (; b + 15 * 32 < B; b += 16 * 32) {
      double v[16];
#pragma unroll
      for (int u = 0; u < 16; ++u) v[u] = src[(long)(b + 32 * u) * stride];
#pragma unroll
      for (int u = 0; u < 16; ++u) acc[u & 3] += v[u];
    }
    for (int u = 0; b < B; b += 32, ++u) acc[u & 3] += src[(long)b * stride];
  }
  red[threadIdx.x] = (acc[0] + acc[1]) + (acc[2] + acc[3]);
  __syncthreads();
  if (threadIdx.x < 64) {                       // (jj, q): four chunk groups of eight per statistic, then a 4-lane sum
    const int q = threadIdx.x >> 3;             // 0 .. 7
    double v = ((red[8 * (4 * q) + jj] + red[8 * (4 * q + 1) + jj]) + (red[8 * (4 * q + 2) + jj] + red[8 * (4 * q + 3) + jj]));
    red2[threadIdx.x] = v;
  }
  __syncthreads();
  if (threadIdx.x < 8 && j < tot) {
    double v = 0.0;
#pragma unroll
    for (int q = 0; q < 8; ++q) v += red2[8 * q + jj];
    out[j] = v;
  }
  if (blockIdx.x == 0 && threadIdx.x == 0) out[tot] = (double)B;
}

}  // namespace svae

static void launch_reduce_stats(int B, int n, const double* E_init, const double* E_pair, const double* lognorm,
                                double* out, void* stream) {
  const int tot = 4 * n * n + n + 1;
  hipLaunchKernelGGL(svae::lds_reduce_stats_kernel, dim3((tot + 7) / 8), dim3(256), 0,
                     (hipStream_t)stream, B, n, E_init, E_pair, lognorm, out);
}

// svae_lds_reduce_stats_f64 and its XL twin: the same checks and launch, each on its own range of n
static int reduce_stats(int B, int n, int n_min, int n_max, const double* E_init, const double* E_pair,
                        const double* lognorm, double* out, void* stream) {
  if (B < 0) return -1;
  if (n < n_min || n > n_max) return -2;
  if (!E_init) return -3;
  if (!E_pair) return -4;
  if (!lognorm) return -5;
  if (!out) return -6;
  launch_reduce_stats(B, n, E_init, E_pair, lognorm, out, stream);
  return hipGetLastError() == hipSuccess ? 0 : -1000;
}

#ifndef SVAE_FILTER_WIDE_MAX_B
#define SVAE_FILTER_WIDE_MAX_B 6144     // filter-only launches without message outputs: the one-register filter (two sequences per wavefront beyond 512) up to this batch; measured 4096: 0.89 vs 0.96 ms packed, 8192: equal
#endif

extern "C" {

// Kernel selection (include/svae_hip.h, SVAE_OPT_*): keep == 0, n <= 10, T >= 4 -> the two-ended kernel
// (lds_estep_twoend.hpp: one sequence per wavefront, both elimination chains in one instruction stream).
// Otherwise batches up to 1023 run the one-directional latency variant (one sequence per wavefront, product
// stages split across the DPP rows: lds_estep_split.hpp), larger ones the packed kernel (four sequences per
// wavefront).  Measured crossover split/packed on MI355X (T=200, n=10): B ~ 1024 (one wavefront per SIMD).
// The selection is a function of the call's arguments only: the library holds no process-global state.
struct Selection { int twoend; bool split; int layout; int prod_max_b; };
static bool decode_options(unsigned options, int B, Selection* s) {
  if ((options & SVAE_OPT_LEAN_ON) && (options & SVAE_OPT_LEAN_OFF)) return false;
  options &= ~(SVAE_OPT_LEAN_ON | SVAE_OPT_LEAN_OFF | SVAE_OPT_INFER_RECORDS);   /* (record format: lean_applies) */
  if (options & ~SVAE_OPT_ALL) return false;
  if ((options & SVAE_OPT_TWOEND_OFF) && (options & SVAE_OPT_TWOEND_FULL)) return false;
  if ((options & SVAE_OPT_LAYOUT_SPLIT) && (options & SVAE_OPT_LAYOUT_PACKED)) return false;
  if ((options & SVAE_OPT_PRODUCERS_ON) && (options & SVAE_OPT_PRODUCERS_OFF)) return false;
  s->twoend = (options & SVAE_OPT_TWOEND_OFF) ? 0 : (options & SVAE_OPT_TWOEND_FULL) ? 2 : 1;
  s->layout = (options & SVAE_OPT_LAYOUT_SPLIT) ? 1 : (options & SVAE_OPT_LAYOUT_PACKED) ? 2 : 0;
  s->split = s->layout == 1 || (s->layout == 0 && B <= 1023);
  s->prod_max_b = (options & SVAE_OPT_PRODUCERS_ON) ? 0x7fffffff : (options & SVAE_OPT_PRODUCERS_OFF) ? 0 : 1024;
  return true;
}

int svae_hip_abi_version(void) { return SVAE_HIP_ABI_VERSION; }

// Record format of svae_lds_inference_f64 (and of the svae_lds_estep_vjp_ex_f64 call that reads its workspace with
// SVAE_OPT_INFER_RECORDS): a pure function of the arguments both calls share -- the library keeps no state.
static bool lean_applies(int B, int T, int n, int S, int inhomog, int keep_vjp, unsigned options) {
  if (n > svae::LEAN_MAX_N || T < 2 || S < 0 || S > svae::LEAN_MAX_S) return false;
  if (inhomog && keep_vjp) return false;          // per-step pair parameters: forward only (the VJP with statistics cotangents reads the full records)
  if ((long)T * svae::lean_rec_doubles(n) * 8 * 4 >= (1l << 31)) return false;     // 32-bit lane offsets inside a wavefront's records
  if (options & SVAE_OPT_LEAN_OFF) return false;
  if (options & SVAE_OPT_LEAN_ON) return true;
  if (options & (SVAE_OPT_LAYOUT_SPLIT | SVAE_OPT_PRODUCERS_ON)) return false;
  return B >= svae::LEAN_MIN_B;
}
int svae_lds_inference_is_lean(int B, int T, int n, int S, int inhomog, int keep_vjp, unsigned options) {
  return lean_applies(B, T, n, S, inhomog, keep_vjp, options) ? 1 : 0;
}

// main region: the one-directional layout (lds_args.hpp), then -- n <= 10 -- the two-ended one (a launch that
// keeps the sampler / VJP hand-off runs BOTH kernels, see svae_lds_estep_f64), then B doubles of scratch
static size_t one_ws_doubles(int B, int T, int n) { return (size_t)B * (size_t)svae::ws_seq_doubles(n, T); }
static size_t main_ws_doubles(int B, int T, int n) {
  const long two = n <= svae::TE_MAX_N ? svae::te_seq_doubles(n, T) : 0;
  return one_ws_doubles(B, T, n) + (size_t)B * (size_t)two + (size_t)B;
}
static size_t factor_ws_doubles(int B, int T, int n) { return (size_t)B * T * (n * n + n); }
static size_t cross_ws_doubles(int B, int T, int n) { return (size_t)B * T * (n + 1) * svae::ws_h_stride(n); }

// the regions behind the main one that a launch keeps (or a reader looks for): keep bit 0 = the factor region of the
// sampler, bit 1 = the cross moments of the VJP behind it; nullptr for a bit that is not set
struct Kept { double* factor; double* cross; };
static Kept kept_regions(const void* workspace, int B, int T, int n, int keep) {
  double* factor = (double*)workspace + main_ws_doubles(B, T, n);
  return {(keep & 1) ? factor : nullptr, (keep & 2) ? factor + factor_ws_doubles(B, T, n) : nullptr};
}

size_t svae_lds_tile_sigma_offset_bytes(int B, int T, int n, int inhomog, int pair_batched) {
  if (n <= SVAE_LDS_MAX_N || n > SVAE_LDS_TILE_MAX_N) return 0;
  return (svae_lds_workspace_bytes_ex(B, T, n, inhomog, pair_batched) + 255) / 256 * 256;
}

size_t svae_lds_workspace_bytes_ex(int B, int T, int n, int inhomog, int pair_batched) {
  if (B <= 0 || T <= 0 || n <= 0 || n > SVAE_LDS_TILE_MAX_N) return 0;
  if (n <= SVAE_LDS_MAX_N) return svae_lds_workspace_bytes(B, T, n);
  return ((size_t)B * T * svae_lds_tile_step_doubles(n) +
          svae_lds_tile_packed_doubles(B, T, n, inhomog, pair_batched)) * sizeof(double);
}

size_t svae_lds_workspace_bytes(int B, int T, int n) {
  if (B <= 0 || T <= 0 || n <= 0 || n > SVAE_LDS_TILE_MAX_N) return 0;
  if (n > SVAE_LDS_MAX_N) return svae_lds_workspace_bytes_ex(B, T, n, 0, 0);
  return (main_ws_doubles(B, T, n) + factor_ws_doubles(B, T, n) + cross_ws_doubles(B, T, n)) * sizeof(double);
}

int svae_lds_estep_f64(int B, int T, int n, int inhomog, int pair_batched, int keep, unsigned options,
                       const double* init_J, const double* init_h, const double* init_logZ,
                       const double* J11, const double* J12, const double* J22,
                       const double* logZ_pair,
                       const double* node_J, const double* node_h, const double* node_logZ,
                       double* lognorm, double* E_init, double* E_pair,
                       double* E_node_diagxx, double* E_node_x,
                       int32_t* info, void* workspace, size_t ws_bytes, void* stream) {
  if (B < 0) return -1;
  if (T < 1) return -2;
  if (n < 1 || n > SVAE_LDS_TILE_MAX_N) return -3;
  if (n > SVAE_LDS_MAX_N ? (keep & ~SVAE_KEEP_SIGMA) != 0 : (keep & ~3) != 0) return -23;   /* factor / cross regions: register path; Sigma: tiled path */
  if (pair_batched && !inhomog) return -5;
  svae::LdsArgs a{};
  svae::set_estep_args(a, B, T, n, pair_batched, init_J, init_h, init_logZ, J11, J12, J22, logZ_pair, node_J, node_h, node_logZ,
                       lognorm, E_init, E_pair, E_node_diagxx, E_node_x, info, workspace);
  if (const int rc = svae::check_model(a)) return rc;
  if (const int rc = svae::check_arrays(a)) return rc;
  if (!workspace || ws_bytes < svae_lds_workspace_bytes_ex(B, T, n, inhomog, pair_batched)) return -22;
  Selection sel;
  const unsigned tile_bits = options & (SVAE_OPT_TILE_FORWARD | SVAE_OPT_TILE_BACKWARD);
  if (tile_bits == (SVAE_OPT_TILE_FORWARD | SVAE_OPT_TILE_BACKWARD) || (tile_bits && n <= SVAE_LDS_MAX_N)) return -24;
  if (!decode_options(options & ~tile_bits, B, &sel)) return -24;
  if (B == 0) return 0;
  const int twoend = sel.twoend;

  a.tile_half = (tile_bits & SVAE_OPT_TILE_FORWARD) ? 1 : (tile_bits & SVAE_OPT_TILE_BACKWARD) ? 2 : 0;
  if (n > SVAE_LDS_MAX_N) {
    if (keep & SVAE_KEEP_SIGMA) {
      const size_t off = svae_lds_tile_sigma_offset_bytes(B, T, n, inhomog, pair_batched);
      if (ws_bytes < off + (size_t)B * T * n * n * sizeof(double)) return -22;
      a.sig_out = (double*)((char*)workspace + off);
    }
    return svae_lds_launch_tile(&a, n, inhomog, stream);
  }
  const Kept kept = kept_regions(workspace, B, T, n, keep);
  a.ws2 = kept.factor; a.ws3 = kept.cross;
  const svae::EstepUnit* unit = estep_units[n];
  const bool split = sel.split;
  if (twoend && keep && split && n <= svae::TE_MAX_N && T >= svae::TE_MIN_T) {
    // Small batch, hand-off kept: the statistics (and the cross moments the VJP reads: posterior moments, the same
    // whichever way the chain is eliminated) come from the two-ended kernel, while the one-directional FILTER --
    // whose factorisation defines the sampler's eps -> sample map and the records the sweeps differentiate --
    // runs NEXT to it on the SIMDs the small batch leaves idle (512 + 512 wavefronts on 1024 SIMDs at B = 512).
    // Round 4: both in ONE launch (lds_forward_pair_kernel: the first B workgroups take the filter's body, the next
    // B the E-step's) instead of two kernels on two streams forked and joined by events (0.31 -> 0.27 ms at B = 512).
    svae::LdsArgs f = a;                       // the filter: one-directional layout at the start of the workspace
    f.ws2 = kept_regions(workspace, B, T, n, 1).factor;
    f.ws3 = nullptr;
    f.lognorm = f.ws2 - B;                     // scratch: the B doubles that end the main region (the E-step's lognorm is the other kernel's)
    f.E_init = nullptr; f.E_pair = nullptr; f.E_node_diagxx = nullptr; f.E_node_x = nullptr;
    svae::LdsArgs e = a;                       // the E-step: two-ended records behind the one-directional ones
    e.ws = (double*)workspace + one_ws_doubles(B, T, n);
    e.ws2 = nullptr;
    return unit->forward_pair(f, e, inhomog, stream);
  }
  if (twoend && !keep && n <= svae::TE_MAX_N && T >= svae::TE_MIN_T)
    return unit->twoend(a, inhomog, twoend == 1 && !inhomog, sel.layout, stream);
  return split ? unit->estep_split(a, inhomog, stream) : unit->estep(a, inhomog, stream);
}

int svae_lds_filter_f64(int B, int T, int n, int inhomog, int pair_batched, unsigned options,
                        const double* init_J, const double* init_h, const double* init_logZ,
                        const double* J11, const double* J12, const double* J22, const double* logZ_pair,
                        const double* node_J, const double* node_h, const double* node_logZ,
                        double* lognorm, double* J_pred, double* h_pred, double* J_filt, double* h_filt,
                        int32_t* info, void* workspace, size_t ws_bytes, void* stream) {
  if (B < 0) return -1;
  if (T < 1) return -2;
  if (n < 1 || n > SVAE_LDS_MAX_N) return -3;
  if (pair_batched && !inhomog) return -5;
  svae::LdsArgs a{};
  svae::set_estep_args(a, B, T, n, pair_batched, init_J, init_h, init_logZ, J11, J12, J22, logZ_pair, node_J, node_h, node_logZ,
                       lognorm, nullptr, nullptr, nullptr, nullptr, info, workspace);
  if (const int rc = svae::check_model(a)) return rc;
  if (!node_J) return -13;
  if (!node_h) return -14;
  if (!lognorm) return -16;
  if (!info) return -21;
  if (!workspace || ws_bytes < svae_lds_workspace_bytes(B, T, n)) return -22;
  Selection sel;
  if (!decode_options(options, B, &sel)) return -24;
  if (B == 0) return 0;
  const int twoend = sel.twoend;
  a.ws2 = kept_regions(workspace, B, T, n, 1).factor;         // factor region: the sampler may follow
  a.msg_Jp = J_pred; a.msg_hp = h_pred; a.msg_Jf = J_filt; a.msg_hf = h_filt;
  // small batches without message outputs: one sequence per wavefront (0.62 -> 0.24 ms at B = 512, T = 200, n = 10).
  // The one-register filter (n <= 10) stays ahead of the packed kernel until ~3 wavefronts per SIMD (filter + sampler,
  // T = 500: 1024 sequences 0.86 vs 1.81 ms, 2048: 1.85 vs 2.53; T = 200, 4096: 1.43 vs 1.27)
  const bool wide = sel.layout == 1 || (sel.layout == 0 && B <= (n <= svae::TE_MAX_N && twoend ? SVAE_FILTER_WIDE_MAX_B : 1023));
  const bool fsplit = wide && !J_pred && !h_pred && !J_filt && !h_filt;
  const svae::EstepUnit* unit = estep_units[n];
  if (!fsplit) return unit->filter(a, inhomog, stream);
  return (n <= svae::TE_MAX_N && twoend) ? unit->filter_1r(a, inhomog, stream) : unit->filter_split(a, inhomog, stream);
}

size_t svae_slds_lds_meanfield_workspace_bytes(int rows, int T, int n) {
  if (rows <= 0 || T < svae::TE_MIN_T || n < 1 || n > svae::TE_MAX_N) return 0;
  return (size_t)rows * (size_t)svae::te_seq_doubles(n, T) * sizeof(double);     // the two-ended records only
}

size_t svae_slds_lds_meanfield_lds_bytes(int n, int K) {
  if (n < 1 || n > svae::TE_MAX_N || K < 1 || K > svae::TE_MIX_MAX_K) return 0;
  return (size_t)svae::te_mix_lds_bytes(n, K);
}

int svae_slds_lds_meanfield_f64(int B, int rows, int T, int n, int K,
                                const double* init_J, const double* init_h,
                                const double* J11, const double* J12, const double* J22,
                                const double* weights,
                                const double* node_J, const double* node_h, const double* node_logZ,
                                const int32_t* seq_index,
                                double* lognorm, double* E_init, double* E_node_diagxx, double* E_node_x,
                                double* pair_contr, int32_t* info,
                                void* workspace, size_t ws_bytes, unsigned options, void* stream) {
  if (B < 0 || B > rows) return -1;
  if (T < svae::TE_MIN_T) return -2;
  if (n < 1 || n > svae::TE_MAX_N) return -3;
  if (K < 1 || K > svae::TE_MIX_MAX_K || svae::te_mix_lds_bytes(n, K) > svae::TE_MIX_MAX_LDS) return -4;
  if (!init_J) return -5;
  if (!init_h) return -6;
  if (!J11 || !J12 || !J22) return -7;
  if (!weights) return -10;
  if (!node_J) return -11;
  if (!node_h) return -12;
  if (!lognorm) return -15;
  if (!E_init) return -16;
  if (!E_node_diagxx) return -17;
  if (!E_node_x) return -18;
  if (!pair_contr) return -19;
  if (!info) return -20;
  if (!workspace || ws_bytes < svae_slds_lds_meanfield_workspace_bytes(rows, T, n)) return -21;
  // kernel selection (a pure function of the arguments): SVAE_OPT_LAYOUT_SPLIT = one sequence per wavefront, the K
  // parameter sets as LDS tables (rounds 2 - 4); SVAE_OPT_LAYOUT_PACKED = row-per-chain consumers + MFMA producer
  // wavefronts (round 5; K <= 8, workspace below 4 GiB: 32-bit lane offsets); 0 = the latter where it applies.
  // SVAE_OPT_PRODUCERS_OFF with the packed layout: reference producers (plain loops, no MFMA: test infrastructure).
  if (options & ~(SVAE_OPT_LAYOUT_SPLIT | SVAE_OPT_LAYOUT_PACKED | SVAE_OPT_PRODUCERS_OFF)) return -24;
  if ((options & SVAE_OPT_LAYOUT_SPLIT) && (options & SVAE_OPT_LAYOUT_PACKED)) return -24;
  const bool rpc_ok = K <= 8 && svae_slds_lds_meanfield_workspace_bytes(rows, T, n) < (1ull << 32);
  if ((options & SVAE_OPT_LAYOUT_PACKED) && !rpc_ok) return -24;
  const bool rpc = rpc_ok && !(options & SVAE_OPT_LAYOUT_SPLIT);
  if (B == 0) return 0;
  svae::LdsArgs a{};
  svae::set_estep_args(a, B, T, n, 0, init_J, init_h, nullptr, J11, J12, J22, nullptr, node_J, node_h, node_logZ,
                       lognorm, E_init, nullptr, E_node_diagxx, E_node_x, info, workspace);
  a.mix_w = weights; a.mix_out = pair_contr; a.seq_index = seq_index; a.mix_K = K;
  const svae::EstepUnit* unit = estep_units[n];
  return rpc ? unit->slds_rpc(a, (options & SVAE_OPT_PRODUCERS_OFF) ? 1 : 0, (options & SVAE_OPT_LAYOUT_PACKED) ? 0 : 1, stream)
             : unit->twoend_mix(a, stream);
}

int svae_lds_reduce_stats_f64(int B, int n, const double* E_init, const double* E_pair,
                              const double* lognorm, double* out, void* stream) {
  return reduce_stats(B, n, 1, SVAE_LDS_TILE_MAX_N, E_init, E_pair, lognorm, out, stream);
}

int svae_lds_xl_reduce_stats_f64(int B, int n, const double* E_init, const double* E_pair,
                                 const double* lognorm, double* out, void* stream) {
  return reduce_stats(B, n, SVAE_LDS_TILE_MAX_N + 1, SVAE_LDS_XL_MAX_N, E_init, E_pair, lognorm, out, stream);
}

}  // extern "C"

static svae::SampleArgs sample_args(int B, int T, int n, int S, int prod_max_b, const double* eps, double* samples,
                                    const void* workspace) {
  svae::SampleArgs a{};
  a.B = B; a.T = T; a.S = S; a.eps = eps; a.samples = samples;
  a.prod_max_b = prod_max_b;
  a.ws = (const double*)workspace;
  a.ws2 = kept_regions(workspace, B, T, n, 1).factor;
  return a;
}

extern "C" int svae_lds_sample_f64(int B, int T, int n, int S, unsigned options, const double* eps, double* samples,
                                   const void* workspace, size_t ws_bytes, void* stream) {
  if (B < 0) return -1;
  if (T < 1) return -2;
  if (n < 1 || n > SVAE_LDS_MAX_N) return -3;
  if (S < 1) return -4;
  if (!eps) return -5;
  if (!samples) return -6;
  if (!workspace || ws_bytes < svae_lds_workspace_bytes(B, T, n)) return -7;
  Selection sel;
  if (!decode_options(options, B, &sel)) return -24;
  if (B == 0) return 0;
  return estep_units[n]->sample(sample_args(B, T, n, S, sel.prod_max_b, eps, samples, workspace), stream);
}

extern "C" int svae_lds_inference_f64(int B, int T, int n, int S, int inhomog, int pair_batched, int keep_vjp, unsigned options,
                                      const double* init_J, const double* init_h, const double* init_logZ,
                                      const double* J11, const double* J12, const double* J22, const double* logZ_pair,
                                      const double* node_J, const double* node_h, const double* node_logZ,
                                      const double* eps, double* samples,
                                      double* lognorm, double* E_init, double* E_pair,
                                      double* E_node_diagxx, double* E_node_x,
                                      int32_t* info, void* workspace, size_t ws_bytes, void* stream) {
  if (n < 1 || n > SVAE_LDS_MAX_N) return -3;
  if (S < 0 || (S > 0 && (!eps || !samples))) return -4;
  if (!lean_applies(B, T, n, S, inhomog, keep_vjp, options)) {
    // the general path: E-step keeping the hand-off, the factor and (keep_vjp) the cross moments, then the sampler
    const unsigned o = options & SVAE_OPT_ALL;
    const int rc = svae_lds_estep_f64(B, T, n, inhomog, pair_batched, keep_vjp ? 3 : (S > 0 ? 1 : 0), o, init_J, init_h, init_logZ, J11, J12, J22,
                                      logZ_pair, node_J, node_h, node_logZ, lognorm, E_init, E_pair, E_node_diagxx,
                                      E_node_x, info, workspace, ws_bytes, stream);
    if (rc != 0 || S == 0 || B == 0) return rc;
    const int rs = svae_lds_sample_f64(B, T, n, S, o, eps, samples, workspace, ws_bytes, stream);
    return rs == 0 ? 0 : -100 + rs;
  }
  if (B < 0) return -1;
  svae::LdsArgs a{};
  svae::set_estep_args(a, B, T, n, pair_batched, init_J, init_h, init_logZ, J11, J12, J22, logZ_pair, node_J, node_h, node_logZ,
                       lognorm, E_init, E_pair, E_node_diagxx, E_node_x, info, workspace);    // lean records at the start of the main region
  if (const int rc = svae::check_model(a)) return rc;       // (T >= 2 here: lean_applies)
  if (pair_batched && !inhomog) return -5;
  if (const int rc = svae::check_arrays(a)) return rc;
  if (!workspace || ws_bytes < svae_lds_workspace_bytes(B, T, n)) return -22;
  Selection sel;
  if (!decode_options(options, B, &sel)) return -24;
  if (B == 0) return 0;
  a.ws3 = kept_regions(workspace, B, T, n, keep_vjp ? 2 : 0).cross;   // cross moments: where the VJP looks
  svae::LeanSample ls;
  ls.S = S; ls.eps = eps; ls.samples = samples;
  return estep_units[n]->infer_lean(a, ls, inhomog, stream);
}

extern "C" size_t svae_lds_vjp_workspace_bytes(int B, int T, int n) {
  if (B <= 0 || T <= 0 || n <= 0 || n > SVAE_LDS_MAX_N) return 0;
  return (size_t)B * T * svae::vjp_step_doubles(n) * sizeof(double);
}

// what every VJP launch carries; the caller adds J12 and its strides and the cotangents of the E_init / E_pair / parameters
static svae::VjpArgs vjp_args(int B, int T, int n, int S, int prod_max_b, const double* g_lognorm,
                              const double* g_E_node_diagxx, const double* g_E_node_x, const double* g_samples,
                              const double* eps, const double* samples, double* g_node_J, double* g_node_h,
                              const void* workspace, void* vjp_workspace) {
  svae::VjpArgs a{};
  a.B = B; a.T = T; a.S = g_samples ? S : 0;
  a.prod_max_b = prod_max_b;
  a.g_lognorm = g_lognorm; a.g_diagxx = g_E_node_diagxx; a.g_x = g_E_node_x;
  a.g_samples = g_samples; a.eps = eps; a.samples = samples;
  a.g_node_J = g_node_J; a.g_node_h = g_node_h;
  const Kept kept = kept_regions(workspace, B, T, n, 3);
  a.ws = (const double*)workspace; a.ws2 = kept.factor; a.ws3 = kept.cross;
  a.adj = (double*)vjp_workspace;
  return a;
}

static int vjp_impl(int B, int T, int n, int S, int inhomog, int pair_batched, unsigned options,
                    const double* J12, const double* g_lognorm,
                    const double* g_E_node_diagxx, const double* g_E_node_x,
                    const double* g_E_init, const double* g_E_pair,
                    const double* g_samples, const double* eps,
                    const double* samples, const double* E_pair,
                    const double* E_node_x, double* g_node_J, double* g_node_h, double* g_node_J_dense, double* g_R,
                    const void* workspace, size_t ws_bytes,
                    void* vjp_workspace, size_t vjp_ws_bytes, void* stream) {
  if (B < 0) return -1;
  if (T < 1) return -2;
  if (n < 1 || n > SVAE_LDS_MAX_N) return -3;
  if (g_samples && (S < 1 || S > 16)) return -4;
  if (T > 1 && !J12) return -5;
  if (!g_lognorm) return -6;
  if (pair_batched && !inhomog) return -7;
  if (g_E_pair && (!inhomog || !E_pair || !E_node_x)) return -8;   /* per-step statistics only */
  if (g_samples && (!eps || !samples)) return -10;
  if (!g_node_J) return -12;
  if (!g_node_h) return -13;
  if (!workspace || ws_bytes < svae_lds_workspace_bytes(B, T, n)) return -14;
  if (!vjp_workspace || vjp_ws_bytes < svae_lds_vjp_workspace_bytes(B, T, n)) return -16;
  Selection sel;
  if (!decode_options(options, B, &sel)) return -24;
  if (B == 0) return 0;
  svae::VjpArgs a = vjp_args(B, T, n, S, sel.prod_max_b, g_lognorm, g_E_node_diagxx, g_E_node_x, g_samples, eps, samples,
                             g_node_J, g_node_h, workspace, vjp_workspace);
  a.J12 = J12;
  a.pair_t_stride = inhomog ? (long)n * n : 0;
  a.pair_seq_stride = pair_batched ? (long)(T - 1) * n * n : 0;
  a.g_E_init = g_E_init; a.g_E_pair = g_E_pair; a.E_pair = E_pair; a.E_node_x = E_node_x;
  a.g_P = g_node_J_dense;
  a.g_R = g_R;
  if (g_node_J_dense && !g_R) a.prod_max_b = 0;  /* the packed sweeps write it (with g_R: launch_vjp adds the packed sweep 2 where the selection is another) */
  if ((options & SVAE_OPT_INFER_RECORDS) && lean_applies(B, T, n, S, inhomog, 1, options)) {
    if (g_E_init || g_E_pair || g_node_J_dense) return -8;        /* lean records: cotangents of the node statistics, lognorm and samples */
    return vjp_units[n]->vjp_lean(a, stream);
  }
  return vjp_units[n]->vjp(a, stream);
}

extern "C" int svae_lds_estep_vjp_ex_f64(int B, int T, int n, int S, int inhomog, int pair_batched, unsigned options,
                                         const double* J12, const double* g_lognorm,
                                         const double* g_E_node_diagxx, const double* g_E_node_x,
                                         const double* g_E_init, const double* g_E_pair,
                                         const double* g_samples, const double* eps,
                                         const double* samples, const double* E_pair,
                                         const double* E_node_x, double* g_node_J, double* g_node_h,
                                         const void* workspace, size_t ws_bytes,
                                         void* vjp_workspace, size_t vjp_ws_bytes, void* stream) {
  return vjp_impl(B, T, n, S, inhomog, pair_batched, options, J12, g_lognorm, g_E_node_diagxx, g_E_node_x, g_E_init, g_E_pair,
                  g_samples, eps, samples, E_pair, E_node_x, g_node_J, g_node_h, nullptr, nullptr, workspace, ws_bytes,
                  vjp_workspace, vjp_ws_bytes, stream);
}

extern "C" int svae_lds_estep_vjp_dense_f64(int B, int T, int n, int S, int inhomog, int pair_batched, unsigned options,
                                            const double* J12, const double* g_lognorm,
                                            const double* g_E_node_diagxx, const double* g_E_node_x,
                                            const double* g_E_init, const double* g_E_pair,
                                            const double* g_samples, const double* eps,
                                            const double* samples, const double* E_pair,
                                            const double* E_node_x, double* g_node_J, double* g_node_h,
                                            double* g_node_J_dense,
                                            const void* workspace, size_t ws_bytes,
                                            void* vjp_workspace, size_t vjp_ws_bytes, void* stream) {
  if (!g_node_J_dense) return -27;
  return vjp_impl(B, T, n, S, inhomog, pair_batched, options, J12, g_lognorm, g_E_node_diagxx, g_E_node_x, g_E_init, g_E_pair,
                  g_samples, eps, samples, E_pair, E_node_x, g_node_J, g_node_h, g_node_J_dense, nullptr, workspace, ws_bytes,
                  vjp_workspace, vjp_ws_bytes, stream);
}

extern "C" int svae_lds_param_grad_launch(int B, int T, int n, int inhomog, int pair_batched, const double* g_P,
                                          const double* g_R, const double* g_node_h, const double* g_lognorm, double* part,
                                          double* g_init_J, double* g_init_h, double* g_init_logZ, double* g_J11,
                                          double* g_J12, double* g_J22, double* g_logZ_pair, void* stream);

extern "C" size_t svae_lds_param_vjp_workspace_bytes(int B, int T, int n, int inhomog, int pair_batched) {
  if (B <= 0 || T <= 0 || n <= 0 || n > SVAE_LDS_MAX_N) return 0;
  (void)pair_batched;
  return (size_t)(svae::pg_gp_doubles(B, T, n) + svae::pg_gr_doubles(B, T, n) + svae::pg_part_doubles(T, n, inhomog)) * sizeof(double);
}

extern "C" int svae_lds_estep_vjp_params_f64(int B, int T, int n, int S, int inhomog, int pair_batched, unsigned options,
                                             const double* J12, const double* g_lognorm,
                                             const double* g_E_node_diagxx, const double* g_E_node_x,
                                             const double* g_E_init, const double* g_E_pair,
                                             const double* g_samples, const double* eps,
                                             const double* samples, const double* E_pair,
                                             const double* E_node_x, double* g_node_J, double* g_node_h,
                                             double* g_init_J, double* g_init_h, double* g_init_logZ,
                                             double* g_J11, double* g_J12, double* g_J22, double* g_logZ_pair,
                                             const void* workspace, size_t ws_bytes,
                                             void* vjp_workspace, size_t vjp_ws_bytes,
                                             void* param_workspace, size_t param_ws_bytes, void* stream) {
  const size_t need = svae_lds_param_vjp_workspace_bytes(B, T, n, inhomog, pair_batched);
  /* (need == 0: B = 0, or sizes that vjp_impl refuses with their own codes) */
  if (need > 0 && (!param_workspace || param_ws_bytes < need)) return -29;
  if (B > 0 && T > 65536) return -30;           /* (one workgroup row per step in the reduction's grid) */
  double* g_P = (double*)param_workspace;
  double* g_R = need > 0 ? g_P + svae::pg_gp_doubles(B, T, n) : nullptr;
  double* part = need > 0 ? g_R + svae::pg_gr_doubles(B, T, n) : nullptr;
  const int rc = vjp_impl(B, T, n, S, inhomog, pair_batched, options, J12, g_lognorm, g_E_node_diagxx, g_E_node_x, g_E_init, g_E_pair,
                          g_samples, eps, samples, E_pair, E_node_x, g_node_J, g_node_h, g_P, g_R, workspace, ws_bytes,
                          vjp_workspace, vjp_ws_bytes, stream);
  if (rc != 0 || B == 0) return rc;
  const int rr = svae_lds_param_grad_launch(B, T, n, inhomog, pair_batched, g_P, g_R, g_node_h, g_lognorm, part,
                                            g_init_J, g_init_h, g_init_logZ, g_J11, g_J12, g_J22, g_logZ_pair, stream);
  return rr;
}

extern "C" int svae_lds_estep_vjp_f64(int B, int T, int n, int S, const double* J12,
                                      const double* g_lognorm, const double* g_E_node_diagxx,
                                      const double* g_E_node_x, const double* g_samples,
                                      const double* eps, const double* samples,
                                      double* g_node_J, double* g_node_h,
                                      const void* workspace, size_t ws_bytes,
                                      void* vjp_workspace, size_t vjp_ws_bytes, void* stream) {
  return svae_lds_estep_vjp_ex_f64(B, T, n, S, 0, 0, SVAE_OPT_DEFAULT, J12, g_lognorm, g_E_node_diagxx, g_E_node_x,
                                   nullptr, nullptr, g_samples, eps, samples, nullptr, nullptr,
                                   g_node_J, g_node_h, workspace, ws_bytes, vjp_workspace,
                                   vjp_ws_bytes, stream);
}

// ---- per-sequence lengths (svae_lds_ragged_*) ----------------------------------------------------------------------
// Sequence b of length L = lengths[b] inside the padded length T is the chain whose pairs t <= L-2 carry the real pair
// parameters and whose pairs t >= L-1 carry the decoupling set Q = (0, 0, -1/2 I, 0), with zero node potentials from step L
// on (lds_estep_kernel.hpp, RAG).  The kernels read the pair blocks from two-entry tables [real | Q] that a one-workgroup
// kernel leaves behind the workspace of the uniform entry points; the VJP finds its J12 table there.  One route at every
// batch size: the packed one-directional E-step (full records), the packed samplers and the packed sweeps.
namespace svae {

// tab = [J11 | 0] [J12 | 0] [J22 | -1/2 I]  (6 n^2 doubles); T = 1: no pair parameters (NULL), the real entries are 0
__global__ __launch_bounds__(256) void lds_ragged_tables_kernel(int n, const double* J11, const double* J12,
                                                                 const double* J22, double* tab) {
  const int nn = n * n;
  for (int e = threadIdx.x; e < nn; e += blockDim.x) {
    tab[e] = J11 ? J11[e] : 0.0;
    tab[nn + e] = 0.0;
    tab[2 * nn + e] = J12 ? J12[e] : 0.0;
    tab[3 * nn + e] = 0.0;
    tab[4 * nn + e] = J22 ? J22[e] : 0.0;
    tab[5 * nn + e] = (e / n == e % n) ? -0.5 : 0.0;
  }
}

// qtab = [0 | -1/2 I]  (2 n^2 doubles): J11 = J12 = 0 and J22 = -1/2 I of the decoupling set Q, what the per-step ragged
// E-step (svae_lds_ragged_perstep_*) reads at the pairs t >= lengths[b] - 1 instead of the caller's blocks
__global__ __launch_bounds__(256) void lds_ragged_qtable_kernel(int n, double* qtab) {
  const int nn = n * n;
  for (int e = threadIdx.x; e < nn; e += blockDim.x) {
    qtab[e] = 0.0;
    qtab[nn + e] = (e / n == e % n) ? -0.5 : 0.0;
  }
}

// out[slot] = sum_b (clamp(lengths[b], 1, T) - 1): integer partial sums in a fixed tree, exact in any order
__global__ __launch_bounds__(256) void lds_ragged_pair_count_kernel(int B, int T, const int32_t* lengths, double* out) {
  __shared__ long long red[256];
  long long acc = 0;
  for (int b = threadIdx.x; b < B; b += 256) {
    const int l = lengths[b];
    acc += (l < 1 ? 1 : (l > T ? T : l)) - 1;
  }
  red[threadIdx.x] = acc;
  __syncthreads();
  for (int s = 128; s > 0; s >>= 1) {
    if ((int)threadIdx.x < s) red[threadIdx.x] += red[threadIdx.x + s];
    __syncthreads();
  }
  if (threadIdx.x == 0) out[0] = (double)red[0];
}

}  // namespace svae

static size_t ragged_table_offset_bytes(int B, int T, int n) { return (svae_lds_workspace_bytes(B, T, n) + 255) / 256 * 256; }

extern "C" size_t svae_lds_ragged_workspace_bytes(int B, int T, int n) {
  if (B <= 0 || T <= 0 || n <= 0 || n > SVAE_LDS_MAX_N) return 0;
  return ragged_table_offset_bytes(B, T, n) + (size_t)6 * n * n * sizeof(double);
}

extern "C" size_t svae_lds_ragged_perstep_workspace_bytes(int B, int T, int n) {
  if (B <= 0 || T <= 0 || n <= 0 || n > SVAE_LDS_MAX_N) return 0;
  return ragged_table_offset_bytes(B, T, n) + (size_t)2 * n * n * sizeof(double);
}

extern "C" int svae_lds_ragged_estep_f64(int B, int T, int n, int inhomog, int pair_batched, int keep, unsigned options,
                                         const double* init_J, const double* init_h, const double* init_logZ,
                                         const double* J11, const double* J12, const double* J22, const double* logZ_pair,
                                         const double* node_J, const double* node_h, const double* node_logZ,
                                         const int32_t* lengths,
                                         double* lognorm, double* E_init, double* E_pair,
                                         double* E_node_diagxx, double* E_node_x,
                                         int32_t* info, void* workspace, size_t ws_bytes, void* stream) {
  if (B < 0) return -1;
  if (T < 1) return -2;
  if (n < 1 || n > SVAE_LDS_MAX_N) return -3;
  if (inhomog || pair_batched) return -32;       /* pair parameters shared by the batch and by the steps */
  if (!lengths) return -31;
  if ((keep & ~3) != 0) return -23;
  svae::LdsArgs a{};
  svae::set_estep_args(a, B, T, n, 0, init_J, init_h, init_logZ, J11, J12, J22, logZ_pair, node_J, node_h, node_logZ,
                       lognorm, E_init, E_pair, E_node_diagxx, E_node_x, info, workspace);
  if (const int rc = svae::check_model(a)) return rc;
  if (const int rc = svae::check_arrays(a)) return rc;
  Selection sel;
  if (!decode_options(options, B, &sel)) return -24;      /* (a valid word; the ragged dispatcher has one route) */
  if (B == 0) return 0;
  if (!workspace || ws_bytes < svae_lds_ragged_workspace_bytes(B, T, n)) return -22;
  double* tab = (double*)((char*)workspace + ragged_table_offset_bytes(B, T, n));
  hipLaunchKernelGGL(svae::lds_ragged_tables_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, n, J11, J12, J22, tab);
  if (hipGetLastError() != hipSuccess) return -1000;
  const long nn = (long)n * n;
  a.J11 = tab; a.J12 = tab + 2 * nn; a.J22 = tab + 4 * nn;
  const Kept kept = kept_regions(workspace, B, T, n, keep);
  a.ws2 = kept.factor; a.ws3 = kept.cross;
  a.lengths = lengths;
  return estep_units[n]->ragged(a, stream);
}

// per-step pair parameters (T-1,n,n) or, pair_batched, (B,T-1,n,n), and an init potential per batch or, init_batched, per
// sequence: the packed E-step in its INHOMOG + RAG instantiation; the decoupling set's blocks come from a table behind the
// uniform workspace layout.  keep_bits: the bits of `keep` the calling entry point accepts (-23 for any other)
static int ragged_perstep_estep(int B, int T, int n, int pair_batched, int init_batched, int keep, int keep_bits,
                                unsigned options,
                                const double* init_J, const double* init_h, const double* init_logZ,
                                const double* J11, const double* J12, const double* J22, const double* logZ_pair,
                                const double* node_J, const double* node_h, const double* node_logZ,
                                const int32_t* lengths,
                                double* lognorm, double* E_init, double* E_pair,
                                double* E_node_diagxx, double* E_node_x,
                                int32_t* info, void* workspace, size_t ws_bytes, void* stream) {
  if (B < 0) return -1;
  if (T < 1) return -2;
  if (n < 1 || n > SVAE_LDS_MAX_N) return -3;
  if ((pair_batched & ~1) != 0 || (init_batched & ~1) != 0) return -32;
  if (!lengths) return -31;
  if ((keep & ~keep_bits) != 0) return -23;
  svae::LdsPerstepArgs a{};
  svae::set_estep_args(a, B, T, n, pair_batched, init_J, init_h, init_logZ, J11, J12, J22, logZ_pair, node_J, node_h, node_logZ,
                       lognorm, E_init, E_pair, E_node_diagxx, E_node_x, info, workspace);
  if (const int rc = svae::check_model(a)) return rc;
  if (const int rc = svae::check_arrays(a, T > 1)) return rc;       /* E_pair (B,T-1,3,n,n): empty for T = 1 */
  Selection sel;
  if (!decode_options(options, B, &sel)) return -24;      /* (a valid word; one route) */
  if (B == 0) return 0;
  if (!workspace || ws_bytes < svae_lds_ragged_perstep_workspace_bytes(B, T, n)) return -22;
  double* qtab = (double*)((char*)workspace + ragged_table_offset_bytes(B, T, n));
  hipLaunchKernelGGL(svae::lds_ragged_qtable_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, n, qtab);
  if (hipGetLastError() != hipSuccess) return -1000;
  /* T = 1: no pair is ever addressed (pair 0 <= L-2 needs L >= 2 > T); the table stands in for the NULL arrays */
  if (T == 1) a.J11 = a.J12 = a.J22 = qtab;
  const Kept kept = kept_regions(workspace, B, T, n, keep);
  a.ws2 = kept.factor; a.ws3 = kept.cross;        /* (cross moments: with the factor only, the KEEPW instantiation) */
  a.lengths = lengths;
  a.qtab = qtab;
  a.init_batched = init_batched;
  return estep_units[n]->ragged_perstep(a, stream);
}

extern "C" int svae_lds_ragged_perstep_estep_f64(int B, int T, int n, int pair_batched, int init_batched, int keep,
                                                 unsigned options,
                                                 const double* init_J, const double* init_h, const double* init_logZ,
                                                 const double* J11, const double* J12, const double* J22, const double* logZ_pair,
                                                 const double* node_J, const double* node_h, const double* node_logZ,
                                                 const int32_t* lengths,
                                                 double* lognorm, double* E_init, double* E_pair,
                                                 double* E_node_diagxx, double* E_node_x,
                                                 int32_t* info, void* workspace, size_t ws_bytes, void* stream) {
  /* keep bit 1, the cross moments of the VJP, is refused here: svae_lds_ragged_perstep_inference_keep_f64 keeps them */
  return ragged_perstep_estep(B, T, n, pair_batched, init_batched, keep, 1, options, init_J, init_h, init_logZ, J11, J12, J22,
                              logZ_pair, node_J, node_h, node_logZ, lengths, lognorm, E_init, E_pair, E_node_diagxx, E_node_x,
                              info, workspace, ws_bytes, stream);
}

static int ragged_sample(int B, int T, int n, int S, const double* eps, double* samples, const int32_t* lengths,
                         const void* workspace, void* stream) {
  svae::SampleArgs a = sample_args(B, T, n, S, 0, eps, samples, workspace);
  a.lengths = lengths;
  return estep_units[n]->sample_ragged(a, stream);
}

extern "C" int svae_lds_ragged_inference_f64(int B, int T, int n, int S, int inhomog, int pair_batched, int keep_vjp,
                                             unsigned options,
                                             const double* init_J, const double* init_h, const double* init_logZ,
                                             const double* J11, const double* J12, const double* J22, const double* logZ_pair,
                                             const double* node_J, const double* node_h, const double* node_logZ,
                                             const int32_t* lengths, const double* eps, double* samples,
                                             double* lognorm, double* E_init, double* E_pair,
                                             double* E_node_diagxx, double* E_node_x,
                                             int32_t* info, void* workspace, size_t ws_bytes, void* stream) {
  if (n < 1 || n > SVAE_LDS_MAX_N) return -3;
  if (S < 0 || (S > 0 && (!eps || !samples))) return -4;
  if (keep_vjp != 0 && keep_vjp != 1) return -23;
  const int rc = svae_lds_ragged_estep_f64(B, T, n, inhomog, pair_batched, keep_vjp ? 3 : (S > 0 ? 1 : 0), options, init_J, init_h,
                                           init_logZ, J11, J12, J22, logZ_pair, node_J, node_h, node_logZ, lengths, lognorm,
                                           E_init, E_pair, E_node_diagxx, E_node_x, info, workspace, ws_bytes, stream);
  if (rc != 0 || S == 0 || B == 0) return rc;
  return ragged_sample(B, T, n, S, eps, samples, lengths, workspace, stream);
}

extern "C" int svae_lds_ragged_perstep_inference_f64(int B, int T, int n, int S, int pair_batched, int init_batched,
                                                     unsigned options,
                                                     const double* init_J, const double* init_h, const double* init_logZ,
                                                     const double* J11, const double* J12, const double* J22,
                                                     const double* logZ_pair,
                                                     const double* node_J, const double* node_h, const double* node_logZ,
                                                     const int32_t* lengths, const double* eps, double* samples,
                                                     double* lognorm, double* E_init, double* E_pair,
                                                     double* E_node_diagxx, double* E_node_x,
                                                     int32_t* info, void* workspace, size_t ws_bytes, void* stream) {
  if (n < 1 || n > SVAE_LDS_MAX_N) return -3;
  if (S < 0 || (S > 0 && (!eps || !samples))) return -4;
  const int rc = svae_lds_ragged_perstep_estep_f64(B, T, n, pair_batched, init_batched, S > 0 ? 1 : 0, options, init_J, init_h,
                                                   init_logZ, J11, J12, J22, logZ_pair, node_J, node_h, node_logZ, lengths,
                                                   lognorm, E_init, E_pair, E_node_diagxx, E_node_x, info, workspace, ws_bytes,
                                                   stream);
  if (rc != 0 || S == 0 || B == 0) return rc;
  return ragged_sample(B, T, n, S, eps, samples, lengths, workspace, stream);
}

// svae_lds_ragged_perstep_inference_f64 with keep_vjp: the E-step keeps the factor region and the cross moments W~_t (its
// KEEPW instantiation), then the ragged sampler runs when S > 0 -- the records svae_lds_ragged_perstep_vjp_f64 reads
extern "C" int svae_lds_ragged_perstep_inference_keep_f64(int B, int T, int n, int S, int pair_batched, int init_batched,
                                                          int keep_vjp, unsigned options,
                                                          const double* init_J, const double* init_h, const double* init_logZ,
                                                          const double* J11, const double* J12, const double* J22,
                                                          const double* logZ_pair,
                                                          const double* node_J, const double* node_h, const double* node_logZ,
                                                          const int32_t* lengths, const double* eps, double* samples,
                                                          double* lognorm, double* E_init, double* E_pair,
                                                          double* E_node_diagxx, double* E_node_x,
                                                          int32_t* info, void* workspace, size_t ws_bytes, void* stream) {
  if (n < 1 || n > SVAE_LDS_MAX_N) return -3;
  if (S < 0 || (S > 0 && (!eps || !samples))) return -4;
  if (keep_vjp != 0 && keep_vjp != 1) return -23;
  const int rc = ragged_perstep_estep(B, T, n, pair_batched, init_batched, keep_vjp ? 3 : (S > 0 ? 1 : 0), 3, options, init_J,
                                      init_h, init_logZ, J11, J12, J22, logZ_pair, node_J, node_h, node_logZ, lengths, lognorm,
                                      E_init, E_pair, E_node_diagxx, E_node_x, info, workspace, ws_bytes, stream);
  if (rc != 0 || S == 0 || B == 0) return rc;
  return ragged_sample(B, T, n, S, eps, samples, lengths, workspace, stream);
}

// the packed ragged sweeps on the records of svae_lds_ragged_perstep_inference_keep_f64(keep_vjp = 1): J12 is the caller's
// per-step array, the zero block of the tail's pairs is the one the forward pass left behind the workspace
extern "C" int svae_lds_ragged_perstep_vjp_f64(int B, int T, int n, int S, int pair_batched, unsigned options,
                                               const double* J12, const double* g_lognorm,
                                               const double* g_E_node_diagxx, const double* g_E_node_x,
                                               const double* g_E_init, const double* g_E_pair,
                                               const double* g_samples, const double* eps, const double* samples,
                                               const double* E_pair, const double* E_node_x,
                                               const int32_t* lengths, double* g_node_J, double* g_node_h,
                                               const void* workspace, size_t ws_bytes,
                                               void* vjp_workspace, size_t vjp_ws_bytes, void* stream) {
  if (B < 0) return -1;
  if (T < 1) return -2;
  if (n < 1 || n > SVAE_LDS_MAX_N) return -3;
  if ((pair_batched & ~1) != 0) return -32;
  if (!lengths) return -31;
  if (g_samples && (S < 1 || S > 16)) return -4;
  if (T > 1 && !J12) return -5;
  if (!g_lognorm) return -6;
  if (g_E_pair && (!E_pair || !E_node_x)) return -8;      /* S~_{t+1} is read back from the forward outputs */
  if (g_samples && (!eps || !samples)) return -10;
  if (!g_node_J) return -12;
  if (!g_node_h) return -13;
  Selection sel;
  if (!decode_options(options, B, &sel)) return -24;
  if (B == 0) return 0;
  if (!workspace || ws_bytes < svae_lds_ragged_perstep_workspace_bytes(B, T, n)) return -14;
  if (!vjp_workspace || vjp_ws_bytes < svae_lds_vjp_workspace_bytes(B, T, n)) return -16;
  svae::VjpPerstepArgs a{};
  static_cast<svae::VjpArgs&>(a) = vjp_args(B, T, n, S, 0, g_lognorm, g_E_node_diagxx, g_E_node_x, g_samples, eps, samples,
                                            g_node_J, g_node_h, workspace, vjp_workspace);
  a.J12 = J12;
  a.pair_t_stride = (long)n * n;
  a.pair_seq_stride = pair_batched ? (long)(T - 1) * n * n : 0;
  a.g_E_init = g_E_init; a.g_E_pair = T > 1 ? g_E_pair : nullptr; a.E_pair = E_pair; a.E_node_x = E_node_x;
  a.lengths = lengths;
  a.qzero = (const double*)((const char*)workspace + ragged_table_offset_bytes(B, T, n));   /* [0 | -1/2 I], left by the forward pass */
  return vjp_units[n]->vjp_ragged_perstep(a, stream);
}

extern "C" int svae_lds_ragged_vjp_f64(int B, int T, int n, int S, int inhomog, int pair_batched, unsigned options,
                                       const double* g_lognorm, const double* g_E_node_diagxx, const double* g_E_node_x,
                                       const double* g_samples, const double* eps, const double* samples,
                                       const int32_t* lengths, double* g_node_J, double* g_node_h,
                                       const void* workspace, size_t ws_bytes,
                                       void* vjp_workspace, size_t vjp_ws_bytes, void* stream) {
  if (B < 0) return -1;
  if (T < 1) return -2;
  if (n < 1 || n > SVAE_LDS_MAX_N) return -3;
  if (inhomog || pair_batched) return -32;
  if (!lengths) return -31;
  if (g_samples && (S < 1 || S > 16)) return -4;
  if (!g_lognorm) return -6;
  if (g_samples && (!eps || !samples)) return -10;
  if (!g_node_J) return -12;
  if (!g_node_h) return -13;
  Selection sel;
  if (!decode_options(options, B, &sel)) return -24;
  if (B == 0) return 0;
  if (!workspace || ws_bytes < svae_lds_ragged_workspace_bytes(B, T, n)) return -14;
  if (!vjp_workspace || vjp_ws_bytes < svae_lds_vjp_workspace_bytes(B, T, n)) return -16;
  const long nn = (long)n * n;
  svae::VjpArgs a = vjp_args(B, T, n, S, 0, g_lognorm, g_E_node_diagxx, g_E_node_x, g_samples, eps, samples, g_node_J, g_node_h,
                             workspace, vjp_workspace);
  a.J12 = (const double*)((const char*)workspace + ragged_table_offset_bytes(B, T, n)) + 2 * nn;   /* [real | 0], left by the forward pass */
  a.lengths = lengths;
  return vjp_units[n]->vjp_ragged(a, stream);
}

// [sum E_init | sum E_pair | sum lognorm | B | sum_b (lengths[b] - 1)]: the uniform layout with one more slot, the number
// of pairs behind the E_pair sums (what the uniform consumers derive as count (T-1))
extern "C" int svae_lds_ragged_reduce_stats_f64(int B, int T, int n, const double* E_init, const double* E_pair,
                                                const double* lognorm, const int32_t* lengths, double* out, void* stream) {
  if (B < 0) return -1;
  if (T < 1) return -7;
  if (n < 1 || n > SVAE_LDS_MAX_N) return -2;
  if (!E_init) return -3;
  if (!E_pair) return -4;
  if (!lognorm) return -5;
  if (!lengths) return -31;
  if (!out) return -6;
  launch_reduce_stats(B, n, E_init, E_pair, lognorm, out, stream);
  hipLaunchKernelGGL(svae::lds_ragged_pair_count_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, B, T, lengths,
                     out + 4 * n * n + n + 2);
  return hipGetLastError() == hipSuccess ? 0 : -1000;
}
