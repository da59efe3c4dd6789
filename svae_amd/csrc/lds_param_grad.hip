// lds_param_grad.hip -- cotangents of the LDS natural parameters (init_J, init_h, init_logZ, J11, J12, J22, logZ_pair)
// from what the packed second VJP sweep leaves per (sequence, step) (lds_vjp_kernel.hpp, PGR instantiations):
//   g_P (B,T,n,n)      -2 Pbar_t                                    J11_t, J22_{t-1} and init_J enter P_t alone:
//                                                                   g_J11_t = g_P[t], g_J22_t = g_P[t+1], g_init_J = g_P[0]
//   g_R (B,T-1,2,n,n)  [Bbar_t[:, :n] | [Abar | hbar]_{t+1} H_t']   Rbar_t = first - second';  g_J12_t = -Rbar_t
//   g_node_h (B,T,n)   hfbar_t                                      g_init_h = hfbar_0
//   g_lognorm (B)                                                   g_init_logZ = g_logZ_pair_t = g_lognorm
// summed over whatever the parameter is shared over: the batch (init, (T-1,n,n) pair parameters), the batch and time
// (homogeneous pair parameters), nothing ((B,T-1,n,n): a re-layout).  g_J11 / g_J22 / g_init_J come out SYMMETRISED (the
// forward pass reads P_t as a symmetric matrix); g_J12 is a full matrix.
// Every output entry is one thread group's sum in a fixed order -- no atomics, the same bits on every run: a workgroup
// owns 16 consecutive entries of a parameter block (the lanes of a quarter wavefront read one 128-byte piece of a
// sequence's block); its 16 chunks take the terms r = chunk, chunk + 16, .. in four interleaved partial sums and meet in
// LDS in a fixed tree.  Homogeneous pair parameters take two passes -- the batch sums per step into scratch, then the sum
// over time -- so that the first pass has (T-1) n^2 / 16 workgroups instead of n^2 / 16.
#include <hip/hip_runtime.h>

#include "lds_args.hpp"

namespace svae {

struct ParamGradArgs {
  int B, T, n;
  int inhomog, pair_batched;
  const double* __restrict__ g_P;
  const double* __restrict__ g_R;
  const double* __restrict__ g_node_h;
  const double* __restrict__ g_lognorm;
  double* __restrict__ part;          // homogeneous: (T-1,3,n*n) per-step batch sums
  double* g_init_J;                   // outputs, any of them nullptr
  double* g_init_h;
  double* g_init_logZ;
  double* g_J11;
  double* g_J12;
  double* g_J22;
  double* g_logZ_pair;
};

// sum of the 16 chunks' partial sums of entry `e` (fixed tree); valid in chunk 0
__device__ __forceinline__ double chunk_sum(double* red, int e, int ch, double v) {
  red[ch * 16 + e] = v;
  __syncthreads();
  double s = 0.0;
  if (ch == 0) {
    double q[4];
#pragma unroll
    for (int k = 0; k < 4; ++k)
      q[k] = (red[(4 * k) * 16 + e] + red[(4 * k + 1) * 16 + e]) + (red[(4 * k + 2) * 16 + e] + red[(4 * k + 3) * 16 + e]);
    s = (q[0] + q[1]) + (q[2] + q[3]);
  }
  __syncthreads();
  return s;
}

// Pair parameters, pass over the batch.  grid (ceil(n^2 / 16), G): G = B (T-1) blocks per-sequence ((B,T-1,n,n): one term
// each) or T-1 (sum over the batch: the per-step outputs, or `part` for homogeneous parameters).
__global__ __launch_bounds__(256) void lds_param_grad_pair_kernel(const ParamGradArgs a) {
  __shared__ double red[3][256];
  const int n = a.n, nn = n * n, T = a.T, B = a.B;
  const int el = threadIdx.x & 15, ch = threadIdx.x >> 4;
  const int e = blockIdx.x * 16 + el;
  const bool live = e < nn;
  const int i = live ? e / n : 0, j = live ? e - i * n : 0;
  const int et = j * n + i;                                   // the transposed entry
  const int g = blockIdx.y;
  const bool per_seq = a.pair_batched != 0;
  const int t = per_seq ? g % (T - 1) : g;
  const int b0 = per_seq ? g / (T - 1) : ch;
  const int bstep = per_seq ? B : 16;                         // (per-sequence blocks: chunk 0 alone has a term)
  double s11[4] = {0.0, 0.0, 0.0, 0.0}, s12[4] = {0.0, 0.0, 0.0, 0.0}, s22[4] = {0.0, 0.0, 0.0, 0.0};
  if (live && !(per_seq && ch != 0)) {
    int u = 0;
    for (int b = b0; b < B; b += bstep, ++u) {
      const double* p0 = a.g_P + ((long)b * T + t) * nn;
      const double* p1 = p0 + nn;
      const double* r = a.g_R + ((long)b * (T - 1) + t) * 2 * nn;
      s11[u & 3] += 0.5 * (p0[e] + p0[et]);
      s22[u & 3] += 0.5 * (p1[e] + p1[et]);
      s12[u & 3] += r[nn + et] - r[e];
    }
  }
  const double v11 = chunk_sum(red[0], el, ch, (s11[0] + s11[1]) + (s11[2] + s11[3]));
  const double v12 = chunk_sum(red[1], el, ch, (s12[0] + s12[1]) + (s12[2] + s12[3]));
  const double v22 = chunk_sum(red[2], el, ch, (s22[0] + s22[1]) + (s22[2] + s22[3]));
  if (ch == 0 && live) {
    if (!a.inhomog) {
      double* o = a.part + (long)g * 3 * nn;
      o[e] = v11; o[nn + e] = v12; o[2 * nn + e] = v22;
    } else {
      if (a.g_J11) a.g_J11[(long)g * nn + e] = v11;
      if (a.g_J12) a.g_J12[(long)g * nn + e] = v12;
      if (a.g_J22) a.g_J22[(long)g * nn + e] = v22;
    }
  }
  if (per_seq && a.g_logZ_pair && blockIdx.x == 0 && threadIdx.x == 0) a.g_logZ_pair[g] = a.g_lognorm[g / (T - 1)];
}

// Homogeneous pair parameters, pass over time: grid (ceil(3 n^2 / 16)); entry e of [g_J11 | g_J12 | g_J22] = sum_t part[t][e]
// (T = 1: no terms, exact zeros)
__global__ __launch_bounds__(256) void lds_param_grad_time_kernel(const ParamGradArgs a) {
  __shared__ double red[256];
  const int nn = a.n * a.n, tot = 3 * nn;
  const int el = threadIdx.x & 15, ch = threadIdx.x >> 4;
  const int e = blockIdx.x * 16 + el;
  double s[4] = {0.0, 0.0, 0.0, 0.0};
  if (e < tot) {
    int u = 0;
    for (int t = ch; t < a.T - 1; t += 16, ++u) s[u & 3] += a.part[(long)t * tot + e];
  }
  const double v = chunk_sum(red, el, ch, (s[0] + s[1]) + (s[2] + s[3]));
  if (ch == 0 && e < tot) {
    double* o = e < nn ? a.g_J11 : (e < 2 * nn ? a.g_J12 : a.g_J22);
    if (o) o[e % nn] = v;
  }
}

// Initial parameters and the log-normaliser terms: entries [g_init_J (n^2) | g_init_h (n) | sum_b g_lognorm], summed over
// the batch; the workgroup that holds the last entry also writes g_init_logZ and the shared forms of g_logZ_pair
// ((T-1) x the sum for homogeneous parameters, the sum at every step for (T-1,n,n) ones).
__global__ __launch_bounds__(256) void lds_param_grad_init_kernel(const ParamGradArgs a) {
  __shared__ double red[256];
  __shared__ double gsum;
  const int n = a.n, nn = n * n, T = a.T, B = a.B, tot = nn + n + 1;
  const int el = threadIdx.x & 15, ch = threadIdx.x >> 4;
  const int e = blockIdx.x * 16 + el;
  double s[4] = {0.0, 0.0, 0.0, 0.0};
  if (e < tot) {
    int u = 0;
    if (e < nn) {
      const int i = e / n, j = e - i * n, et = j * n + i;
      for (int b = ch; b < B; b += 16, ++u) {
        const double* p0 = a.g_P + (long)b * T * nn;
        s[u & 3] += 0.5 * (p0[e] + p0[et]);
      }
    } else if (e < nn + n) {
      for (int b = ch; b < B; b += 16, ++u) s[u & 3] += a.g_node_h[(long)b * T * n + (e - nn)];
    } else {
      for (int b = ch; b < B; b += 16, ++u) s[u & 3] += a.g_lognorm[b];
    }
  }
  const double v = chunk_sum(red, el, ch, (s[0] + s[1]) + (s[2] + s[3]));
  if (ch == 0 && e < tot) {
    if (e < nn) { if (a.g_init_J) a.g_init_J[e] = v; }
    else if (e < nn + n) { if (a.g_init_h) a.g_init_h[e - nn] = v; }
    else {
      if (a.g_init_logZ) a.g_init_logZ[0] = v;
      gsum = v;
    }
  }
  __syncthreads();
  if (blockIdx.x == (tot - 1) / 16 && a.g_logZ_pair && !a.pair_batched) {
    if (!a.inhomog) { if (threadIdx.x == 0) a.g_logZ_pair[0] = (double)(T - 1) * gsum; }
    else for (int t = threadIdx.x; t < T - 1; t += 256) a.g_logZ_pair[t] = gsum;
  }
}

}  // namespace svae

extern "C" int svae_lds_param_grad_launch(int B, int T, int n, int inhomog, int pair_batched, const double* g_P,
                                          const double* g_R, const double* g_node_h, const double* g_lognorm, double* part,
                                          double* g_init_J, double* g_init_h, double* g_init_logZ, double* g_J11,
                                          double* g_J12, double* g_J22, double* g_logZ_pair, void* stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  svae::ParamGradArgs a;
  a.B = B; a.T = T; a.n = n; a.inhomog = inhomog; a.pair_batched = pair_batched;
  a.g_P = g_P; a.g_R = g_R; a.g_node_h = g_node_h; a.g_lognorm = g_lognorm; a.part = part;
  a.g_init_J = g_init_J; a.g_init_h = g_init_h; a.g_init_logZ = g_init_logZ;
  a.g_J11 = g_J11; a.g_J12 = g_J12; a.g_J22 = g_J22; a.g_logZ_pair = g_logZ_pair;
  const int nn = n * n;
  if (g_init_J || g_init_h || g_init_logZ || (g_logZ_pair && !pair_batched))
    hipLaunchKernelGGL(svae::lds_param_grad_init_kernel, dim3((nn + n + 1 + 15) / 16), dim3(256), 0, stream, a);
  const bool pairs = g_J11 || g_J12 || g_J22;
  if (T > 1 && (pairs || (pair_batched && g_logZ_pair))) {
    const long G = pair_batched ? (long)B * (T - 1) : T - 1;
    if (G > 65535) {
      // (grid.y is 16 bits wide: the per-sequence re-layout goes in slabs of whole sequences)
      const int seqs = 65535 / (T - 1);
      if (!pair_batched || seqs < 1) return -1003;         // (T > 65536: refused by the caller)
      for (int b0 = 0; b0 < B; b0 += seqs) {
        svae::ParamGradArgs s = a;
        const int nb = B - b0 < seqs ? B - b0 : seqs;
        s.B = nb;
        s.g_P = g_P + (long)b0 * T * nn; s.g_R = g_R + (long)b0 * (T - 1) * 2 * nn; s.g_lognorm = g_lognorm + b0;
        const long off = (long)b0 * (T - 1);
        s.g_J11 = g_J11 ? g_J11 + off * nn : nullptr; s.g_J12 = g_J12 ? g_J12 + off * nn : nullptr;
        s.g_J22 = g_J22 ? g_J22 + off * nn : nullptr; s.g_logZ_pair = g_logZ_pair ? g_logZ_pair + off : nullptr;
        hipLaunchKernelGGL(svae::lds_param_grad_pair_kernel, dim3((nn + 15) / 16, nb * (T - 1)), dim3(256), 0, stream, s);
      }
    } else {
      hipLaunchKernelGGL(svae::lds_param_grad_pair_kernel, dim3((nn + 15) / 16, (unsigned)G), dim3(256), 0, stream, a);
    }
  }
  if (!inhomog && pairs)
    hipLaunchKernelGGL(svae::lds_param_grad_time_kernel, dim3((3 * nn + 15) / 16), dim3(256), 0, stream, a);
  return hipGetLastError() == hipSuccess ? 0 : -1000;
}
