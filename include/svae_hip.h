/* svae_hip.h -- C ABI of libsvae_hip.so: the MI355X (gfx950) structured E-step of mattjj/svae.
 *
 * Every entry point replaces one function at the reference's Python->Cython boundary
 * (/root/reference/svae/lds/lds_inference.py:18-24; svae/hmm/hmm_inference.py:11-13) or one hot loop
 * of svae/models/gmm.py, batched over independent sequences / data points.  Plain pointers and sizes only; no torch types.
 *
 * Conventions (identical to the reference's API level):
 *   - all arrays are float64, C-order, time-major, and hold NATURAL parameters:
 *       Gaussian potentials are (-1/2 J, h); pair potentials are
 *       (J11 = -1/2 A'Q^-1 A, J12 = A'Q^-1, J22 = -1/2 Q^-1, logZ)        [gaussian.py:130-143]
 *   - every pointer is a DEVICE pointer owned by the caller; calls are asynchronous on `stream`
 *     (a hipStream_t, passed as void*); nothing is allocated internally.
 *   - return value: 0 = launched, <0 = bad argument number -k (nothing launched).
 *   - numerical failures (non-positive pivot = potentials not positive definite; the reference
 *     silently ignores LAPACK `info`, cython_gaussian_grads.pxd:54-76) are reported through the
 *     device-side `info` word: 0 = ok, k>0 = 1 + index of the first offending sequence/point.
 */
#ifndef SVAE_HIP_H
#define SVAE_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SVAE_HIP_ABI_VERSION 15   /* 15: (+ svae_lds_ragged_perstep_inference_keep_f64, svae_lds_ragged_perstep_vjp_f64: the forward records and the reverse sweeps of the per-step ragged LDS, added without a new number -- additions only) (+ svae_hmm_estep_vjp_workspace_bytes, svae_hmm_estep_vjp_f64, svae_hmm_ragged_estep_vjp_f64: the reverse-mode derivative of the HMM E-step, uniform and with per-sequence lengths, added without a new number -- additions only) (+ svae_hmm_sample_workspace_bytes, svae_hmm_sample_f64, svae_hmm_ragged_sample_f64: HMM posterior sampling, uniform and with per-sequence lengths, added without a new number -- additions only) (+ svae_lds_ragged_perstep_workspace_bytes, svae_lds_ragged_perstep_estep_f64, svae_lds_ragged_perstep_inference_f64: per-sequence lengths with per-step pair parameters and a per-sequence init potential, added without a new number -- additions only) (+ svae_hmm_ragged_estep_f64, svae_hmm_ragged_viterbi_f64: per-sequence lengths for the HMM E-step and Viterbi, added without a new number -- additions only, compatible with every caller of 15) (+ svae_lds_estep_vjp_params_f64, svae_lds_param_vjp_workspace_bytes: cotangents of the init / pair natural parameters, added without a new number -- additions only) + svae_gmm_wide_mw_workspace_bytes, svae_gmm_wide_mw_begin, svae_gmm_wide_mw_step_f64, svae_gmm_wide_sample_f64, svae_gmm_wide_local_vjp_f64, svae_gmm_wide_global_step_f64 (the GMM local step for N <= 16; additions only), svae_lds_filter_vjp_f64, svae_lds_smoother_vjp_f64 (+ svae_lds_smoother_vjp_workspace_bytes), svae_lds_sample_vjp_f64 (the reference's three reverse-mode primitives on caller-held forward messages); 14: + svae_lds_estep_vjp_dense_f64 (cotangent of dense node potentials), svae_hmm_* up to K = 64, svae_lds_inference_f64 (E-step + sampler in one call; lean per-step records for large homogeneous batches), svae_lds_inference_is_lean, SVAE_OPT_LEAN_ON / _OFF / SVAE_OPT_INFER_RECORDS; 13: + svae_slds_pair_contract_f64 (the two contractions of the SLDS final pass over the per-step pair statistics in one pass); 12: svae_gmm_global_step_f64 writes kl[0..1] (as spelled | as shipped), svae_ipc_allreduce_f64 takes the mailbox stride and never writes `out` on a timeout, + svae_slds_lds_meanfield options; 11: + svae_lds_global_step_multi_f64 (K parameter sets in one launch: the SLDS global -> local maps), svae_lds_diag_sample_f64 (filter + sampler of an all-diagonal LDS: the SLDS initial path); 10: + svae_ipc_allreduce_f64 / svae_ipc_mailbox_bytes, svae_gmm_sample_f64, svae_gmm_local_vjp_f64, svae_gmm_global_step_f64 (the differentiable tail and the global side of the GMM local step); 9: keep bit SVAE_KEEP_SIGMA of svae_lds_estep_f64 (16 <= n <= 64) + svae_lds_tile_sigma_offset_bytes; 8: step ranges (t_begin, t_end) in svae_lds_tile_vjp_f64 / svae_lds_tile_noise_f64, SVAE_OPT_TILE_FORWARD / _BACKWARD; 7: + svae_slds_path_nodeparams_f64, svae_slds_mix_pair_natparam_f64; 6: per-call `options` word replaces the process-global svae_lds_set_* selectors (re-entrant library), + svae_slds_hmm_meanfield_f64, svae_slds_sweep_glue_f64, g_E_pair in svae_lds_tile_vjp_f64; 5: + svae_lds_set_prod_max_b; 4: + svae_slds_lds_meanfield_f64, svae_gmm_mw_*, svae_lds_global_step_f64, svae_lds_natgrad_f64, svae_lds_tile_vjp_f64; 2: + svae_lds_workspace_bytes_ex, svae_lds_estep_vjp_ex_f64, svae_hmm_*, tiled path (n <= 64) */
#define SVAE_HMM_MAX_K 64   /* svae_hmm_estep_f64 / svae_slds_hmm_meanfield_f64: K <= 16 one DPP row per sequence; 17 <= K <= 64 one wavefront per sequence (round 6) */
#define SVAE_LDS_MAX_N 15   /* register/DPP path: one 16-lane row per sequence, n+1 <= 16 */
#define SVAE_LDS_TILE_MAX_N 64   /* 16 <= n <= 64: LDS-tiled MFMA path (keep: SVAE_KEEP_SIGMA or 0) */
#define SVAE_LDS_XL_MAX_N 128   /* 65 <= n <= 128: register-panel MFMA path, svae_lds_xl_* (E-step only) */
#define SVAE_KEEP_SIGMA 4         /* keep bit of svae_lds_estep_f64, 16 <= n <= 64 only: see svae_lds_tile_sigma_offset_bytes */

/* Library/ABI version (host only, no GPU needed). */
int svae_hip_abi_version(void);

/* Bytes of scratch `svae_lds_estep_f64` / `svae_lds_sample_f64` need for (B, T, n): the per-step
 * backward kernels (G_t, c_t, P_t^-1: (2n+1)n doubles) written by the forward filter, followed by
 * the factor region (unit LDL' factor + pivots of P_t: n*n+n doubles) the sampler reads and the
 * cross-moment region (W~_t) the VJP reads. */
size_t svae_lds_workspace_bytes(int B, int T, int n);

/* Same, exact for the tiled path (n > SVAE_LDS_MAX_N), whose workspace also holds the pair
 * parameters re-packed in MFMA fragment order: 2 slots when they are homogeneous (what
 * svae_lds_workspace_bytes assumes), T-1 slots per parameter set when they are per-step
 * (`inhomog`), one set per sequence when `pair_batched`.  Equal to svae_lds_workspace_bytes for
 * n <= SVAE_LDS_MAX_N. */
size_t svae_lds_workspace_bytes_ex(int B, int T, int n, int inhomog, int pair_batched);
/* 16 <= n <= 64, keep & SVAE_KEEP_SIGMA: the backward half of the E-step also leaves the smoothed covariances
 * Sigma_t = Cov(x_t | y) as a compact (B,T,n,n) array at THIS byte offset of the workspace (svae_lds_workspace_bytes_ex
 * rounded up to 256), which must then be at least offset + B T n n 8 bytes long.  That array is the first section of the
 * workspace of svae_lds_tile_vjp_f64: a caller that lets its VJP workspace START at workspace + offset (one allocation
 * of offset + 8 svae_lds_tile_vjp_workspace_doubles(..) bytes) skips phase 0 of the VJP, which would rebuild the same
 * matrices from the hand-off.  0 for n <= 15. */
size_t svae_lds_tile_sigma_offset_bytes(int B, int T, int n, int inhomog, int pair_batched);

/* Batched LDS E-step = filter + RTS smoother + expected sufficient statistics + log-normalizer.
 *
 * Replaces, for B independent sequences sharing (init, pair) parameters,
 *   cython_natural_lds_estep_general(natparam, node_params) -> (lognorm, expected_stats)
 *     /root/reference/svae/lds/lds_inference.py:232-237, i.e.
 *   natural_filter_forward_general  /root/reference/svae/lds/cython_lds_inference.pyx:28-90
 *   natural_smoother_general        /root/reference/svae/lds/cython_lds_inference.pyx:149-195
 *   _compute_stats                  /root/reference/svae/lds/cython_lds_inference.pyx:197-210
 *
 *  in : init_J (n,n), init_h (n), init_logZ (1)           = init_params (sum of trailing logZ terms)
 *       J11, J12, J22: (n,n) if !inhomog, else (T-1,n,n) per sequence-independent step;
 *       logZ_pair: (1) if !inhomog else (T-1)
 *       pair_batched != 0 (inhomog only): J11/J12/J22 are (B,T-1,n,n), logZ_pair (B,T-1)
 *         (the SLDS case, slds_svae.py:92-103, where pair params depend on each sequence's
 *          discrete-state marginals)
 *       keep: bit 0 = also write the factor region of the workspace so that svae_lds_sample_f64 can
 *         follow; bit 1 = also write the cross-moment region so that svae_lds_estep_vjp_f64 can
 *         follow (each costs a few % of the E-step); 16 <= n <= 64: SVAE_KEEP_SIGMA or 0
 *       node_J (B,T,n) diagonal of -1/2 precision, node_h (B,T,n), node_logZ (B,T) or NULL (=0)
 *  out: lognorm (B)
 *       E_init  (B, n*n + n)      = [E[x0 x0'] (n,n) | E[x0] (n)]   (the two trailing 1's of the
 *                                    reference tuple are implied)
 *       E_pair  (B, 3, n, n)      = [sum_t E[x_t x_t'], sum_t E[x_t x_{t+1}'], sum_t E[x_{t+1}x_{t+1}']]
 *                                    t = 0..T-2 (4th entry of the reference tuple is T-1)
 *                                    if inhomog: (B, T-1, 3, n, n) per-step blocks (no sum)
 *       E_node_diagxx (B,T,n) = diag E[x_t x_t'],   E_node_x (B,T,n) = E[x_t]
 *       info (1) int32, must be zeroed by the caller (or by a previous successful call)
 */
int svae_lds_estep_f64(int B, int T, int n, int inhomog, int pair_batched, int keep, unsigned options,
                       const double* init_J, const double* init_h, const double* init_logZ,
                       const double* J11, const double* J12, const double* J22,
                       const double* logZ_pair,
                       const double* node_J, const double* node_h, const double* node_logZ,
                       double* lognorm, double* E_init, double* E_pair,
                       double* E_node_diagxx, double* E_node_x,
                       int32_t* info, void* workspace, size_t ws_bytes, void* stream);

/* Filter only = natural_filter_forward_general (/root/reference/svae/lds/cython_lds_inference.pyx:28-90),
 * the first of the six functions the reference imports at lds_inference.py:18-24, batched.  Same inputs as
 * svae_lds_estep_f64 (n <= SVAE_LDS_MAX_N).
 *  out: lognorm (B); the forward messages in the reference's scaling (natural parameters, :84-85), each
 *       optional (NULL = not wanted):  J_pred, J_filt (B,T,n,n) = -1/2 precision,  h_pred, h_filt (B,T,n).
 * The workspace afterwards holds what svae_lds_sample_f64 needs: filter + sampler without the smoother is
 * cython_natural_lds_sample (lds_inference.py:260-264). */
int svae_lds_filter_f64(int B, int T, int n, int inhomog, int pair_batched, unsigned options,
                        const double* init_J, const double* init_h, const double* init_logZ,
                        const double* J11, const double* J12, const double* J22, const double* logZ_pair,
                        const double* node_J, const double* node_h, const double* node_logZ,
                        double* lognorm, double* J_pred, double* h_pred, double* J_filt, double* h_filt,
                        int32_t* info, void* workspace, size_t ws_bytes, void* stream);

/* `options` word of svae_lds_estep_f64 / svae_lds_filter_f64 / svae_lds_sample_f64 / svae_lds_estep_vjp_ex_f64
 * (n <= SVAE_LDS_MAX_N; ignored above).  0 = the library's own choice; the bits force one of the kernel variants --
 * all give the same results up to rounding -- for A/B measurements and for the tests that run every kernel.  The
 * library keeps NO process-global selection state and reads no environment variables: two host threads / streams /
 * devices may use different options at the same time.
 *
 * Default dispatch of svae_lds_estep_f64: with keep == 0, n <= 10 and T >= 4 the two-ended kernel (block elimination
 * from both ends of the chain, meeting in the middle: half the serial depth; lean hand-off record) -- up to 512
 * sequences one sequence per workgroup (shortest instruction stream per sequence), above two sequences per wavefront
 * (fewest instructions per sequence).  With keep != 0,
 * n <= 10, T >= 4 and B <= 1023 the call runs TWO kernels side by side, joined by events before it returns to the
 * caller's stream: the two-ended E-step (statistics, log-normaliser, and the cross moments the VJP reads) and the
 * one-directional filter (hand-off records and LDL' factors for svae_lds_sample_f64 / svae_lds_estep_vjp_f64); the
 * helper stream and the two events are created once per (device, caller stream).  Otherwise batches with B <= 1023
 * run the one-directional small-batch variant (one sequence per wavefront, product stages split across the four DPP
 * rows), larger ones the packed kernel (four sequences per wavefront).
 * svae_lds_sample_f64 (S <= 4) and the sweeps of svae_lds_estep_vjp_f64 run, for batches B <= 1024, with PRODUCER
 * wavefronts: the serial loop of a workgroup's sequences reads its per-step records from an LDS ring that more
 * wavefronts of the workgroup fill several steps ahead (and, in the first sweep, HELPER wavefronts take the work that
 * does not feed the recursion); larger batches hide the latency by occupancy instead. */
#define SVAE_OPT_DEFAULT        0x00u
#define SVAE_OPT_TWOEND_OFF     0x01u   /* never the two-ended kernel (one-directional kernels only) */
#define SVAE_OPT_TWOEND_FULL    0x02u   /* two-ended kernel with the full hand-off record (no lean record) */
#define SVAE_OPT_LAYOUT_SPLIT   0x04u   /* one sequence per wavefront whatever B */
#define SVAE_OPT_LAYOUT_PACKED  0x08u   /* several sequences per wavefront whatever B (two-ended kernel: two, one DPP row
                                           per elimination chain; one-directional kernels: four) */
#define SVAE_OPT_PRODUCERS_ON   0x10u   /* producer / helper wavefronts whatever B */
#define SVAE_OPT_PRODUCERS_OFF  0x20u   /* never */
#define SVAE_OPT_ALL            0x3fu   /* (contradictory pairs or unknown bits: the call returns -24) */
/* Record format of svae_lds_inference_f64 (below); accepted and ignored by the other entry points, so that a caller can
 * pass one word with every call of a plan. */
#define SVAE_OPT_LEAN_ON        0x100u  /* lean per-step records whatever B (where they apply: see svae_lds_inference_f64) */
#define SVAE_OPT_LEAN_OFF       0x200u  /* never */
#define SVAE_OPT_INFER_RECORDS  0x400u  /* svae_lds_estep_vjp_ex_f64 only: `workspace` was written by svae_lds_inference_f64 */
/* svae_lds_estep_f64 with 16 <= n <= 64 only (any other use: -24): run HALF of the E-step.  The forward half (filter,
 * hand-off, log-normaliser) and the backward half (smoother + statistics, from the hand-off a forward-only call left
 * in the same workspace) meet only through the hand-off, so a training step can run the backward half on one stream
 * NEXT to the kernels that need the hand-off alone (svae_lds_tile_noise_f64 + svae_lds_tile_sample_f64, phase 0 of
 * svae_lds_tile_vjp_f64) on others -- each is one workgroup per sequence or shorter than the smoother. */
#define SVAE_OPT_TILE_FORWARD   0x40u
#define SVAE_OPT_TILE_BACKWARD  0x80u

/* LDS mean-field step of the SLDS-SVAE coordinate ascent with the mixing of the K per-state parameter sets
 * and the contraction of the pair statistics FUSED into the E-step:
 *   lds_meanfield + get_var_lds_local_natparam  /root/reference/svae/models/slds_svae.py:80-103
 *   the pair part of get_arhmm_local_nodeparams /root/reference/svae/models/slds_svae.py:131-147
 * For sequence b the LDS has init potential sum_k w[b,0,k] (init_J_k, init_h_k) and, at step t, pair
 * parameters sum_k w[b,t+1,k] (J11_k, J12_k, J22_k) -- never materialised: the K sets sit in LDS, w streams.
 *  in : init_J (K,n,n), init_h (K,n), J11/J12/J22 (K,n,n) natural parameters per discrete state;
 *       weights (rows,T,K) = E[z_t = k]; node potentials (rows,T,n) as in svae_lds_estep_f64;
 *       seq_index (B) int32 or NULL: the launch processes B <= rows sequences, slot i working on row
 *       seq_index[i] of every array and of the workspace (NULL: row i); rows not listed are left untouched;
 *       a NEGATIVE entry marks an unused slot (skipped): a caller may launch on more slots than are live
 *       (converged sequences of the coordinate ascent are frozen, slds_svae.py:170-172: the caller lists the
 *       ones still iterating)
 *  out: lognorm (rows) WITHOUT the mixed constants sum_k w[b,0,k] init_logZ_k + sum_t sum_k w[b,t+1,k] logZ_k
 *       (a (B,T,K) x (K) product the caller adds); E_init, E_node_diagxx, E_node_x as in svae_lds_estep_f64;
 *       pair_contr (rows,T,2,K):  [b,t,0,k] = <E x_t x_t', J11_k> + <E x_t x_{t+1}', J12_k>   (t < T-1)
 *                              [b,t,1,k] = <E x_t x_t', J22_k>                              (t > 0)
 *         so that the HMM node potential of slds_svae.py:141-146 is
 *         node[b,t+1,k] = pair_contr[b,t,0,k] + pair_contr[b,t+1,1,k] + logZ_k
 *         (which of the two slots carries the cross term depends on the chain that owns node t; only the sum
 *          above is defined).
 * n <= 10, T >= 4, K <= 16 and svae_slds_lds_meanfield_lds_bytes(n, K) <= 160 KiB (else -4: use the
 * per-step entry point).  workspace: svae_slds_lds_meanfield_workspace_bytes(rows, T, n) (the two-ended kernel's
 * records only: a third of svae_lds_workspace_bytes).
 * options (ABI 12; 0 = the library's choice, a pure function of the arguments):
 *   SVAE_OPT_LAYOUT_PACKED  row-per-chain consumers (two sequences per wavefront, lean records) + producer wavefronts that
 *                           form the K-state mixing and the K-state contraction on v_mfma_f64_16x16x4, 8 sequences per
 *                           workgroup in lock-step (csrc/lds_estep_twoend_rpcmix.hpp): K <= 8 and a workspace below
 *                           4 GiB, else -24; the default where it applies;
 *   SVAE_OPT_LAYOUT_SPLIT   one sequence per wavefront, the K parameter sets as LDS tables (rounds 2 - 4; any K <= 16);
 *   SVAE_OPT_PRODUCERS_OFF  with the packed layout: the producers compute with plain loops instead of MFMA (slow; test
 *                           infrastructure that separates the lock-step protocol from the MFMA operand layouts). */
size_t svae_slds_lds_meanfield_lds_bytes(int n, int K);
size_t svae_slds_lds_meanfield_workspace_bytes(int rows, int T, int n);
int svae_slds_lds_meanfield_f64(int B, int rows, int T, int n, int K,
                                const double* init_J, const double* init_h,
                                const double* J11, const double* J12, const double* J22,
                                const double* weights,
                                const double* node_J, const double* node_h, const double* node_logZ,
                                const int32_t* seq_index,
                                double* lognorm, double* E_init, double* E_node_diagxx, double* E_node_x,
                                double* pair_contr, int32_t* info,
                                void* workspace, size_t ws_bytes, unsigned options, void* stream);

/* Reverse-mode derivative of the E-step (+ sampler) w.r.t. the node potentials for latent dimension 16 <= n <= 64,
 * on the hand-off the LDS-tiled E-step kernel leaves in `handoff_workspace` (the workspace of the LAST
 * svae_lds_estep_f64 call with this (B,T,n)): natural_filter_grad / natural_smoother_general_grad /
 * natural_sample_backward_grad, /root/reference/svae/lds/cython_lds_inference.pyx:92-145, 236-306, 357-409,
 * composed as /root/reference/svae/lds/lds_inference.py:26-39.  Three phases, one call each, in order:
 *   0: smoothed covariances (backward in time); 1: adjoint of the smoother / sampler recursions (forward in
 *   time); 2: adjoint of the filter (backward in time) -> g_node_J, g_node_h (B,T,n).
 * Between phases 1 and 2 the caller adds the Cholesky adjoint of the sampler's noise factor -- batched over all
 * (sequence, step) pairs, from `xbar` and eps -- into the `pinv_bar` section of `workspace`
 * (layout [sig (B,T,n,n) | pinv_bar (B,T,n,n) | g_bar (B,T-1,n,n) | c_bar (B,T,n) | xbar (B,T,S,n)],
 * svae_lds_tile_vjp_workspace_doubles); without sample cotangents (g_samples NULL) there is nothing to add.
 * Step ranges: phases 0 and 1 take (t_begin, t_end) = (0, T).  Phase 2 may be split into launches over
 * [t_begin, t_end), called from the LAST range down to the first (the recursion runs backward in time; its state
 * travels through the tail of `workspace`): a caller can then run the Cholesky adjoint of the next (earlier) range
 * (svae_lds_tile_noise_f64, mode 1, same range arguments) on another stream NEXT to phase 2 of the current one -- one
 * workgroup per sequence leaves most of the chip to it.  Bad ranges: -20.
 * Cotangents: g_lognorm (B); g_E_node_diagxx, g_E_node_x (B,T,n) or NULL; g_E_init (B, n*n+n) or NULL;
 * g_E_pair (B,T-1,3,n,n) or NULL: of the per-step pair statistics (inhomog only; _compute_stats_grad,
 * cython_lds_inference.pyx:212-234); g_samples (B,T,S,n) or NULL with the samples drawn (S <= 16).  J12 as in svae_lds_estep_vjp_ex_f64. */
size_t svae_lds_tile_vjp_workspace_doubles(int B, int T, int n, int S);
int svae_lds_tile_vjp_f64(int phase, int B, int T, int n, int S, int t_begin, int t_end, int inhomog, int pair_batched,
                          const double* J12, const double* g_lognorm, const double* g_E_node_diagxx,
                          const double* g_E_node_x, const double* g_E_init, const double* g_E_pair,
                          const double* g_samples,
                          const double* samples, const double* E_node_x, double* g_node_J, double* g_node_h,
                          const void* handoff_workspace, void* workspace, size_t ws_doubles, void* stream);

/* Backward sampling (natural_sample_backward, /root/reference/svae/lds/cython_lds_inference.pyx:310-355) for latent
 * dimension 16 <= n <= 64 from the hand-off of the tiled svae_lds_estep_f64: the serial recursion
 * x_t = c_t + noise_t + G_t x_{t+1}; `noise` (B,T,S,n) = chol(P_t)^-T eps_t is the caller's batched factorisation
 * of the hand-off's P_t^-1 (it does not depend on the recursion).  S <= 16. */
int svae_lds_tile_sample_f64(int B, int T, int n, int S, const double* noise, double* samples,
                             const void* handoff_workspace, void* stream);

/* The sampler's noise factor for latent dimension 16 <= n <= 64 and its adjoint, from the P_t^-1 of the tiled
 * E-step's hand-off, one workgroup per (sequence, step): the reference's noise map is chol(P_t)^-T eps_t
 * (/root/reference/svae/lds/cython_gaussian_grads.pxd:431-454), and chol(P_t)^-T is the upper-triangular M with
 * P_t^-1 = M M'.
 *   mode 0: noise (B,T,S,n) = M_t eps_t   (input of svae_lds_tile_sample_f64)
 *   mode 1: adds the Cholesky-path cotangent sym(M^-T Phi(M' Mbar) M^-1), Mbar = triu(sum_s xbar_s eps_s'), into the
 *           pinv_bar section of `vjp_workspace` -- between phases 1 and 2 of svae_lds_tile_vjp_f64
 *           (the adjoint of cython_gaussian_grads.pxd:456-487 `_natural_sample_grad`).           S <= 16.
 * Only the steps t_begin <= t < t_end of every sequence are processed ((0, T): all; bad ranges: -20). */
int svae_lds_tile_noise_f64(int mode, int B, int T, int n, int S, int t_begin, int t_end, const double* eps, double* noise,
                            const void* handoff_workspace, void* vjp_workspace, int32_t* info, void* stream);

/* The once-per-step GLOBAL side of the LDS-SVAE in one launch ("global->local maps
 * on device"): niw.expectedstats (/root/reference/svae/distributions/niw.py:15-25) and mniw.expectedstats
 * (/root/reference/svae/distributions/mniw.py:19-20, 33-55) of the global factors -> the LDS init and pair
 * potentials (svae/models/lds.py:23-25), and the prior KL of svae/models/lds.py:16-20 (with niw.logZ niw.py:27-31
 * and mniw.logZ mniw.py:13-17) against `prior_*` (all five NULL: no KL).
 *  in : niw (n+2,n+2) dense-packed NIW natural parameter; mniw_A, mniw_B, mniw_C (n,n), mniw_d (1)
 *  out: init_J (n,n) = -1/2 E[J], init_h (n) = E[h], init_logZ (1) = -1/2 E[h'J^-1 h] + 1/2 E[log|J|];
 *       J11, J12, J22 (n,n), logZ_pair (1) = the MNIW expected statistics;
 *       niw_expectedstats (n+2,n+2) dense-packed or NULL; global_kl (1) or NULL;
 *       info: 1 if an inversion met a non-positive pivot, kappa <= 0 or nu <= n - 1 of either factor (natural parameters
 *       outside the domain; the prior's likewise).   n <= 64. */
int svae_lds_global_step_f64(int n, const double* niw, const double* mniw_A, const double* mniw_B,
                             const double* mniw_C, const double* mniw_d,
                             const double* prior_niw, const double* prior_A, const double* prior_B,
                             const double* prior_C, const double* prior_d,
                             double* init_J, double* init_h, double* init_logZ,
                             double* J11, double* J12, double* J22, double* logZ_pair,
                             double* niw_expectedstats, double* global_kl, int32_t* info, void* stream);

/* The same maps for K parameter sets in ONE launch (the SLDS global -> local maps, get_all_lds_local_natparams,
 * /root/reference/svae/models/slds_svae.py:86-89: K factor pairs, no prior / KL): the five inputs are HOST arrays of K
 * device pointers (shapes as above), the outputs are stacked over the leading K axis -- init_J (K,n,n), init_h (K,n),
 * init_logZ (K), J11 / J12 / J22 (K,n,n), logZ_pair (K), niw_expectedstats (K,n+2,n+2) or NULL.   K <= 16. */
int svae_lds_global_step_multi_f64(int K, int n, const double* const* niw, const double* const* mniw_A,
                                   const double* const* mniw_B, const double* const* mniw_C,
                                   const double* const* mniw_d,
                                   double* init_J, double* init_h, double* init_logZ,
                                   double* J11, double* J12, double* J22, double* logZ_pair,
                                   double* niw_expectedstats, int32_t* info, void* stream);

/* Filter + backward sampler (cython_natural_lds_sample, /root/reference/svae/lds/lds_inference.py:260-264) of an LDS
 * whose natural parameters are all DIAGONAL -- the random-walk model of initialize_local_meanfield
 * (/root/reference/svae/models/slds_svae.py:203-226) under diagonal recognition potentials: n independent scalar
 * recursions per sequence, one lane each.  Same eps -> sample map as svae_lds_filter_f64 + svae_lds_sample_f64 on the
 * dense form of the same model (one sample per sequence).
 *  in : init_J, init_h (n); J11, J12, J22 (n): the diagonals (natural parameters as in svae_lds_estep_f64);
 *       node_J, node_h (B,T,n); eps (B,T,n)
 *  out: samples (B,T,n); info: b + 1 of a sequence with a non-positive precision, else untouched
 *  workspace: svae_lds_diag_sample_workspace_bytes(B,T,n) */
size_t svae_lds_diag_sample_workspace_bytes(int B, int T, int n);
int svae_lds_diag_sample_f64(int B, int T, int n, const double* init_J, const double* init_h,
                             const double* J11, const double* J12, const double* J22,
                             const double* node_J, const double* node_h, const double* eps,
                             double* samples, int32_t* info, void* workspace, size_t ws_bytes, void* stream);

/* Natural-gradient expression of /root/reference/svae/svae.py:33-34 for the LDS global parameter, straight from
 * the (all-reduced) buffer of svae_lds_reduce_stats_f64:
 *   natgrad = -scale * (prior + num_batches * stats - params)
 * over the flat parameter [NIW dense (n+2)^2 | A (n^2) | B (n^2) | C (n^2) | d (1)], where stats =
 * (pack_dense(sum E[x0 x0'], sum E[x0], count, count), (E_pair sums, count (T-1))).  One launch. */
int svae_lds_natgrad_f64(int n, int T, const double* packed_stats, const double* prior_flat,
                         const double* params_flat, double num_batches, double scale,
                         double* natgrad_flat, void* stream);

/* Deterministic sum over the batch of the per-sequence global statistics (the quantity that is
 * all-reduced across GPUs for the natural-gradient step, svae.py:33-34):
 *   out (n*n + n + 3*n*n + 2) = [sum_b E_init | sum_b E_pair | sum_b lognorm | B]
 * Homogeneous E_pair layout only. */
int svae_lds_reduce_stats_f64(int B, int n, const double* E_init, const double* E_pair,
                              const double* lognorm, double* out, void* stream);

/* ---- LDS E-step for latent dimension 65 <= n <= SVAE_LDS_XL_MAX_N (csrc/lds_estep_xl.hip) ---------------------------
 * Replaces cython_natural_lds_estep_general (svae/lds/lds_inference.py:232-237 of the reference) =
 *   natural_filter_forward_general  svae/lds/cython_lds_inference.pyx:28-90
 *   natural_smoother_general        svae/lds/cython_lds_inference.pyx:149-195
 *   _compute_stats                  svae/lds/cython_lds_inference.pyx:197-210
 * at the latent sizes above the tiled path.  One workgroup of NB = ceil(n/16) wavefronts per sequence; the step's panel
 * lives in registers, one 16-row block row per wavefront.
 *
 * Workspace bytes for (B, T, n): per (sequence, step) the hand-off record [X_t | P_t^-1 (row-major NP x NP) | c_t (NP)],
 * NP = 16 ceil(n/16), then the pair parameters re-packed in MFMA fragment order (3 NP^2 doubles per slot; 2 slots when
 * homogeneous, T-1 per parameter set when `inhomog`, one set per sequence when `pair_batched`; none when T = 1):
 *   8 (B T (2 NP^2 + NP) + [T >= 2] (pair_batched ? B : 1) (inhomog ? T-1 : 2) 3 NP^2)
 * n = 128: 263 KB per step and sequence -- B = 512, T = 200 needs 26.9 GB.  0 for B <= 0, T <= 0 or n outside
 * 65 .. SVAE_LDS_XL_MAX_N. */
size_t svae_lds_xl_workspace_bytes(int B, int T, int n, int inhomog, int pair_batched);

/* svae_lds_estep_f64's arguments, outputs and error codes for 65 <= n <= SVAE_LDS_XL_MAX_N (any other n: -3).  keep and
 * options must be 0 (-23 / -24): there is no sampler, VJP or kernel choice at these sizes.  Returns 0; -k for a bad
 * argument (before any HIP call); -22 workspace NULL or shorter than svae_lds_xl_workspace_bytes; -1000 / -1001 launch
 * errors; B = 0 returns 0 after the checks of T, n, keep, pair_batched, the shared parameters and options (the
 * per-sequence arrays and the workspace may then be NULL).  The status word `info` is set as by svae_lds_estep_f64
 * (non-positive pivot or a NaN log-normaliser). */
int svae_lds_xl_estep_f64(int B, int T, int n, int inhomog, int pair_batched, int keep, unsigned options,
                          const double* init_J, const double* init_h, const double* init_logZ,
                          const double* J11, const double* J12, const double* J22,
                          const double* logZ_pair,
                          const double* node_J, const double* node_h, const double* node_logZ,
                          double* lognorm, double* E_init, double* E_pair,
                          double* E_node_diagxx, double* E_node_x,
                          int32_t* info, void* workspace, size_t ws_bytes, void* stream);

/* svae_lds_reduce_stats_f64 (the batch sums all-reduced for svae.py:33-34) for the outputs of svae_lds_xl_estep_f64:
 * the same fixed-order reduction and output layout, 65 <= n <= SVAE_LDS_XL_MAX_N (else -2). */
int svae_lds_xl_reduce_stats_f64(int B, int n, const double* E_init, const double* E_pair,
                                 const double* lognorm, double* out, void* stream);

/* Backward sampling given the forward messages held in `workspace` by the LAST call of
 * svae_lds_estep_f64 with the same (B,T,n) and keep_factor != 0 [natural_sample_backward,
 * /root/reference/svae/lds/cython_lds_inference.pyx:310-355].
 *   eps     (B,T,S,n) standard-normal draws (the reference draws them inside, :333; passing them
 *           in makes the op deterministic and parity-testable)
 *   samples (B,T,S,n)
 */
int svae_lds_sample_f64(int B, int T, int n, int S, unsigned options, const double* eps, double* samples,
                        const void* workspace, size_t ws_bytes, void* stream);

/* E-step + backward sampling in ONE call: the composite the reference's model layer uses,
 *   cython_natural_lds_inference_general(natparam, node_params, num_samples) -> (samples, expected_stats, lognorm)
 *     /root/reference/svae/lds/lds_inference.py:196-202  (= natural_filter_forward_general, natural_smoother_general,
 *     natural_sample_backward: /root/reference/svae/lds/cython_lds_inference.pyx:28-90, 149-210, 310-355),
 * keeping in `workspace` -- keep_vjp != 0 -- what svae_lds_estep_vjp_ex_f64 needs (called with SVAE_OPT_INFER_RECORDS, the
 * same B, T, n, S, inhomog and `options`); keep_vjp = 0: forward values only (no cross-moment record; lean records then
 * also serve per-step / per-sequence pair parameters: the final pass of the SLDS's run_inference, slds_svae.py:289-310).  Arguments as svae_lds_estep_f64 (n <= SVAE_LDS_MAX_N) plus eps, samples (B,T,S,n) as
 * svae_lds_sample_f64; S = 0: no sampling (eps, samples may be NULL).  Same results as svae_lds_estep_f64 with keep = 3
 * followed by svae_lds_sample_f64 -- and in general exactly those two calls.  What the single entry point buys: for
 * homogeneous pair parameters, n <= 10, T >= 2, S <= 2 and batches of more than 2048 sequences (or SVAE_OPT_LEAN_ON)
 * the per-step records that travel through HBM shrink from (4n+3)n + (n+1)(n+2) doubles to n(n+1)/2 + n (+ the cross
 * moments): the forward pass keeps only U_t = chol(P_t)^-T and c_t, every reader rebuilds P_t^-1 = U U' and P_t^-1 J12,
 * the sampler runs inside the smoother's loop, and the first VJP sweep hands the second one symmetric triangle
 * (csrc/lds_lean_estep.hpp, lds_lean_vjp.hpp).  After a lean call svae_lds_sample_f64 cannot follow (the samples were
 * drawn here) and the VJP takes no cotangents of E_init / E_pair.  svae_lds_inference_is_lean: which format a call with
 * these arguments uses (1 = lean; host only, a pure function of its arguments).
 * Return values as svae_lds_estep_f64; -4: bad S / missing eps or samples; -100 + k: the sampler stage returned k. */
int svae_lds_inference_is_lean(int B, int T, int n, int S, int inhomog, int keep_vjp, unsigned options);
int svae_lds_inference_f64(int B, int T, int n, int S, int inhomog, int pair_batched, int keep_vjp, unsigned options,
                           const double* init_J, const double* init_h, const double* init_logZ,
                           const double* J11, const double* J12, const double* J22, const double* logZ_pair,
                           const double* node_J, const double* node_h, const double* node_logZ,
                           const double* eps, double* samples,
                           double* lognorm, double* E_init, double* E_pair,
                           double* E_node_diagxx, double* E_node_x,
                           int32_t* info, void* workspace, size_t ws_bytes, void* stream);

/* Bytes of scratch svae_lds_estep_vjp_f64 needs in addition to the E-step workspace. */
size_t svae_lds_vjp_workspace_bytes(int B, int T, int n);

/* Reverse-mode derivative (vector-Jacobian product) of the E-step [+ sampler] w.r.t. the node
 * potentials, for the LAST svae_lds_estep_f64 call on `workspace` with keep = 3 (and, if g_samples
 * is given, the svae_lds_sample_f64 call that followed).  One entry point for what the reference
 * wires as three autograd primitives (/root/reference/svae/lds/lds_inference.py:26-39):
 *   natural_filter_grad            /root/reference/svae/lds/cython_lds_inference.pyx:92-145
 *   natural_smoother_general_grad  /root/reference/svae/lds/cython_lds_inference.pyx:236-306
 *   natural_sample_backward_grad   /root/reference/svae/lds/cython_lds_inference.pyx:357-409
 *  in : J12 (n,n) natural pair parameter (homogeneous pair parameters only)
 *       g_lognorm (B); g_E_node_diagxx, g_E_node_x (B,T,n) or NULL; g_samples (B,T,S,n) or NULL with
 *       the eps (B,T,S,n) and samples (B,T,S,n) of the sampler call (S <= 16)
 *       (cotangents of E_init / E_pair are taken as zero: the model code never differentiates the
 *        global statistics, /root/reference/svae/svae.py:21)
 *  out: g_node_J (B,T,n), g_node_h (B,T,n)   [g_node_logZ[b,t] = g_lognorm[b]: trivial, left to the caller]
 */
int svae_lds_estep_vjp_f64(int B, int T, int n, int S, const double* J12,
                           const double* g_lognorm, const double* g_E_node_diagxx,
                           const double* g_E_node_x, const double* g_samples,
                           const double* eps, const double* samples,
                           double* g_node_J, double* g_node_h,
                           const void* workspace, size_t ws_bytes,
                           void* vjp_workspace, size_t vjp_ws_bytes, void* stream);

/* The same with per-step pair parameters and cotangents of the remaining statistics -- what the
 * SLDS-SVAE differentiates (/root/reference/svae/models/slds_svae.py:295-300: lds_stats feed
 * get_hmm_vlb; _compute_stats_grad /root/reference/svae/lds/cython_lds_inference.pyx:212-234):
 *   inhomog / pair_batched: J12 is (T-1,n,n) / (B,T-1,n,n) as in svae_lds_estep_f64
 *   g_E_init (B, n*n+n) or NULL: cotangent of [E[x0 x0'] | E[x0]]
 *   g_E_pair (B,T-1,3,n,n) or NULL (inhomog only): cotangent of the per-step pair statistics; needs
 *     the forward outputs E_pair (B,T-1,3,n,n) and E_node_x (B,T,n) of the E-step call
 * All other arguments as svae_lds_estep_vjp_f64 (which is this with inhomog = 0 and NULLs). */
int svae_lds_estep_vjp_ex_f64(int B, int T, int n, int S, int inhomog, int pair_batched, unsigned options,
                              const double* J12, const double* g_lognorm,
                              const double* g_E_node_diagxx, const double* g_E_node_x,
                              const double* g_E_init, const double* g_E_pair,
                              const double* g_samples, const double* eps, const double* samples,
                              const double* E_pair, const double* E_node_x,
                              double* g_node_J, double* g_node_h,
                              const void* workspace, size_t ws_bytes,
                              void* vjp_workspace, size_t vjp_ws_bytes, void* stream);

/* The same with one more output: g_node_J_dense (B,T,n,n) = -2 Pbar_t, the cotangent of a DENSE node potential J_t --
 * the (T,n,n) node potentials of the reference's Python path (natural_condition_on_general,
 * /root/reference/svae/lds/gaussian.py:46-49; lds_inference.py:65-82, 205-218), which the host folds into per-step
 * pair parameters (svae_amd/lds/lds_inference.py:_fold_dense_nodes): J_t enters the recursion only through the pivot
 * block P_t = J_pred,t + J_t (+ J11,t), so its cotangent is the whole of P_t's, of which g_node_J is the diagonal.  Not
 * symmetrised (the caller takes the symmetric part); runs the packed sweeps whatever B (only they write it).  -27: NULL
 * g_node_J_dense; -8 also with SVAE_OPT_INFER_RECORDS on lean records. */
int svae_lds_estep_vjp_dense_f64(int B, int T, int n, int S, int inhomog, int pair_batched, unsigned options,
                                 const double* J12, const double* g_lognorm,
                                 const double* g_E_node_diagxx, const double* g_E_node_x,
                                 const double* g_E_init, const double* g_E_pair,
                                 const double* g_samples, const double* eps, const double* samples,
                                 const double* E_pair, const double* E_node_x,
                                 double* g_node_J, double* g_node_h, double* g_node_J_dense,
                                 const void* workspace, size_t ws_bytes,
                                 void* vjp_workspace, size_t vjp_ws_bytes, void* stream);

/* Bytes of scratch svae_lds_estep_vjp_params_f64 needs in addition to the E-step and the VJP workspace: the per-step
 * blocks the second sweep leaves (-2 Pbar_t (B,T,n,n); the two halves of Rbar_t (B,T-1,2,n,n)) and, for homogeneous pair
 * parameters (inhomog = 0), the per-step batch sums (T-1,3,n,n) of the reduction's first pass.  0 for n outside
 * 1 .. SVAE_LDS_MAX_N or B, T <= 0. */
size_t svae_lds_param_vjp_workspace_bytes(int B, int T, int n, int inhomog, int pair_batched);

/* svae_lds_estep_vjp_ex_f64 plus the cotangents of the seven NATURAL PARAMETERS of the model -- the gradients the
 * reference's Python path has through autograd (/root/reference/svae/lds/lds_inference.py:205-218), which the compiled
 * path does not offer.  1 <= n <= SVAE_LDS_MAX_N, full (not lean) records.  With P_t = J_pred,t - 2 diag(node_J_t) - 2 J11_t,
 * R_t = -J12_t, H_t = P_t^-1 [R_t | h_filt,t], [J_pred | h_pred]_{t+1} = [-2 J22_t | 0] - R_t' H_t (info form):
 *   g_J11_t = -2 Pbar_t (t <= T-2), g_J22_t = -2 Pbar_{t+1}, g_init_J = -2 Pbar_0      -- returned SYMMETRISED
 *   g_J12_t = -(Bbar_t[:, :n] - H_t [Abar | hbar]_{t+1}')                               -- a full matrix
 *   g_init_h = hfbar_0 (= g_node_h[:,0]);  g_init_logZ = g_logZ_pair_t = g_lognorm
 * each summed over what the parameter is shared over, in a fixed order (bit-reproducible; csrc/lds_param_grad.hip):
 *   out: g_init_J (n,n), g_init_h (n), g_init_logZ (1): summed over the batch
 *        g_J11, g_J12, g_J22, g_logZ_pair in the layout of the pair parameters: (n,n) / (1) summed over batch and time
 *        (g_logZ_pair = (T-1) sum_b g_lognorm); (T-1,n,n) / (T-1) summed over the batch; (B,T-1,n,n) / (B,T-1) per sequence
 *        any of the seven may be NULL (not wanted)
 *        g_node_J, g_node_h (B,T,n): required, bit-identical to svae_lds_estep_vjp_ex_f64 on the same arguments (the
 *        sweeps run as they do there; where that second sweep is not the packed one -- batches up to 1024 by default --
 *        the packed sweep follows as a second pass for the parameter blocks alone)
 *   param_workspace: svae_lds_param_vjp_workspace_bytes(B,T,n,inhomog,pair_batched)
 * Returns the codes of svae_lds_estep_vjp_ex_f64 (-1 B, -2 T, -3 n outside 1 .. 15, -4 S, -5 J12, -6 g_lognorm,
 * -7 pair_batched without inhomog, -8 g_E_pair without its operands -- and lean records under SVAE_OPT_INFER_RECORDS --,
 * -10 eps / samples, -12 g_node_J, -13 g_node_h, -14 workspace, -16 vjp_workspace, -24 options), -29 param_workspace NULL
 * or too small, -30 T > 65536; all before any HIP call.  B = 0 returns 0. */
int svae_lds_estep_vjp_params_f64(int B, int T, int n, int S, int inhomog, int pair_batched, unsigned options,
                                  const double* J12, const double* g_lognorm,
                                  const double* g_E_node_diagxx, const double* g_E_node_x,
                                  const double* g_E_init, const double* g_E_pair,
                                  const double* g_samples, const double* eps, const double* samples,
                                  const double* E_pair, const double* E_node_x,
                                  double* g_node_J, double* g_node_h,
                                  double* g_init_J, double* g_init_h, double* g_init_logZ,
                                  double* g_J11, double* g_J12, double* g_J22, double* g_logZ_pair,
                                  const void* workspace, size_t ws_bytes,
                                  void* vjp_workspace, size_t vjp_ws_bytes,
                                  void* param_workspace, size_t param_ws_bytes, void* stream);

/* Batched HMM E-step: log-normaliser and expected statistics of B chains with K <= SVAE_HMM_MAX_K = 64 states
 * (K <= 16: one 16-lane DPP row per sequence, two-ended scaled recursions; 17 <= K <= 64, round 6: one wavefront per
 * sequence, lane = state, scaled recursions with a log-space redo of flagged sequences -- csrc/hmm_estep_wide.hip)
 * [hmm_logZ  /root/reference/svae/hmm/cython_hmm_inference.pyx:93-121 and hmm_logZ_grad :126-166 at
 *  g = 1, i.e. `hmm_estep_slow = vgrad(hmm_logZ)` /root/reference/svae/hmm/hmm_inference.py:65; the
 *  reference's hmm_estep (:21-41) delegates to the un-vendored pyhsmm].
 *  in : init_params (K) log initial potentials; pair_params (K,K) log transition potentials [j][k] =
 *       j -> k, or (B,K,K) if pair_batched; node_params (B,T,K) log node potentials
 *  out: logZ (B); E_init (B,K) = E[z_0]; E_trans (B,K,K) = sum_t E[z_t = j, z_{t+1} = k];
 *       E_states (B,T,K) = E[z_t]
 *  workspace: svae_hmm_workspace_bytes(B,T,K) = B T R doubles, R = 50 for K <= 16, KP + 2 above (KP = 32 or 64 padded
 *       states); 0 for B <= 0, T <= 0 or K outside 1..SVAE_HMM_MAX_K.
 *  Range: the recursions are SCALED (potentials shifted by their maximum and exponentiated, messages renormalised), and a
 *  scaled step loses whatever falls below 2.3e-308 of its scale -- for good: a lost component is never rebuilt.  A
 *  sequence keeps the scaled result only while every state's component of every step's unnormalised message stays >= 1e-250
 *  (and every normaliser above 1e-200): what a step drops is then 1e-50 below the positive sum it is dropped from.  Every
 *  other sequence is RECOMPUTED IN LOG SPACE by a second launch (the reference's own arithmetic, K log-sum-exps per step;
 *  by its operation count -- K exp and a log per state and step where the scaled step has K multiply-adds -- roughly 10x a
 *  scaled sequence's time, an estimate: no workload with flagged sequences has been timed; the launch costs a flag read
 *  per sequence otherwise), so for finite or -inf potentials every sequence WITH A PATH OF FINITE SCORE has the log-space
 *  result to rounding.  A sequence with no such path (log Z = -inf) is outside the contract: the log-space pass divides
 *  every step's marginals by their own sum, and its outputs for that sequence are NaN; no other sequence is affected.  A state forbidden by a -1e4 or -inf potential sends its
 *  sequence that way.  Which did is recorded: after the call, double R - 1 of a sequence's FIRST workspace record (entry
 *  [b T R + R - 1]) is 1.0 if sequence b was recomputed, else 0.0.
 */
size_t svae_hmm_workspace_bytes(int B, int T, int K);
int svae_hmm_estep_f64(int B, int T, int K, int pair_batched,
                       const double* init_params, const double* pair_params,
                       const double* node_params,
                       double* logZ, double* E_init, double* E_trans, double* E_states,
                       void* workspace, size_t ws_bytes, void* stream);

/* Batched HMM Viterbi decoding: the most probable state path of B chains with K <= SVAE_HMM_MAX_K states and its
 * score, on the LOG potentials svae_hmm_estep_f64 takes (entries may be -inf) -- csrc/hmm_viterbi.hip
 * [hmm_viterbi of the reference, svae/hmm/hmm_inference.py:54-63, delegates to the un-vendored pyhsmm: the arithmetic is
 *  defined HERE, and reproducible bit for bit by restating it in the same order]:
 *    delta_0[k] = init[k] + node[0][k];   delta_t[k] = (max_j (delta_{t-1}[j] + pair[j][k])) + node[t][k]   (fp64 adds
 *    in that order);  psi_t[k] = the LOWEST j attaining the maximum;  z_{T-1} = the lowest k attaining
 *    max_k delta_{T-1}[k];  z_t = psi_{t+1}[z_{t+1}];  score = delta_{T-1}[z_{T-1}].
 *  A chain all of whose potentials are -inf at some step has score -inf and the labels the lowest-index rule gives.
 *  NaN inputs: unspecified labels in 0..K-1, no fault.
 *  in : init_params (K); pair_params (K,K) [j][k] = j -> k, or (B,K,K) if pair_batched; node_params (B,T,K)
 *  out: states (B,T) int32; score (B) or NULL
 *  workspace: svae_hmm_viterbi_workspace_bytes(B,T,K) = B T KP bytes rounded up to a multiple of 8 (one back-pointer
 *       byte per step and padded state, KP = 16, 32 or 64 for K <= 16, <= 32, <= 64); 0 for B <= 0, T <= 0 or K outside
 *       1..SVAE_HMM_MAX_K.  16-byte aligned.
 *  Returns 0, or (decided on the host before any HIP call) -1 B < 0, -2 T < 1, -3 K outside 1..SVAE_HMM_MAX_K,
 *  -4 pair_batched not 0 or 1, -5 init_params NULL, -6 pair_params NULL, [B = 0 returns 0 here], -7 node_params NULL,
 *  -8 states NULL, -10 workspace NULL, -11 ws_bytes too small, -12 workspace not 16-byte aligned; -1000 launch error.
 *  Asynchronous on `stream`, no internal allocation, safe under graph capture. */
size_t svae_hmm_viterbi_workspace_bytes(int B, int T, int K);
int svae_hmm_viterbi_f64(int B, int T, int K, int pair_batched,
                         const double* init_params, const double* pair_params,
                         const double* node_params, int32_t* states, double* score,
                         void* workspace, size_t ws_bytes, void* stream);

/* svae_hmm_estep_f64 / svae_hmm_viterbi_f64 with PER-SEQUENCE LENGTHS: one padded batch, sequence b occupying steps
 * 0 .. L_b - 1 of its (T, K) block, L_b = lengths[b] (device int32).  Additions to ABI 15 (no new number).
 *  E-step : logZ[b], E_init[b], E_trans[b] and E_states[b, :L] are those of the sequence cut to L steps (E_trans sums the
 *           sequence's own L - 1 transitions: exactly 0 for L = 1; E_init = the marginal at t = 0); E_states[b, t >= L] is
 *           exactly 0.0.  K <= 16: the one-directional DPP-row kernel, rows of different lengths under per-row masks;
 *           17 <= K <= 64: the wide kernel, loops to L; both with the log-space launch of the uniform call behind them
 *           (the range criterion and the REDO word of svae_hmm_estep_f64, over the sequence's own L steps).
 *  Viterbi: states[b, :L] and score[b] are those of the cut sequence under the exact arithmetic defined above;
 *           states[b, t >= L] = -1.
 *  Nothing stored at t >= L is ever read: node potentials there may be NaN or +-inf.  No sequence sees another's length or
 *  data.  A length outside 1..T is clamped to [1, T] for addressing and trip counts and ORs 1 into the device word `info`
 *  (an atomic; never cleared by the library, never read on the host: no synchronisation).
 *  Arrays, workspace sizes (svae_hmm_workspace_bytes / svae_hmm_viterbi_workspace_bytes) and record strides are those of
 *  the uniform calls.  Returns 0, or (decided on the host before any HIP call, the first failing check)
 *   both   : -1 B < 0, -2 T < 1, -3 K outside 1..SVAE_HMM_MAX_K, -4 pair_batched not 0 or 1, -5 init_params NULL,
 *            -6 pair_params NULL, [B = 0 returns 0 here], -7 node_params NULL, -8 lengths NULL;
 *   E-step : -9 logZ NULL, -10 E_init NULL, -11 E_trans NULL, -12 E_states NULL, -13 info NULL, -14 workspace NULL,
 *            -15 ws_bytes too small;
 *   Viterbi: -9 states NULL, -10 info NULL, -11 workspace NULL, -12 ws_bytes too small, -13 workspace not 16-byte aligned;
 *  -1000 launch error.  Asynchronous on `stream`, no internal allocation, safe under graph capture. */
int svae_hmm_ragged_estep_f64(int B, int T, int K, int pair_batched,
                              const double* init_params, const double* pair_params, const double* node_params,
                              const int32_t* lengths,
                              double* logZ, double* E_init, double* E_trans, double* E_states,
                              int32_t* info, void* workspace, size_t ws_bytes, void* stream);
int svae_hmm_ragged_viterbi_f64(int B, int T, int K, int pair_batched,
                                const double* init_params, const double* pair_params, const double* node_params,
                                const int32_t* lengths,
                                int32_t* states, double* score /* or NULL */,
                                int32_t* info, void* workspace, size_t ws_bytes, void* stream);

/* svae_hmm_estep_f64 PARTITIONED IN TIME, for long sequences, K <= 16 -- csrc/hmm_estep_chunked.hip.  Additions to ABI 15
 * (no new number).  The T steps are cut into C = ceil(T / chunk) chunks (the last may be as short as one step): stage 1
 * builds every chunk's K x K transfer operator as K independently scaled rows, in parallel over (sequence, chunk, start
 * state); stage 2 scans the C operators of a sequence for log Z and the messages at the chunk boundaries; stage 3 runs the
 * scaled forward-backward of every chunk in parallel and sums the chunks' transition counts in chunk order (no
 * floating-point atomics: the outputs are reproducible bit for bit).  Arguments and results are svae_hmm_estep_f64's.
 *  chunk  : steps per chunk, >= 2.  chunk >= T runs svae_hmm_estep_f64's launches and nothing else (same bits).
 *           svae_hmm_chunked_default_chunk(B,T,K) is the library's pick; it returns T where the serial route is expected
 *           to win, and for arguments this entry refuses.
 *  logZ only: E_init, E_trans and E_states all NULL -- stages 1 and 2 alone; a mix of NULL and non-NULL is refused.
 *  Range  : the contract of svae_hmm_estep_f64.  A sequence keeps the chunked result only while every live component --
 *           of every operator row from its chunk's second step on, of the first chunk's filter, of every weighted entry and
 *           product of stage 2, of stage 3's forward messages -- stays >= 1e-250 of its scale and every normaliser above
 *           1e-200.  Any other sequence is recomputed WHOLE by the serial route (an indexed launch over the flagged
 *           sequences), whose own log-space redo stands behind it.  Which were is recorded: after the call with chunk < T
 *           the workspace opens with B int32 route words, 1 = sequence b was recomputed by the serial route, else 0.
 *  workspace: svae_hmm_chunked_workspace_bytes(B,T,K,chunk) = 8 B (1 + T (50 + K) + K K + K + C (2 K K + 3 K)) bytes,
 *           C = ceil(T / chunk) (1 for chunk >= T): the route words and the recompute launch's slots, the serial route's
 *           records (stage 3's alias them) and statistics (used for logZ only), the operators, their log scales, the
 *           boundary messages and the chunks' counts (layout: csrc/hmm_args.hpp).  0 for B <= 0, T <= 0, K outside 1..16
 *           or chunk < 2.  8-byte aligned.
 *  Returns 0, or (decided on the host before any HIP call, the first failing check) -1 B < 0, -2 T < 1, -3 K outside
 *  1..16, -4 pair_batched not 0 or 1, -5 init_params NULL, -6 pair_params NULL, [B = 0 returns 0 here], -7 chunk < 2,
 *  -8 node_params NULL, -9 logZ NULL, -10 some but not all of E_init / E_trans / E_states NULL, -11 workspace NULL,
 *  -12 ws_bytes too small; -1000 launch error.  Asynchronous on `stream`, no internal allocation, safe under graph
 *  capture. */
int svae_hmm_chunked_default_chunk(int B, int T, int K);
size_t svae_hmm_chunked_workspace_bytes(int B, int T, int K, int chunk);
int svae_hmm_chunked_estep_f64(int B, int T, int K, int pair_batched, int chunk,
                               const double* init_params, const double* pair_params, const double* node_params,
                               double* logZ, double* E_init /* or NULL */, double* E_trans /* or NULL */,
                               double* E_states /* or NULL */, void* workspace, size_t ws_bytes, void* stream);

/* svae_hmm_viterbi_f64 PARTITIONED IN TIME, for long sequences, K <= 16 -- csrc/hmm_viterbi_chunked.hip.  Additions to
 * ABI 15 (no new number).  Arguments and results are svae_hmm_viterbi_f64's; there are no per-sequence lengths.
 * The arithmetic, DEFINED here: fp64 adds and strict-`>` running maxima in the stated order, nothing else, so a restatement
 * in the same order reproduces labels and score bit for bit.  L = chunk, C = ceil(T / L); chunk c covers steps
 * t0 = c L .. t1 - 1, t1 = min((c + 1) L, T) (the last chunk may be one step).
 *   step(d, t)[k] = (max_j (d[j] + pair[j][k])) + node[t][k], the running maximum in j order, the lowest j on ties
 *   (the step of svae_hmm_viterbi_f64's recursion).
 *  1 operators: for c >= 1, row j of M_c starts as pair[j][:] + node[t0][:] and takes `step` over t0+1 .. t1-1; chunk 0
 *    is the recursion from delta_0 = init + node[0], its end vector D_0.  Parallel over (sequence, chunk, start state).
 *  2 scan: D_c[k] = max_j (D_{c-1}[j] + M_c[j][k]), the running maximum in j order; serial over c, one row per sequence.
 *  3 decode: chunk c enters with D_{c-1} (chunk 0 with init + node[0]) and runs `step` over its own steps (step t0 included
 *    for c >= 1), keeping psi_t[k] = the lowest j attaining the maximum (psi_0 = 0).  The last chunk gives z_{T-1} = the
 *    lowest k attaining the maximum of its final delta, and score = that maximum.  Then, for every end state k at once,
 *    the path that ends the chunk in k is followed down to t0: cand[t][k] = its label at t, f_c[k] = psi_{t0}[cand[t0][k]]
 *    = the end state of chunk c - 1 it arrives at.  Parallel over (sequence, chunk).
 *  4 resolve: e_{C-1} = z_{T-1}; e_{c-1} = f_c[e_c].   5 gather: states[b,t] = cand[t][e_{c(t)}], c(t) = t / L.
 * The serial call has chains of T and T steps; this one chains of L, C, L, L and C steps and one flat pass.
 * Against svae_hmm_viterbi_f64:
 *  (a) chunk >= T runs svae_hmm_viterbi_f64's launch and nothing else: the same bits.
 *  (b) where every fp64 add of the recursion is exact (potentials that are multiples of 2^-q with
 *      T max|potential| 2^q < 2^53, say; -inf entries included) max-plus is associative, D_{c-1} is the serial delta, and
 *      labels and score equal svae_hmm_viterbi_f64's bit for bit, ties included.
 *  (c) otherwise the boundary deltas differ from the serial ones in rounding: the labels are a path whose serially summed
 *      score (((init + node_0) + pair) + node_1 ...) lies within 4 T 2^-53 A of svae_hmm_viterbi_f64's score, and so does
 *      the returned score; A = max|init| + sum_t max_k |node_t| + (T - 1) max|pair| over the finite entries (the
 *      first-order bound for <= 2 T roundings of partial sums no larger than A, doubled).
 *  (d) NaN inputs: unspecified labels in 0..K-1, no fault, as for the serial entry.
 *  (e) no atomics: the outputs are reproducible bit for bit.  Asynchronous on `stream`, no internal allocation, safe under
 *      graph capture.
 *  chunk  : steps per chunk, >= 2.  svae_hmm_chunked_viterbi_default_chunk(B,T,K) is the library's pick; it returns T
 *           where the serial route is expected to win, and for arguments this entry refuses.
 *  workspace: svae_hmm_chunked_viterbi_workspace_bytes(B,T,K,chunk) =
 *           32 B T + 16 B C + 16 ceil(B C / 16) + 8 B C K (K + 1) bytes, C = ceil(T / chunk) (1 for chunk >= T): the
 *           back-pointers (B T 16, at the head: never less than svae_hmm_viterbi_workspace_bytes(B,T,K), so route (a)
 *           fits), the candidates (B T 16, a buffer of their own: they do not alias the back-pointers), the chunk maps f
 *           (B C 16), the chunk end states e (B C bytes, padded to 16), the operators (B C K K doubles) and the boundary
 *           deltas (B C K doubles) (layout: csrc/hmm_args.hpp).  0 for B <= 0, T <= 0, K outside 1..16 or chunk < 2.
 *           16-byte aligned.
 *  Returns 0, or (decided on the host before any HIP call, the first failing check) -1 B < 0, -2 T < 1, -3 K outside
 *  1..16, -4 pair_batched not 0 or 1, -5 init_params NULL, -6 pair_params NULL, [B = 0 returns 0 here], -7 chunk < 2,
 *  -8 node_params NULL, -9 states NULL, -10 workspace NULL, -11 ws_bytes too small, -12 workspace not 16-byte aligned;
 *  -1000 launch error. */
int svae_hmm_chunked_viterbi_default_chunk(int B, int T, int K);
size_t svae_hmm_chunked_viterbi_workspace_bytes(int B, int T, int K, int chunk);
int svae_hmm_chunked_viterbi_f64(int B, int T, int K, int pair_batched, int chunk,
                                 const double* init_params, const double* pair_params, const double* node_params,
                                 int32_t* states, double* score /* or NULL */,
                                 void* workspace, size_t ws_bytes, void* stream);

/* Batched HMM posterior sampling: S state paths per chain, z_{0:T-1} ~ p(z | potentials), by forward filtering and
 * backward sampling, on the LOG potentials svae_hmm_viterbi_f64 takes (entries may be -inf), K <= SVAE_HMM_MAX_K --
 * csrc/hmm_sample.hip.  Additions to ABI 15 (no new number).  [pyhsmm's message interface, to which the reference
 * delegates its HMM work, has the operation; the arithmetic is defined HERE.]  The caller supplies the randomness.
 * For sequence b of length L (= T in the uniform call) and sample s:
 *  Filtered distributions  a_t[k] = p(z_t = k | node_{0..t}), t < L: the scaled forward filter of the E-step kernels
 *    (per-step max-shift of the node potentials, renormalisation to sum 1, log Z accumulated as mantissa/exponent pairs),
 *    under the E-step's RANGE contract (svae_hmm_estep_f64, above; csrc/hmm_args.hpp, HMM_LOW): a sequence keeps its scaled
 *    filter only while every live state's component of every step's unnormalised message (sum_j a_{t-1}[j] P[j][k]) e_t[k]
 *    -- P and e shifted to a maximum of 1; at t = 0 the shifted, exponentiated init + node_0 -- stays >= 1e-250 and every
 *    normaliser above 1e-200.  Any other sequence (a transition more than ~575 nats below the matrix' maximum on a path
 *    that matters or not, E[log pi] of a sparse Dirichlet row, a state forbidden by -1e4 or -inf) is filtered again, ALL
 *    of it, in log space -- x_t[k] = logsumexp_j(la_{t-1}[j] + pair[j][k]) + node_t[k], la_t = x_t - logsumexp_k x_t[k],
 *    log Z = the sum of those normalisers (csrc/hmm_sample_log.hip) -- and its draws use the log-space weights below at
 *    every step.  So for finite or -inf log-potentials every sequence has the paths of the log-space definition to
 *    rounding.  Example: K = 2, T = 4, init (0, 0), pair ((0, -800), (0, 0)), node ((0, -inf), (0, 0), (-inf, 0),
 *    (0, log 2)): the chain starts in state 0, must be in state 1 at t = 2 and gets there through the -800 entry at either
 *    step; log Z = -800 + log 6, and the draws have the marginals (1, 0), (1/2, 1/2), (0, 1), (1/3, 2/3).
 *  Weights  t = L-1: w[k] = a_{L-1}[k];  t < L-1: w[k] = a_t[k] exp(pair[k][z_{t+1}] - M), M = the matrix' largest entry.
 *    If sum_k w[k] < 1e-200 the weights of that draw are recomputed in log space:
 *    w[k] = exp(log a_t[k] + pair[k][z_{t+1}] - max_k(log a_t[k] + pair[k][z_{t+1}])).
 *    A sequence whose filter was redone in log space draws EVERY step with these weights, from the stored log a_t
 *    (t = L-1: w[k] = exp(log a_{L-1}[k] - max_k log a_{L-1}[k])).
 *  Selection  C[k] = w[0] + .. + w[k], fp64 additions IN INDEX ORDER (both kernel mappings implement exactly this order:
 *    K <= 16 as K broadcast multiply-adds by 1.0 or 0.0, 17 <= K <= 64 as KP sequential adds of an LDS line that holds KP
 *    zeros and then w), so C is non-decreasing and rises only where w[k] > 0.  thr = clamp(u[b,s,t], 0, 1) C[K-1]; a NaN u
 *    counts as 0.  z_t = the number of k with C[k] <= thr; if that number is K (the product rounded up to the total),
 *    z_t = the lowest k with C[k] = C[K-1].  [One test: z_t = #{k : C[k] <= thr and C[k] < C[K-1]}.]
 *    Consequence: on a chain with finite log Z a drawn state always has positive weight -- a forbidden (-inf) transition
 *    or observation is never sampled; u = 0 draws the lowest allowed state, u = 1 the highest.
 *  Degenerate input: a chain with logZ = -inf, or NaN potentials, gives unspecified labels in 0..K-1: no fault, and no
 *    effect on any other sequence (every data-dependent index is masked into range before it addresses LDS or memory).
 *  in : init_params (K); pair_params (K,K) [j][k] = j -> k, or (B,K,K) if pair_batched; node_params (B,T,K);
 *       S >= 1 samples per sequence; u (B,S,T) fp64 uniforms
 *  out: states (B,S,T) int32, sample-major: states[:, s] is a (B,T) label array of the form svae_hmm_viterbi_f64 returns;
 *       logZ (B) or NULL
 *  workspace: svae_hmm_sample_workspace_bytes(B,T,K) = B T KP doubles, KP = 16, 32 or 64 for K <= 16, <= 32, <= 64; 0
 *       for B <= 0, T <= 0 or K outside 1..SVAE_HMM_MAX_K.  16-byte aligned.  One record of KP doubles per (sequence,
 *       step), and the records say themselves which route a sequence took: a SCALED record holds a_t (padding lanes 0) --
 *       it sums to 1, so it has a strictly positive entry and none below 0; a LOG record holds log a_t, normalised and
 *       clamped to <= 0 (padding lanes -inf) -- it has no positive entry.  Between the launches a sequence the scaled
 *       filter flagged carries -1 in every live lane of its step-0 record; the log-space launch replaces all of its
 *       records 0 .. L-1 and its logZ; the draw tests the first record it reads (step L-1): no live entry > 0 = a log
 *       record.  Afterwards "no live entry > 0 in the step-0 record" tells which sequences were redone (Python:
 *       hmm_inference.sample_redone_sequences).  A redone sequence costs K log-sum-exps of KP terms per step.
 *  Ragged form (svae_hmm_ragged_sample_f64, lengths (B) device int32), the conventions of the other ragged entries:
 *    results up to L are those of the sequence cut at L; states[b, :, t >= L] = -1; node_params[b, L:] and u[b, :, L:]
 *    are never read and may be NaN; no sequence sees another's length or data; a length outside 1..T is clamped to [1, T]
 *    for addressing and ORs 1 into the device word `info`.
 *  Returns 0, or (decided on the host before any HIP call, the first failing check)
 *   both   : -1 B < 0, -2 T < 1, -3 K outside 1..SVAE_HMM_MAX_K, -4 pair_batched not 0 or 1, -5 init_params NULL,
 *            -6 pair_params NULL, [B = 0 returns 0 here], -7 node_params NULL;
 *   uniform: -8 S < 1, -9 u NULL, -10 states NULL, -11 workspace NULL, -12 ws_bytes too small, -13 workspace not
 *            16-byte aligned;
 *   ragged : -8 lengths NULL, -9 S < 1, -10 u NULL, -11 states NULL, -12 info NULL, -13 workspace NULL, -14 ws_bytes too
 *            small, -15 workspace not 16-byte aligned;
 *  -1000 launch error.  Three launches (scaled filter; log-space filter, whose workgroups leave at once where the sequence
 *  is not flagged; draw), asynchronous on `stream`, no internal allocation, safe under graph capture.  B S T must be below
 *  2^31. */
size_t svae_hmm_sample_workspace_bytes(int B, int T, int K);
int svae_hmm_sample_f64(int B, int T, int K, int S, int pair_batched,
                        const double* init_params, const double* pair_params,
                        const double* node_params, const double* u,
                        int32_t* states, double* logZ /* or NULL */,
                        void* workspace, size_t ws_bytes, void* stream);
int svae_hmm_ragged_sample_f64(int B, int T, int K, int S, int pair_batched,
                               const double* init_params, const double* pair_params,
                               const double* node_params, const int32_t* lengths, const double* u,
                               int32_t* states, double* logZ /* or NULL */,
                               int32_t* info, void* workspace, size_t ws_bytes, void* stream);

/* svae_hmm_sample_f64 PARTITIONED IN TIME, for long sequences, K <= 16 -- csrc/hmm_sample_chunked.hip.  Additions to
 * ABI 15 (no new number).  Arguments and results are svae_hmm_sample_f64's (u (B,S,T), states (B,S,T) int32 sample-major,
 * potentials finite or -inf, logZ (B) or NULL); there are no per-sequence lengths.  With the uniforms fixed, the backward
 * draw at step t is a MAP from z_{t+1} to z_t, like a Viterbi back-pointer.  The arithmetic, DEFINED here: L = chunk,
 * C = ceil(T / L); chunk c covers steps t0 = c L .. t1 - 1, t1 = min((c + 1) L, T) (the last chunk may be one step).
 *  1 operators, 2 forward scan: stages 1 and 2 of svae_hmm_chunked_estep_f64 in its log-Z-only form, by that unit's own
 *    kernels.  They give the filtered message a^_c at every chunk's last step, log Z -- svae_hmm_chunked_estep_f64's bit
 *    for bit at the same chunk -- and that call's range flags for these stages.
 *  3 filter: chunk c runs the scaled step of svae_hmm_sample_f64's filter over its own steps, entered with a^_{c-1} in
 *    place of the initial message (chunk 0: from `init`), and stores a_t, 16 doubles per step, padding lanes 0, under the
 *    same per-step range test (live component >= 1e-250, normaliser > 1e-200, a NaN fails).  Parallel over (sequence, chunk).
 *  4 maps: for every chain (b, s) and step t >= 1, psi_t[k] = the state drawn at t - 1 given z_t = k, for all K values of
 *    k, from the record a_{t-1}, column k of the matrix and u[b,s,t-1]; z_{T-1} is drawn from a_{T-1} with u[b,s,T-1].
 *    Weights and selection are exactly svae_hmm_sample_f64's (above): w[j] = a[j] exp(pair[j][k] - M) a rounded product
 *    (not contracted into the sum), C summed in index order, thr = clamp(u) C[K-1] (a NaN u counts as 0),
 *    z = #{j : C[j] <= thr and C[j] < C[K-1]}; the log-space recompute where the total is below 1e-200, and the log-space
 *    weights at every step of a sequence whose record is a log record (no live entry > 0 in its record of step T-1).
 *    One uniform serves all K conditioning states: a valid coupling, and only the entry on the realised path reaches the
 *    output, so the labels are those of svae_hmm_sample_f64's draw run on the same records.  Flat over (chain, step).
 *  5 chase: for every end state k of chunk c at once the maps are followed down to t0: cand[t][k] = the label at t of the
 *    path that ends the chunk in k, f_c[k] = psi_{t0}[cand[t0][k]].  Parallel over (chain, chunk).
 *  6 resolve: e_{C-1} = z_{T-1}; e_{c-1} = f_c[e_c].   7 gather: states[b,s,t] = cand[t][e_{c(t)}], c(t) = t / L -- the
 *    chunked Viterbi decoder's kernels, on B S chains.
 * The serial call has chains of T and T steps; this one chains of L, C, L, L and C steps and two flat passes.
 * RANGE: svae_hmm_sample_f64's contract, whole.  A sequence flagged in any of stages 1 - 3 raises an int32 route word in the
 * workspace (zeroed by a memset node at the start of the call); a small kernel writes -1 into the live lanes of its step-0
 * record; the log-space filter launch of svae_hmm_sample_f64 then replaces all of its records and its log Z (its workgroups
 * leave at once elsewhere), and stage 4 draws every step of it with the log-space weights.  So every sequence with finite
 * log Z has the paths of the log-space definition to rounding.  A flagged sequence costs one serial log-space filter of T
 * steps, K log-sum-exps of 16 terms each (an operation-count estimate; it has not been timed).  Afterwards "no live entry
 * > 0 in the step-0 record" tells which sequences were redone, as for the serial call.
 * Against svae_hmm_sample_f64: chunk >= T runs svae_hmm_sample_f64 on the head of the workspace and nothing else: the same
 * bits.  Otherwise the records differ from the serial filter's in rounding (the boundary messages come from the scan), so
 * a draw whose uniform lies within that rounding of a boundary of the cumulative weights may differ.  NaN potentials or a
 * chain with log Z = -inf: unspecified labels in 0..K-1, no fault, no effect on other sequences.  No atomics: the outputs
 * are reproducible bit for bit.  Asynchronous on `stream`, no internal allocation, safe under graph capture.
 *  chunk  : steps per chunk, >= 2.  svae_hmm_chunked_sample_default_chunk(B,T,K,S) is the library's pick: the chunked
 *           E-step's rule applied to B -- T (the serial route) for T < 500 or B > 128, else the power of two nearest
 *           1.2 sqrt(T).  Derived from the table of DESIGN 4.5m (tools/bench_hmm_sample_chunked.py, one MI355X, K = 8 and
 *           16, S = 1 and 8): chunked beat the serial call at every measured shape with T >= 500 and B <= 128 (1.9x - 5x at
 *           T = 500, 2.7x - 25x at T = 5000, 10x - 93x at T = 50000), the rule's pick within 3.2 % of the best measured
 *           chunk; at 512 x 500 it lost at K = 16.  T < 500 and 129 .. 511 sequences were not measured: serial.  It
 *           returns T for arguments this entry refuses.
 *  workspace: svae_hmm_chunked_sample_workspace_bytes(B,T,K,S,chunk) = 128 B T + r16(8 B) + r16(4 B) + r16(8 B C K K) +
 *           2 r16(8 B C K) + 32 R T + 16 R C + r16(R C) bytes, R = B S, C = ceil(T / chunk) (1 for chunk >= T), r16(x) = x
 *           rounded up to a multiple of 16: the records (B T 16 doubles AT THE HEAD, svae_hmm_sample_f64's layout: never
 *           less than svae_hmm_sample_workspace_bytes(B,T,K), so the chunk >= T route fits), log Z where the caller passes
 *           none, the route words, the operators, their log scales, the boundary messages a^, the maps (R T 16 bytes), the
 *           candidates (R T 16, a buffer of their own: they do not alias the maps), the chunk maps f (R C 16) and the chunk
 *           end states e (R C bytes) (layout: csrc/hmm_args.hpp).  0 for B <= 0, T <= 0, K outside 1..16, S <= 0 or
 *           chunk < 2.  16-byte aligned.
 *  Returns 0, or (decided on the host before any HIP call, the first failing check) -1 B < 0, -2 T < 1, -3 K outside
 *  1..16, -4 pair_batched not 0 or 1, -5 init_params NULL, -6 pair_params NULL, [B = 0 returns 0 here], -7 chunk < 2,
 *  -8 node_params NULL, -9 S < 1, -10 B S T not below 2^31, -11 u NULL, -12 states NULL, -13 workspace NULL, -14 ws_bytes
 *  too small, -15 workspace not 16-byte aligned; -1000 launch error. */
int svae_hmm_chunked_sample_default_chunk(int B, int T, int K, int S);
size_t svae_hmm_chunked_sample_workspace_bytes(int B, int T, int K, int S, int chunk);
int svae_hmm_chunked_sample_f64(int B, int T, int K, int S, int pair_batched, int chunk,
                                const double* init_params, const double* pair_params,
                                const double* node_params, const double* u,
                                int32_t* states, double* logZ /* or NULL */,
                                void* workspace, size_t ws_bytes, void* stream);

/* Reverse-mode derivative of the batched HMM E-step (svae_hmm_estep_f64 / svae_hmm_ragged_estep_f64), K <=
 * SVAE_HMM_MAX_K -- csrc/hmm_estep_vjp.hip, which states the arithmetic.  Additions to ABI 15 (no new number).  The
 * cotangents of all four outputs are pulled back to all three inputs: with phi(z) = g_init[z_0] + sum_t g_trans[z_t,
 * z_{t+1}] + sum_t g_states[t, z_t], gamma_t and xi_t the state and pair marginals of sequence b (length L = T in the
 * uniform call),
 *    d_node[b,t,k] = gamma_t[k] (g_logZ[b] + E[phi | z_t = k] - E[phi]),   d_init[b] = d_node[b,0],
 *    d_pair[b,i,j] = sum_{t < L-1} xi_t[i,j] (g_logZ[b] + E[phi | z_t = i, z_{t+1} = j] - E[phi])
 *  (the Hessian of log Z applied to the cotangents of the statistics, plus g_logZ times the statistics).  A -inf
 *  potential has gradient exactly 0; a finite cotangent at a position of probability 0 contributes exactly 0.  A
 *  sequence with log Z = -inf is outside the contract, as for the E-step.
 *  in : init_params (K); pair_params (K,K) or (B,K,K) if pair_batched; node_params (B,T,K);
 *       g_logZ (B), g_init (B,K), g_trans (B,K,K), g_states (B,T,K): each may be NULL = a zero cotangent
 *  out: d_init (B,K), d_pair (B,K,K), d_node (B,T,K), all per sequence: for shared parameters the caller sums d_init
 *       (and d_pair, if not pair_batched) over the batch
 *  Range: the E-step's contract -- every sequence with a path of finite score gets the log-space result to rounding.
 *       The scaled kernels raise a sequence's route flag when a live component of an unnormalised message falls below
 *       1e-250 or a normaliser below 1e-200, in the forward or in the backward sweep; the log-space launch behind them
 *       recomputes those sequences, all of each.
 *  workspace: svae_hmm_estep_vjp_workspace_bytes(B,T,K) = (B T 2 KP + B) doubles rounded up to 128 bytes, KP = 16, 32 or
 *       64 for K <= 16, <= 32, <= 64: per step [a_t | r_t] (on the log-space route log a_t), then B route flags (1.0 =
 *       the sequence was redone in log space); 0 for B <= 0, T <= 0 or K outside 1..SVAE_HMM_MAX_K.  16-byte aligned.
 *  Ragged form (svae_hmm_ragged_estep_vjp_f64, lengths (B) device int32), the conventions of the other ragged entries:
 *    the gradients are those of the sequence cut at L; d_node[b, t >= L] is exactly 0; node_params[b, L:] and
 *    g_states[b, L:] are never read and may be NaN; a length outside 1..T is clamped to [1, T] and ORs 1 into `info`.
 *  Returns 0, or (decided on the host before any HIP call, the first failing check)
 *   both   : -1 B < 0, -2 T < 1, -3 K outside 1..SVAE_HMM_MAX_K, -4 pair_batched not 0 or 1, -5 init_params NULL,
 *            -6 pair_params NULL, [B = 0 returns 0 here], -7 node_params NULL;
 *   uniform: -8 d_init NULL, -9 d_pair NULL, -10 d_node NULL, -11 workspace NULL, -12 ws_bytes too small, -13 workspace
 *            not 16-byte aligned;
 *   ragged : -8 lengths NULL, -9 d_init NULL, -10 d_pair NULL, -11 d_node NULL, -12 info NULL, -13 workspace NULL,
 *            -14 ws_bytes too small, -15 workspace not 16-byte aligned;
 *  -1000 launch error.  Two launches (scaled, log-space redo), asynchronous on `stream`, no internal allocation, safe
 *  under graph capture. */
size_t svae_hmm_estep_vjp_workspace_bytes(int B, int T, int K);
int svae_hmm_estep_vjp_f64(int B, int T, int K, int pair_batched,
                           const double* init_params, const double* pair_params, const double* node_params,
                           const double* g_logZ /* or NULL */, const double* g_init /* or NULL */,
                           const double* g_trans /* or NULL */, const double* g_states /* or NULL */,
                           double* d_init, double* d_pair, double* d_node,
                           void* workspace, size_t ws_bytes, void* stream);
int svae_hmm_ragged_estep_vjp_f64(int B, int T, int K, int pair_batched,
                                  const double* init_params, const double* pair_params, const double* node_params,
                                  const int32_t* lengths,
                                  const double* g_logZ /* or NULL */, const double* g_init /* or NULL */,
                                  const double* g_trans /* or NULL */, const double* g_states /* or NULL */,
                                  double* d_init, double* d_pair, double* d_node,
                                  int32_t* info, void* workspace, size_t ws_bytes, void* stream);

/* Batched HMM E-step with PER-STEP transition potentials (time-inhomogeneous chains: input-driven and recurrent
 * transitions, time-varying priors, per-step expected pair terms), K <= SVAE_HMM_MAX_K -- csrc/hmm_estep_perstep.hip,
 * which states the arithmetic.  Additions to ABI 15 (no new number).  For sequence b of length L (= T without lengths):
 *    log p(z) ∝ init[z_0] + sum_{t<L-1} pair[t][z_t][z_{t+1}] + sum_{t<L} node[b,t][z_t]
 *  in : init_params (K); pair_params (T-1,K,K), [t][j][k] = z_t = j -> z_{t+1} = k, or (B,T-1,K,K) if pair_batched (T = 1
 *       reads no pair parameters: the pointer may then be NULL); node_params (B,T,K); lengths (B) device int32 or NULL =
 *       every sequence has length T
 *  out: logZ (B); E_init (B,K) = the marginal at t = 0; E_states (B,T,K); E_trans (B,T-1,K,K) PER STEP: E_trans[b,t] is the
 *       posterior pairwise marginal of (z_t, z_{t+1}), its rows sum to E_states[b,t] and its columns to E_states[b,t+1] --
 *       or NULL = not wanted (log-normaliser / marginals only): the pass that forms it is skipped and the other three
 *       outputs are bit for bit those of the call with E_trans.
 *  Domain: potentials finite or -inf; one step's matrix may sit at any common offset (it only shifts logZ) and its entries
 *       may lie hundreds of nats below its maximum.  ONE route, log space throughout (a scaled step would pay the same K^2
 *       exponentials per step for exp(P_t - max)): every sequence with finite logZ has the log-space forward-backward's
 *       result to rounding, and there is no fallback to report.  A sequence with logZ = -inf is outside the contract.
 *  Lengths: the conventions of the svae_hmm_ragged_* entries -- L = lengths[b] clamped to [1, T] for addressing and trip
 *       counts, a length outside 1..T ORs 1 into the device word `info` (an atomic; never cleared by the library, never read
 *       on the host); results up to L are those of the sequence cut there; E_states[b, L:] and E_trans[b, L-1:] are exactly
 *       0.0; nothing stored at node steps >= L or pair steps >= L-1 is read (it may be NaN); no sequence sees another's
 *       length or data.
 *  workspace: svae_hmm_perstep_workspace_bytes(B,T,K) = B T K doubles rounded up to 128 bytes (log alpha_t[k], one record of
 *       K doubles per (sequence, step)); 0 for B <= 0, T <= 0 or K outside 1..SVAE_HMM_MAX_K.  16-byte aligned.
 *  Returns 0, or (decided on the host before any HIP call, the first failing check)
 *   -1 B < 0, -2 T < 1, -3 K outside 1..SVAE_HMM_MAX_K, -4 pair_batched not 0 or 1, -5 init_params NULL, -6 pair_params
 *   NULL with T > 1, [B = 0 returns 0 here], -7 node_params NULL, -8 logZ NULL, -9 E_init NULL, -10 E_states NULL,
 *   -11 info NULL with lengths given, -12 workspace NULL, -13 ws_bytes too small, -14 workspace not 16-byte aligned;
 *  -1000 launch error.  One launch, asynchronous on `stream`, no internal allocation, no host synchronisation, safe under
 *  graph capture. */
size_t svae_hmm_perstep_workspace_bytes(int B, int T, int K);
int svae_hmm_perstep_estep_f64(int B, int T, int K, int pair_batched,
                               const double* init_params, const double* pair_params, const double* node_params,
                               const int32_t* lengths /* or NULL */,
                               double* logZ, double* E_init, double* E_trans /* or NULL */, double* E_states,
                               int32_t* info /* NULL only if lengths is */, void* workspace, size_t ws_bytes, void* stream);

/* Reverse-mode derivative of svae_hmm_perstep_estep_f64: the VJP of all four outputs (logZ, E_init, the per-step E_trans,
 * E_states) w.r.t. all three inputs, K <= SVAE_HMM_MAX_K -- csrc/hmm_estep_perstep_vjp.hip.  Additions to ABI 15 (no new
 * number).  Inputs, lengths and the status word as svae_hmm_perstep_estep_f64.
 *  in : cotangents g_logZ (B), g_init (B,K), g_trans (B,T-1,K,K) PER STEP, g_states (B,T,K); each may be NULL = zero
 *  out: PER-SEQUENCE gradients d_init (B,K), d_pair (B,T-1,K,K), d_node (B,T,K), as svae_hmm_estep_vjp_f64: a shared
 *       parameter's gradient is their sum over b, formed by the caller.  d_pair may be NULL = not wanted (the pair
 *       parameters need no gradient): the pass that forms it is skipped and d_init, d_node are bit for bit those of the call
 *       with d_pair.  With g_trans == NULL no V_t is loaded.
 *  Arithmetic, for one sequence of length L, potentials init, P_t = pair[t], node and cotangents g, u0 = g_init,
 *  V_t = g_trans[t], W = g_states; phi(z) = u0[z_0] + sum_t V_t[z_t, z_{t+1}] + sum_t W[t, z_t]; log space throughout:
 *    forward   la_0 = init + node_0                         r_0 = u0 + W[0]
 *              w_t[j,k] = softmax_j(la_t[j] + P_t[j,k])     (0 where the column is all -inf)
 *              la_{t+1}[k] = node_{t+1}[k] + lse_j(la_t[j] + P_t[j,k])
 *              r_{t+1}[k]  = sum_j w_t[j,k] (r_t[j] + V_t[j,k]) + W[t+1,k]
 *    end       logZ = lse_k la_{L-1};  gamma_{L-1} = exp(la_{L-1} - logZ);  E[phi] = sum_k gamma_{L-1}[k] r_{L-1}[k];
 *              c = g - E[phi]
 *    backward  lb_{L-1} = 0, s_{L-1} = 0;   y_{t+1} = W[t+1] + s_{t+1}
 *              q_t[j,k] = softmax_k(P_t[j,k] + node_{t+1}[k] + lb_{t+1}[k])              (0 where the row is all -inf)
 *              lb_t[j] = lse_k(...),   s_t[j] = sum_k q_t[j,k] (V_t[j,k] + y_{t+1}[k]),   gamma_t = exp(la_t + lb_t - logZ)
 *              d_pair[t,j,k] = gamma_t[j] q_t[j,k] (c + r_t[j] + V_t[j,k] + y_{t+1}[k])
 *              d_node[t,k]   = gamma_t[k] (c + r_t[k] + s_t[k]),      d_init = d_node[0]
 *  The softmax weights are the two sweeps' own exponentials (2 K^2 exp per step, as in the E-step); r and s are bounded by
 *  L max|cotangent| and are not scaled; a -inf potential gives exactly 0 in d_pair (the 0-weight convention keeps r and s
 *  finite); the shift of an empty maximum is 0.  ONE route: no flags, nothing redone.  Domain: that of
 *  svae_hmm_perstep_estep_f64; cotangents finite.
 *  Lengths: L = lengths[b] clamped to [1, T], a length outside 1..T ORs 1 into `info` (a vector atomic); the gradients are
 *       those of the sequence cut to L; d_node[b, L:] and d_pair[b, L-1:] are exactly +0.0; nothing at node / g_states steps
 *       >= L or pair / g_trans steps >= L-1 is loaded (it may be NaN); no sequence sees another's length or data.
 *  workspace: svae_hmm_perstep_estep_vjp_workspace_bytes(B,T,K) = B T 2 K doubles rounded up to 128 bytes (the records
 *       [la_t | r_t], 2 K doubles per (sequence, step)); 0 for B <= 0, T <= 0 or K outside 1..SVAE_HMM_MAX_K.  16-byte aligned.
 *  Returns 0, or (decided on the host before any HIP call, the first failing check)
 *   -1 B < 0, -2 T < 1, -3 K outside 1..SVAE_HMM_MAX_K, -4 pair_batched not 0 or 1, -5 init_params NULL, -6 pair_params
 *   NULL with T > 1, [B = 0 returns 0 here], -7 node_params NULL, -8 d_init NULL, -9 d_node NULL, -10 info NULL with
 *   lengths given, -11 workspace NULL, -12 ws_bytes too small, -13 workspace not 16-byte aligned; -1000 launch error.
 *  One launch, asynchronous on `stream`, no internal allocation, no host synchronisation, safe under graph capture. */
size_t svae_hmm_perstep_estep_vjp_workspace_bytes(int B, int T, int K);
int svae_hmm_perstep_estep_vjp_f64(int B, int T, int K, int pair_batched,
                                   const double* init_params, const double* pair_params, const double* node_params,
                                   const int32_t* lengths /* or NULL */,
                                   const double* g_logZ /* (B) or NULL */, const double* g_init /* (B,K) or NULL */,
                                   const double* g_trans /* (B,T-1,K,K) or NULL */, const double* g_states /* (B,T,K) or NULL */,
                                   double* d_init /* (B,K) */, double* d_pair /* (B,T-1,K,K) or NULL */, double* d_node /* (B,T,K) */,
                                   int32_t* info /* NULL only if lengths is */, void* workspace, size_t ws_bytes, void* stream);

/* Viterbi decoding with PER-STEP transition potentials, K <= SVAE_HMM_MAX_K -- csrc/hmm_viterbi_perstep.hip.  Addition to
 * ABI 15 (no new number).  Inputs, lengths and the status word as svae_hmm_perstep_estep_f64; the arithmetic is that of
 * svae_hmm_viterbi_f64 with the step's own matrix, for sequence b of length L (= T without lengths):
 *    delta_0[k] = init[k] + node[0][k]
 *    delta_t[k] = (max_j (delta_{t-1}[j] + pair[t-1][j][k])) + node[t][k]      fp64, the additions in that order
 *    psi_t[k]   = the LOWEST j attaining the maximum
 *    z_{L-1}    = the lowest k attaining max_k delta_{L-1}[k];   z_t = psi_{t+1}[z_{t+1}];   score = delta_{L-1}[z_{L-1}]
 *  Labels and score are reproducible bit for bit (where the reduction over j is split over wavefronts the shares are
 *  combined in ascending j with a strict `>`, which keeps exactly this rule).  A step whose potentials are all -inf gives
 *  score -inf and the labels the lowest-index rule gives; NaN inputs give unspecified labels in 0..K-1 and no fault.
 *  out: states (B,T) int32, states[b, L:] = -1; score (B) or NULL.
 *  Lengths: L clamped to [1,T], a value outside ORs 1 into `info` (a vector atomic); results up to L are those of the
 *       sequence cut there; nothing at node steps >= L or pair steps >= L-1 is loaded; no sequence sees another's length or data.
 *  workspace: at least svae_hmm_viterbi_workspace_bytes(B,T,K) (one back-pointer byte per step and padded state), 16-byte
 *       aligned.
 *  Returns 0, or (decided on the host before any HIP call, the first failing check) -1 B < 0, -2 T < 1, -3 K outside
 *   1..SVAE_HMM_MAX_K, -4 pair_batched not 0 or 1, -5 init_params NULL, -6 pair_params NULL with T > 1, [B = 0 returns 0
 *   here], -7 node_params NULL, -8 states NULL, -9 info NULL with lengths given, -10 workspace NULL, -11 ws_bytes too small,
 *   -12 workspace not 16-byte aligned; -1000 launch error.  One launch, asynchronous on `stream`, no internal allocation,
 *  safe under graph capture. */
int svae_hmm_perstep_viterbi_f64(int B, int T, int K, int pair_batched,
                                 const double* init_params, const double* pair_params, const double* node_params,
                                 const int32_t* lengths /* or NULL */, int32_t* states, double* score /* or NULL */,
                                 int32_t* info /* NULL only if lengths is */, void* workspace, size_t ws_bytes, void* stream);

/* Posterior sampling (forward filter, backward draw) with PER-STEP transition potentials, K <= SVAE_HMM_MAX_K, S >= 1
 * samples per sequence -- csrc/hmm_sample_perstep.hip.  Addition to ABI 15 (no new number).  Inputs, lengths and the status
 * word as svae_hmm_perstep_estep_f64; u (B,S,T) uniforms; out: states (B,S,T) int32, states[b, :, L:] = -1; logZ (B) or NULL.
 * ONE route, log space throughout, as the per-step E-step: no range flags, no second filter launch, nothing redone.
 *    filter: la_0 = init + node_0;  la_{t+1}[k] = node_{t+1}[k] + logsumexp_j(la_t[j] + pair[t][j][k]) -- the forward sweep
 *            of svae_hmm_perstep_estep_f64 itself; its unnormalised records la_t stay in the workspace;
 *            logZ = logsumexp_k la_{L-1}[k], bit for bit the E-step's.
 *    draw:   t = L-1: lw[k] = la_{L-1}[k];   t < L-1: lw[k] = la_t[k] + pair[t][k][z_{t+1}]
 *            m = max_k lw[k], taken as 0 if that is -inf;  w[k] = exp(lw[k] - m)
 *            and from there the selection rule of svae_hmm_sample_f64: C[k] = w[0] + .. + w[k] in index order,
 *            thr = clamp(u,0,1) C[K-1] (a NaN u counts as 0),  z_t = #{k : C[k] <= thr and C[k] < C[K-1]}.
 *  A state with a forbidden (-inf) transition or observation is never drawn; u = 0 draws the lowest allowed state, u = 1 the
 *  highest.  A chain with logZ = -inf or NaN potentials gives unspecified labels in 0..K-1 and affects no other sequence;
 *  every data-dependent index is masked into range before it addresses memory.
 *  Lengths: as above; nothing at node steps >= L, pair steps >= L-1 or u steps >= L is loaded.
 *  workspace: at least svae_hmm_perstep_workspace_bytes(B,T,K) (the E-step's la_t records), 16-byte aligned.
 *  Returns 0, or (decided on the host before any HIP call, the first failing check) -1 .. -7 as svae_hmm_perstep_viterbi_f64,
 *   -8 S < 1, -9 u NULL, -10 states NULL, -11 info NULL with lengths given, -12 workspace NULL, -13 ws_bytes too small,
 *   -14 workspace not 16-byte aligned; -1000 launch error.  Two launches (filter, draw), asynchronous on `stream`, no
 *  internal allocation, safe under graph capture. */
int svae_hmm_perstep_sample_f64(int B, int T, int K, int S, int pair_batched,
                                const double* init_params, const double* pair_params, const double* node_params,
                                const int32_t* lengths /* or NULL */, const double* u,
                                int32_t* states, double* logZ /* or NULL */,
                                int32_t* info /* NULL only if lengths is */, void* workspace, size_t ws_bytes, void* stream);

/* HMM step of the SLDS coordinate ascent on the rows `seq_index` lists (B of `rows`; NULL: rows 0..B-1; negative
 * entries = unused slots, which must follow the live ones -- the list svae_slds_sweep_glue_f64 writes):
 *   hmm_meanfield + get_arhmm_local_nodeparams   /root/reference/svae/models/slds_svae.py:108-115, 131-147
 * Node log-potentials: `node_params` (rows,T,K) if given; else built on the fly from the outputs of
 * svae_slds_lds_meanfield_f64 --  node[b,0,k] = <E x_0 x_0', init_J_k> + <E x_0, init_h_k> + cinit_k  (lds_E_init
 * (rows, n*n+n), init_J (K,n,n), init_h (K,n), cinit (K) = the init potential's constants),
 * node[b,t,k] = pair_contr[b,t-1,0,k] + pair_contr[b,t,1,k] + lz_k  (t >= 1; lz (K) = the pair potentials' constants).
 * Outputs as svae_hmm_estep_f64, written at the listed rows only; node_out (rows,T,K) or NULL: the potentials used. */
int svae_slds_hmm_meanfield_f64(int B, int rows, int T, int K, int n,
                                const double* hmm_init, const double* hmm_pair, const double* node_params,
                                const double* pair_contr, const double* lds_E_init, const double* init_J,
                                const double* init_h, const double* cinit, const double* lz,
                                const int32_t* seq_index,
                                double* logZ, double* E_init, double* E_trans, double* E_states,
                                double* node_out, void* workspace, size_t ws_bytes, void* stream);

/* End of one sweep of the SLDS coordinate ascent (optimize_local_meanfield, slds_svae.py:159-175), after the HMM and the
 * fused LDS kernels, for the B listed rows:  lds_vlb = lognorm + <E z_0, cinit> + sum_{t>=1} <E z_t, lz>;
 * vlb_new = hmm_vlb + lds_vlb;  iters += 1;  the row keeps iterating unless |vlb_new - vlb| < tol (:170-172);  vlb = vlb_new.
 * next_index (B) / next_count (1): the rows still iterating, in the order of `seq_index` (a different buffer), padded
 * with -1 up to B: the next sweep may be launched on B slots before the host has read next_count (negative slots are
 * skipped by the three kernels of a sweep).
 * keep_scratch: B int32.  No host arithmetic is needed between two sweeps (the caller reads next_count to size them). */
int svae_slds_sweep_glue_f64(int B, int T, int K, double tol, const int32_t* seq_index,
                             const double* E_states, const double* cinit, const double* lz,
                             const double* lognorm, const double* hmm_vlb, double* lds_vlb, double* vlb,
                             int32_t* iters, int32_t* keep_scratch, int32_t* next_index, int32_t* next_count,
                             void* stream);

/* The two dense contractions at the ends of the ascent, as kernels (they were library GEMMs over materialised outer
 * products / per-step parameter blocks):
 *   initialize_local_meanfield + get_arhmm_local_nodeparams  /root/reference/svae/models/slds_svae.py:203-226, 131-147
 *     HMM node potentials of sweep 0 from ONE sample path x (B,T,n):  node[b,0,k] = x_0' init_J_k x_0 + init_h_k' x_0 +
 *     cinit_k;  node[b,t,k] = x_{t-1}' J11_k x_{t-1} + x_{t-1}' J12_k x_t + x_t' J22_k x_t + lz_k  (t >= 1).  n <= 15.
 *   get_var_lds_local_natparam (the pair part)               /root/reference/svae/models/slds_svae.py:92-103
 *     out_J11/J12/J22 (B,T-1,n,n), out_logZ (B,T-1):  out[b,t] = sum_k E_states[b,t+1,k] P_k.
 * Parameter blocks carry a leading K axis (K <= 16). */
int svae_slds_path_nodeparams_f64(int B, int T, int K, int n, const double* x, const double* init_J,
                                  const double* init_h, const double* cinit, const double* J11, const double* J12,
                                  const double* J22, const double* lz, double* node_out, void* stream);
int svae_slds_mix_pair_natparam_f64(int B, int T, int K, int n, const double* E_states, const double* J11,
                                    const double* J12, const double* J22, const double* lz, double* out_J11,
                                    double* out_J12, double* out_J22, double* out_logZ, void* stream);

/* The two contractions of the SLDS final pass (run_inference, /root/reference/svae/models/slds_svae.py:289-310) over the
 * per-step pair statistics pair_stats (B,T-1,3,n,n) of the last LDS E-step, in ONE pass over them:
 *   get_arhmm_local_nodeparams :131-147   node_out[b,t+1,k] = <pair_stats[b,t], P_k> + lz_k   (rows 1..T-1 of (B,T,K);
 *                                         row 0 -- the init statistics -- is the caller's)
 *   get_global_stats :229-243             sum_{b,t} weights[b,t+1,k] pair_stats[b,t]: `blocks` partial sums
 *                                         gpart (blocks, 8, 3 n^2), to be added in index order (rows k >= K are zero)
 * P (K, 3 n^2) = [J11_k | J12_k | J22_k] flattened, lz (K), weights (B,T,K) = the HMM marginals.  n <= 10, K <= 8, T >= 2. */
int svae_slds_pair_contract_f64(int B, int T, int K, int n, const double* pair_stats, const double* P, const double* lz,
                                const double* weights, double* node_out, double* gpart, int blocks, void* stream);

/* GMM mean-field fixed point + global statistics for one minibatch of T points
 * [local_meanfield, /root/reference/svae/models/gmm.py:62-88; meanfield_fixed_point :90-110;
 *  gaussian_meanfield :112-117; label_meanfield :119-124].
 *
 *  in : label_global (K)             = dirichlet.expectedstats(dirichlet natparam)
 *       gaussian_globals (K,N+2,N+2) = niw.expectedstats(niw natparams), dense-packed
 *       node_J (T,N) diagonal -1/2 precision, node_h (T,N)      (the recognition potentials)
 *       label_init (T,K)  initial responsibilities (reference: normalize(rand(T,K)), gmm.py:126-128)
 *       tol, max_iter     (reference: 1e-3, 100); the stop rule is on the batch-total KL
 *  out: label_stats (T,K) responsibilities at the fixed point (after the final extra pass, :74-77)
 *       label_fixed (T,K) or NULL: the fixed point itself, i.e. what that final pass started from
 *         (:71; callers that keep the final pass on an autograd tape re-run it from here)
 *       gaussian_stats (T,N+2,N+2) dense-packed E[t(x_t)]
 *       label_natparam (T,K), gaussian_natparam (T,N+2,N+2)
 *       dirichlet_stats (K), niw_stats (K,N+2,N+2)      (sums over points, :80-81)
 *       kl (1) = label_kl + gaussian_kl (:86),  iters (1) number of fixed-point iterations run
 *       assign (T) int32 argmax_k label_stats
 *       info (1) int32 status word, untouched on valid input: t + 1 of the LOWEST point t whose Gaussian factor met a
 *         non-positive pivot or whose KL term is not finite (a NaN or infinite potential passes every pivot test)
 *  Limits: N <= 8, K <= 64.  Single workgroup (the minibatch total KL is a block reduction).
 */
int svae_gmm_meanfield_f64(int T, int N, int K,
                           const double* label_global, const double* gaussian_globals,
                           const double* node_J, const double* node_h, const double* label_init,
                           double tol, int max_iter,
                           double* label_stats, double* label_fixed, double* gaussian_stats,
                           double* label_natparam, double* gaussian_natparam,
                           double* dirichlet_stats, double* niw_stats,
                           double* kl, int32_t* iters, int32_t* assign,
                           int32_t* info, void* stream);

/* The same fixed point spread over MANY workgroups -- and, through the caller's all-reduce, over many GPUs --
 * with the reference's stopping rule on the batch-total KL (/root/reference/svae/models/gmm.py:104-105)
 * kept exact: one launch per sweep, each ending in a fixed-order reduction of its workgroups' KL partials
 * into kl_hist[sweep] (first max_iter+1 doubles of the workspace; svae_gmm_mw_kl_hist); every launch first
 * scans kl_hist for an earlier sweep that met |kl_j - kl_{j-1}| < tol and is a no-op if there is one, so the
 * host enqueues max_iter sweeps blindly, with no synchronisation.  Multi-GPU (points sharded over ranks):
 * all-reduce kl_hist[sweep] in place after each sweep launch -- every rank then takes the same decision.
 *   svae_gmm_mw_begin     zeroes the state (once per fixed point)
 *   svae_gmm_mw_step_f64  phase 0: sweep number `sweep`; phase 1: the final pass of gmm.py:74-86 (writes
 *                         every per-point output, kl = this rank's total, iters); phase 2: the global
 *                         statistics (dirichlet_stats, niw_stats of this rank's points).
 * Arguments as svae_gmm_meanfield_f64.  Results agree with the single-workgroup kernel up to the summation
 * order of the KL total (same per-point arithmetic: identical labels unless a sweep sits on the tolerance). */
size_t svae_gmm_mw_workspace_bytes(int T, int N, int K, int max_iter);
int svae_gmm_mw_begin(int T, int N, int K, int max_iter, void* workspace, size_t ws_bytes, void* stream);
int svae_gmm_mw_step_f64(int phase, int sweep, int T, int N, int K,
                         const double* label_global, const double* gaussian_globals,
                         const double* node_J, const double* node_h,
                         const double* label_init, double tol, int max_iter,
                         double* label_stats, double* label_fixed, double* gaussian_stats,
                         double* label_natparam, double* gaussian_natparam,
                         double* dirichlet_stats, double* niw_stats,
                         double* kl, int32_t* iters, int32_t* assign, int32_t* info,
                         void* workspace, size_t ws_bytes, void* stream);
double* svae_gmm_mw_kl_hist(void* workspace);
/* Single GPU: the same sweeps, final pass and statistics as svae_gmm_mw_begin + max_iter x phase 0 + phase 1 + phase 2,
 * in ONE plain launch (+ the statistics launch): per sweep the workgroups exchange their KL partials as data-tagged
 * 8-byte agent-scope words (no grid barrier, no atomics read-modify-write, no cooperative launch), every workgroup sums
 * them in index order and takes the same stopping decision; with at most one point per thread and K <= 16 the
 * responsibilities stay in registers for the whole fixed point.  Removes the 16-21 us per-sweep launch cost that bounds
 * the fixed point below ~100 k points.  Same results as the per-sweep calls, bit for bit.  Every spin is bounded: a
 * workgroup that never sees a partner's partial sets *info = -77.  Returns -50 only when the device cannot be queried. */
int svae_gmm_mw_fixed_point_f64(int T, int N, int K,
                                const double* label_global, const double* gaussian_globals,
                                const double* node_J, const double* node_h,
                                const double* label_init, double tol, int max_iter,
                                double* label_stats, double* label_fixed, double* gaussian_stats,
                                double* label_natparam, double* gaussian_natparam,
                                double* dirichlet_stats, double* niw_stats,
                                double* kl, int32_t* iters, int32_t* assign, int32_t* info,
                                void* workspace, size_t ws_bytes, void* stream);


/* ---- GMM-SVAE local step, differentiable tail (csrc/gmm_train.hip) -------------------------------------------
 * Replaces /root/reference/svae/distributions/gaussian.py:27-33 (`natural_sample`) and autograd's reverse pass
 * through /root/reference/svae/models/gmm.py:74-86 + gmm.py:12-16 (`run_inference`: samples and local_kl are what
 * svae.py:21-30 differentiates w.r.t. the recognition network's node potentials).
 *   svae_gmm_sample_f64     samples[t,s,:] = J_t^-1 h_t + chol(J_t)^-T eps[t,s,:], (J_t, h_t) unpacked from the
 *                           dense (N+2)x(N+2) gaussian_natparam[t] the fixed-point kernels return.
 *   svae_gmm_local_vjp_f64  cotangents of the node potentials (g_node_J, g_node_h: (T,N)) given g_kl (device scalar,
 *                           cotangent of the final pass's local KL; NULL = 0) and g_samples ((T,S,N); NULL = none,
 *                           then eps may be NULL).  gaussian_natparam / label_natparam: the final pass's outputs.
 * One point per lane, N <= 8, K <= 64; device pointers, asynchronous on `stream`.  0 / -k (argument k).
 *   svae_gmm_global_step_f64  the global side of a step in ONE launch: label_global (K) = dirichlet.expectedstats
 *                           (dirichlet.py:5-7), gaussian_globals (K,N+2,N+2) = niw.expectedstats (niw.py:15-25) -- the two
 *                           potentials svae_gmm_meanfield_f64 / svae_gmm_mw_* take -- and, if `kl` (TWO doubles, ABI 12) is
 *                           given, the prior KL of gmm.py:54-58: kl[0] as the code spells it (full contraction;
 *                           dirichlet.logZ, niw.logZ), kl[1] as the reference AS SHIPPED evaluates it (util.py:39 `flat`
 *                           after util.py:166 rebinds `flatten`: the contraction keeps its first term only).  *info is
 *                           raised to 1 on invalid parameters of the global factor or the prior: a non-positive-definite
 *                           NIW scale matrix, kappa <= 0, nu <= N - 1, a Dirichlet alpha <= 0. */
int svae_gmm_global_step_f64(int K, int N, const double* dirichlet_natparam, const double* niw_natparam,
                             const double* prior_dirichlet, const double* prior_niw,
                             double* label_global, double* gaussian_globals, double* kl, int32_t* info, void* stream);
int svae_gmm_sample_f64(int T, int N, int S, const double* gaussian_natparam, const double* eps,
                        double* samples, void* stream);
int svae_gmm_local_vjp_f64(int T, int N, int K, int S, const double* label_global,
                           const double* gaussian_globals, const double* node_J, const double* node_h,
                           const double* gaussian_natparam, const double* label_natparam,
                           const double* g_kl, const double* eps, const double* g_samples,
                           double* g_node_J, double* g_node_h, void* stream);

/* ---- GMM-SVAE local step for latent dimensions up to 16 (csrc/gmm_wide.hip) ---------------------------------------
 * One 16-lane row per point (lane i: row i of the point's J, Sigma, E[x x'] and Cholesky factor), the K <= 64
 * responsibilities spread over the row.  Each entry takes the argument list of its N <= 8 counterpart above, accepts
 * 1 <= N <= 16 (so it can be checked against the N <= 8 kernels) and returns the same code for the same bad argument;
 * an N outside 1..16 gets the counterpart's code for N > 8.  Arguments are checked before any HIP call.
 *   svae_gmm_wide_mw_workspace_bytes / _mw_begin / _mw_step_f64   the per-sweep fixed point of svae_gmm_mw_*: phase 0
 *       sweep `sweep`, phase 1 the final pass, phase 2 the global statistics; kl_hist stays at the start of the
 *       workspace (svae_gmm_mw_kl_hist applies), sweeps after the stopping rule fired are device-side no-ops.
 *   svae_gmm_wide_sample_f64      as svae_gmm_sample_f64.
 *   svae_gmm_wide_local_vjp_f64   as svae_gmm_local_vjp_f64 (two launches when g_samples is given).
 *   svae_gmm_wide_global_step_f64 as svae_gmm_global_step_f64 (one row per component). */
size_t svae_gmm_wide_mw_workspace_bytes(int T, int N, int K, int max_iter);
int svae_gmm_wide_mw_begin(int T, int N, int K, int max_iter, void* workspace, size_t ws_bytes, void* stream);
int svae_gmm_wide_mw_step_f64(int phase, int sweep, int T, int N, int K,
                              const double* label_global, const double* gaussian_globals,
                              const double* node_J, const double* node_h,
                              const double* label_init, double tol, int max_iter,
                              double* label_stats, double* label_fixed, double* gaussian_stats,
                              double* label_natparam, double* gaussian_natparam,
                              double* dirichlet_stats, double* niw_stats,
                              double* kl, int32_t* iters, int32_t* assign, int32_t* info,
                              void* workspace, size_t ws_bytes, void* stream);
int svae_gmm_wide_sample_f64(int T, int N, int S, const double* gaussian_natparam, const double* eps,
                             double* samples, void* stream);
int svae_gmm_wide_local_vjp_f64(int T, int N, int K, int S, const double* label_global,
                                const double* gaussian_globals, const double* node_J, const double* node_h,
                                const double* gaussian_natparam, const double* label_natparam,
                                const double* g_kl, const double* eps, const double* g_samples,
                                double* g_node_J, double* g_node_h, void* stream);
int svae_gmm_wide_global_step_f64(int K, int N, const double* dirichlet_natparam, const double* niw_natparam,
                                  const double* prior_dirichlet, const double* prior_niw,
                                  double* label_global, double* gaussian_globals, double* kl, int32_t* info,
                                  void* stream);


/* ---- one-shot all-reduce of a small buffer over IPC-mapped mailboxes (csrc/ipc_allreduce.hip) -----------------------
 * The exchange step (/root/reference/svae/svae.py:33-34: the batch-summed statistics) as ONE kernel: every rank stores
 * its n doubles, as tagged 8-byte words, into slot `rank` of EVERY rank's mailbox (fine-grained device memory of
 * svae_ipc_mailbox_bytes(capacity, world) bytes, zero-initialised once, IPC-mapped into every peer: mailboxes[q] = rank
 * q's mailbox as mapped into this process), then sums the words that arrived in its own mailbox in rank order -> out
 * (may alias in).  `capacity` (doubles) fixes the mailbox layout for its lifetime -- the same on every rank and in every
 * call; a call may reduce any n <= capacity, and consecutive calls may differ in n (ABI 12).  epoch: 1, 2, 3, .. per
 * call, the same on every rank.  Bit-identical results on every rank.  spin_limit: polls per word before a peer counts
 * as absent (0 = 2^28, minutes); an element whose words never arrive comes out as NaN and *info = -78 -- a timeout never
 * passes for a sum.  world <= 16.  Opt-in alternative to the RCCL all-reduce (svae_amd/ipc.py).
 * Returns 0 / -k (argument k). */
size_t svae_ipc_mailbox_bytes(int capacity, int world);
int svae_ipc_allreduce_f64(int n, int capacity, int rank, int world, unsigned epoch, unsigned spin_limit,
                           const double* in, double* out, void* const* mailboxes, int32_t* info, void* stream);

/* ---- The reference's three reverse-mode primitives, on caller-held forward messages (n <= SVAE_LDS_MAX_N) ----
 * Each differentiates the reference's recursion as a function of the forward messages (J_pred, h_pred, J_filt, h_filt)
 * (B,T,n,n) / (B,T,n) -- natural scaling, J = -1/2 precision, as svae_lds_filter_f64 writes them -- and rebuilds every
 * per-step factor from them (no record of an earlier call).  Pair parameters J11, J12, J22 as in svae_lds_estep_f64:
 * (n,n), per step (T-1,n,n) with inhomog, per sequence and step (B,T-1,n,n) with pair_batched.  All cotangents in the
 * reference's scaling and index order.  info (int32, may be NULL): bit 0 is OR-ed in when a pivot is not positive
 * definite.  Return values: 0; -1 B < 0; -2 T < 1; -3 n outside 1..SVAE_LDS_MAX_N; -4 bad S; -5 NULL pair parameter
 * (T > 1); -6 NULL message; -7 pair_batched without inhomog; -8 NULL required cotangent input; -9 NULL output;
 * -14 workspace NULL or too small; -1000 launch error.  Arguments are checked before any HIP call. */

/* natural_filter_grad (/root/reference/svae/lds/cython_lds_inference.pyx:92-145, helpers
 * cython_gaussian_grads.pxd:17-206): the cotangent of the node potentials given cotangents of the filter's outputs.
 *  in : J11, J12; J_filt, h_filt; g_J_pred, g_J_filt (B,T,n,n), g_h_pred, g_h_filt (B,T,n), g_lognorm (B)
 *  out: g_node_J (B,T,n) (diagonal node potentials), g_node_h (B,T,n), g_node_logZ (B,T) */
int svae_lds_filter_vjp_f64(int B, int T, int n, int inhomog, int pair_batched,
                            const double* J11, const double* J12,
                            const double* J_filt, const double* h_filt,
                            const double* g_J_pred, const double* g_h_pred,
                            const double* g_J_filt, const double* g_h_filt, const double* g_lognorm,
                            double* g_node_J, double* g_node_h, double* g_node_logZ,
                            int32_t* info, void* stream);

/* Bytes of workspace svae_lds_smoother_vjp_f64 needs: B * T * (3 n^2 + 2 n) * 8 (per sequence-step the smoothed
 * Js, Cov[x_t], E[x_t+1 x_t'] and hs, E[x_t] of the RTS recursion); 0 for invalid sizes. */
size_t svae_lds_smoother_vjp_workspace_bytes(int B, int T, int n);

/* natural_smoother_general_grad (/root/reference/svae/lds/cython_lds_inference.pyx:236-306, _compute_stats_grad :212-234,
 * helpers cython_gaussian_grads.pxd:208-430): cotangents of the four message arrays given cotangents of the statistics.
 *  in : J11, J12, J22; the four messages; each of g_E_init (B, n*n+n) [E[x0 x0'] | E[x0]], g_E_pair ((B,3,n,n) for
 *       homogeneous pair parameters -- the summed statistics -- else (B,T-1,3,n,n)), g_E_node_diagxx, g_E_node_x (B,T,n)
 *       may be NULL (zero)
 *  out: g_J_pred, g_J_filt (B,T,n,n), g_h_pred, g_h_filt (B,T,n); g_J_pred[:,0] = g_h_pred[:,0] = 0 */
int svae_lds_smoother_vjp_f64(int B, int T, int n, int inhomog, int pair_batched,
                              const double* J11, const double* J12, const double* J22,
                              const double* J_pred, const double* h_pred,
                              const double* J_filt, const double* h_filt,
                              const double* g_E_init, const double* g_E_pair,
                              const double* g_E_node_diagxx, const double* g_E_node_x,
                              double* g_J_pred, double* g_h_pred, double* g_J_filt, double* g_h_filt,
                              int32_t* info, void* workspace, size_t ws_bytes, void* stream);

/* natural_sample_backward_grad (/root/reference/svae/lds/cython_lds_inference.pyx:357-409, helpers
 * cython_gaussian_grads.pxd:456-530): cotangents of the messages given the cotangent of the samples.
 *  in : J11, J12; J_filt, h_filt; eps, samples, g_samples (B,T,S,n) with eps[:,t] the noise applied at step t, 1 <= S <= 16
 *       (larger S: -4)
 *  out: g_J_filt (B,T,n,n), g_h_filt (B,T,n); g_J_pred, g_h_pred written with zeros */
int svae_lds_sample_vjp_f64(int B, int T, int n, int S, int inhomog, int pair_batched,
                            const double* J11, const double* J12,
                            const double* J_filt, const double* h_filt,
                            const double* eps, const double* samples, const double* g_samples,
                            double* g_J_pred, double* g_h_pred, double* g_J_filt, double* g_h_filt,
                            int32_t* info, void* stream);

/* ---- Variable-length sequences in one batch: per-sequence lengths, n <= SVAE_LDS_MAX_N (csrc/lds_estep.hip) -----------
 * The reference runs one sequence per call (natural_filter_forward_general svae/lds/cython_lds_inference.pyx:28-90,
 * natural_smoother_general + _compute_stats :149-210, natural_sample_backward :310-355), so every sequence there has its
 * own length; these entries give the batch axis the same freedom: `lengths` (B) int32 on the device, sequence b occupying
 * steps 0 .. lengths[b]-1 of its (T, n) rows.  Pair and init parameters shared by the batch ((n,n) blocks; `inhomog` and
 * `pair_batched` must be 0), diagonal node potentials (B,T,n).
 *
 * Sequence b of length L runs as a chain of T steps whose pairs t <= L-2 carry the real (J11, J12, J22, logZ) and whose
 * pairs t >= L-1 carry the decoupling set Q = (0, 0, -1/2 I, 0), with zero node potentials from step L on: the tail is a
 * chain of independent standard normals, detached from the real steps -- the last real node sees no J11 term, every tail
 * step adds exactly 0 to the log-normaliser -- so all rows of a wavefront keep one trip count.  (Padding with zero node
 * potentials and the REAL pair parameters is not exact: an expected-statistics pair potential is no normalised conditional.)
 * The kernels are the ragged instantiations of the packed one-directional E-step, samplers and VJP sweeps: the pair blocks
 * come from two-entry tables [real | Q], entry (t <= lengths[b]-2 ? 0 : 1) per row; one route at every batch size.
 *
 * Contract, per sequence b with L = lengths[b]: lognorm[b], E_init[b], E_pair[b] (3,n,n: the sums over the sequence's own
 * L-1 pairs; all zero for L = 1), E_node_*[b,:L], samples[b,:L] (for eps[b,:L]) and g_node_*[b,:L] are those of the
 * sequence truncated to L steps; every output and gradient at t >= L is 0; node_*[b,L:], eps[b,L:] and the cotangents at
 * t >= L are never used (they may be NaN); no result of sequence b depends on another sequence's length.
 * A length outside 1..T is device data: it raises the status word `info` (b+1, like a non-positive pivot) and is clamped
 * to 1..T for addressing.
 *
 * Workspace: the layout of svae_lds_workspace_bytes(B,T,n), then (256-byte aligned) the pair tables, 6 n^2 doubles. */
size_t svae_lds_ragged_workspace_bytes(int B, int T, int n);

/* svae_lds_estep_f64 with per-sequence lengths.  keep: bit 0 the factor region (sampler), bit 1 the cross moments (VJP).
 * options: a valid SVAE_OPT_* word (-24 otherwise); it selects nothing here.  Returns 0, or before any HIP call: -1 B,
 * -2 T, -3 n outside 1..SVAE_LDS_MAX_N, -32 inhomog / pair_batched, -31 lengths NULL, -23 keep, -6.. -21 NULL pointers as
 * svae_lds_estep_f64, -24 options, -22 workspace NULL or shorter than svae_lds_ragged_workspace_bytes; B = 0 returns 0
 * after the checks up to options. */
int svae_lds_ragged_estep_f64(int B, int T, int n, int inhomog, int pair_batched, int keep, unsigned options,
                              const double* init_J, const double* init_h, const double* init_logZ,
                              const double* J11, const double* J12, const double* J22, const double* logZ_pair,
                              const double* node_J, const double* node_h, const double* node_logZ,
                              const int32_t* lengths,
                              double* lognorm, double* E_init, double* E_pair,
                              double* E_node_diagxx, double* E_node_x,
                              int32_t* info, void* workspace, size_t ws_bytes, void* stream);

/* svae_lds_inference_f64 with per-sequence lengths: the ragged E-step keeping the factor (S > 0) and, keep_vjp = 1, the
 * cross moments, then the ragged sampler.  Full per-step records at every batch size.  Error codes of
 * svae_lds_ragged_estep_f64; -4 for S < 0 or S > 0 without eps / samples; -23 keep_vjp outside {0, 1}. */
int svae_lds_ragged_inference_f64(int B, int T, int n, int S, int inhomog, int pair_batched, int keep_vjp, unsigned options,
                                  const double* init_J, const double* init_h, const double* init_logZ,
                                  const double* J11, const double* J12, const double* J22, const double* logZ_pair,
                                  const double* node_J, const double* node_h, const double* node_logZ,
                                  const int32_t* lengths, const double* eps, double* samples,
                                  double* lognorm, double* E_init, double* E_pair,
                                  double* E_node_diagxx, double* E_node_x,
                                  int32_t* info, void* workspace, size_t ws_bytes, void* stream);

/* The VJP sweeps (svae_lds_estep_vjp_ex_f64) w.r.t. the node potentials on the records of the last
 * svae_lds_ragged_estep_f64 (keep = 3) / svae_lds_ragged_inference_f64 (keep_vjp = 1) call with the same (B,T,n) and
 * `lengths`; the J12 table is read from `workspace`.  Cotangents of lognorm (B), E_node_diagxx / E_node_x (B,T,n or NULL)
 * and samples (B,T,S,n or NULL, S <= 16, with eps and samples).  g_node_logZ[b,t] = g_lognorm[b] for t < lengths[b], else 0
 * (host side).  Returns 0, or before any HIP call: -1, -2, -3, -32, -31 as above, -4 S, -6 g_lognorm, -10 eps / samples,
 * -12 / -13 outputs, -24 options, -14 workspace short, -16 vjp_workspace shorter than svae_lds_vjp_workspace_bytes. */
int svae_lds_ragged_vjp_f64(int B, int T, int n, int S, int inhomog, int pair_batched, unsigned options,
                            const double* g_lognorm, const double* g_E_node_diagxx, const double* g_E_node_x,
                            const double* g_samples, const double* eps, const double* samples,
                            const int32_t* lengths, double* g_node_J, double* g_node_h,
                            const void* workspace, size_t ws_bytes,
                            void* vjp_workspace, size_t vjp_ws_bytes, void* stream);

/* svae_lds_reduce_stats_f64 for a ragged batch: the same fixed-order sums and one more slot, the number of pairs behind the
 * E_pair sums (the uniform consumers derive it as count (T-1), which is wrong here):
 *   out (4 n^2 + n + 3) = [sum_b E_init | sum_b E_pair | sum_b lognorm | B | sum_b (lengths[b] - 1)]
 * (lengths clamped to 1..T; integer sum, exact).  -1 B, -7 T, -2 n outside 1..SVAE_LDS_MAX_N, -3.. -6 NULL pointers as
 * svae_lds_reduce_stats_f64, -31 lengths NULL. */
int svae_lds_ragged_reduce_stats_f64(int B, int T, int n, const double* E_init, const double* E_pair,
                                     const double* lognorm, const int32_t* lengths, double* out, void* stream);

/* svae_lds_natgrad_f64 on the (all-reduced) buffer of svae_lds_ragged_reduce_stats_f64: the MNIW count is the buffer's
 * last slot, not count (T-1). */
int svae_lds_ragged_natgrad_f64(int n, const double* packed_stats, const double* prior_flat,
                                const double* params_flat, double num_batches, double scale,
                                double* natgrad_flat, void* stream);

/* ---- Per-sequence lengths with PER-STEP pair parameters, n <= SVAE_LDS_MAX_N (csrc/lds_estep.hip) -----------------------
 * What the SLDS needs from the LDS side for a ragged batch: the construction above -- sequence b of length L = lengths[b]
 * is the chain whose pairs t <= L-2 carry the real parameters and whose pairs t >= L-1 carry Q = (0, 0, -1/2 I, 0), zero node
 * potentials from step L on -- with pair parameters that differ from step to step, (T-1,n,n) and (T-1), or, pair_batched = 1,
 * from sequence to sequence as well, (B,T-1,n,n) and (B,T-1); and with the init potential shared, (n,n), (n), (1), or,
 * init_batched = 1, one per sequence, (B,n,n), (B,n), (B).  The kernel is the INHOMOG + RAG instantiation of the packed
 * one-directional E-step: per step a pointer select between the caller's block of pair t and a table [0 | -1/2 I] that a
 * one-workgroup kernel leaves behind the uniform workspace layout.
 *
 * Contract, per sequence b with L = lengths[b]: lognorm[b], E_init[b], E_pair[b,:L-1] (per-step blocks (3,n,n)),
 * E_node_*[b,:L] and samples[b,:L] (for eps[b,:L]) are those of the sequence cut at L steps -- pair parameters [:L-1], node
 * potentials [:L], logZ_pair summed over t <= L-2 and node_logZ over t < L; E_pair[b,L-1:], E_node_*[b,L:] and
 * samples[b,L:] are 0; J11 / J12 / J22 / logZ_pair at t >= L-1 (any sequence's with pair_batched = 0 only through another
 * sequence's longer length), node_*[b,L:] and eps[b,L:] are never read (they may be NaN); no result of sequence b depends on
 * another sequence's length.  A length outside 1..T raises the status word `info` (b+1) and is clamped to 1..T for
 * addressing.  The reverse sweeps run on the records of svae_lds_ragged_perstep_inference_keep_f64 (keep_vjp = 1):
 * svae_lds_ragged_perstep_vjp_f64 below; the records of the two entries without keep_vjp carry no cross moments.
 *
 * Workspace: the layout of svae_lds_workspace_bytes(B,T,n), then (256-byte aligned) the table, 2 n^2 doubles. */
size_t svae_lds_ragged_perstep_workspace_bytes(int B, int T, int n);

/* keep: 0, or 1 = keep the factor region for the sampler; bit 1 (the VJP's cross moments) is refused.  options: a valid
 * SVAE_OPT_* word; it selects nothing here.  Returns 0, or before any HIP call: -1 B, -2 T, -3 n outside
 * 1..SVAE_LDS_MAX_N, -32 pair_batched / init_batched outside {0, 1}, -31 lengths NULL, -23 keep, -6 init_J, -7 init_h,
 * -8 init_logZ, -9 a pair array NULL with T > 1, -13 node_J, -14 node_h, -16 lognorm, -17 E_init, -18 E_pair (T > 1),
 * -19 E_node_diagxx, -20 E_node_x, -21 info, -24 options, -22 workspace NULL or shorter than
 * svae_lds_ragged_perstep_workspace_bytes; B = 0 returns 0 after the checks up to options. */
int svae_lds_ragged_perstep_estep_f64(int B, int T, int n, int pair_batched, int init_batched, int keep, unsigned options,
                                      const double* init_J, const double* init_h, const double* init_logZ,
                                      const double* J11, const double* J12, const double* J22, const double* logZ_pair,
                                      const double* node_J, const double* node_h, const double* node_logZ,
                                      const int32_t* lengths,
                                      double* lognorm, double* E_init, double* E_pair,
                                      double* E_node_diagxx, double* E_node_x,
                                      int32_t* info, void* workspace, size_t ws_bytes, void* stream);

/* The E-step above (keeping the factor region whenever S > 0), then the ragged sampler of svae_lds_ragged_inference_f64 on
 * its records: full per-step records at every batch size, any S that entry covers.  Error codes of
 * svae_lds_ragged_perstep_estep_f64; -4 for S < 0 or S > 0 without eps / samples. */
int svae_lds_ragged_perstep_inference_f64(int B, int T, int n, int S, int pair_batched, int init_batched, unsigned options,
                                          const double* init_J, const double* init_h, const double* init_logZ,
                                          const double* J11, const double* J12, const double* J22, const double* logZ_pair,
                                          const double* node_J, const double* node_h, const double* node_logZ,
                                          const int32_t* lengths, const double* eps, double* samples,
                                          double* lognorm, double* E_init, double* E_pair,
                                          double* E_node_diagxx, double* E_node_x,
                                          int32_t* info, void* workspace, size_t ws_bytes, void* stream);

/* svae_lds_ragged_perstep_inference_f64 with keep_vjp: keep_vjp = 1 keeps the factor region AND the cross moments W~_t of
 * all T steps (the KEEPW instantiation of the kernel: a compile-time property, not a branch), then runs the ragged sampler
 * when S > 0; the records of steps t >= L are those of the decoupled tail, finite.  keep_vjp = 0 is
 * svae_lds_ragged_perstep_inference_f64.  The forward outputs are the same bits either way.  Error codes of that entry;
 * -23 keep_vjp outside {0, 1}. */
int svae_lds_ragged_perstep_inference_keep_f64(int B, int T, int n, int S, int pair_batched, int init_batched, int keep_vjp,
                                               unsigned options,
                                               const double* init_J, const double* init_h, const double* init_logZ,
                                               const double* J11, const double* J12, const double* J22, const double* logZ_pair,
                                               const double* node_J, const double* node_h, const double* node_logZ,
                                               const int32_t* lengths, const double* eps, double* samples,
                                               double* lognorm, double* E_init, double* E_pair,
                                               double* E_node_diagxx, double* E_node_x,
                                               int32_t* info, void* workspace, size_t ws_bytes, void* stream);

/* The VJP sweeps w.r.t. the node potentials on the records of the last svae_lds_ragged_perstep_inference_keep_f64
 * (keep_vjp = 1) call with the same (B,T,n), pair_batched, J12 and `lengths`: the packed ragged sweeps, one route at every
 * batch size.  J12 (T-1,n,n) or, pair_batched = 1, (B,T-1,n,n): pair t of sequence b reads the caller's block for
 * t <= L-2 and the zero block of the table in `workspace` behind it -- nothing stored at pairs t >= L-1 is read.
 * Cotangents of lognorm (B), E_node_diagxx / E_node_x (B,T,n or NULL), E_init (B, n n + n, or NULL), the per-step E_pair
 * (B,T-1,3,n,n or NULL; with the forward outputs E_pair and E_node_x) and samples (B,T,S,n or NULL, S <= 16, with eps and
 * samples).  g_E_pair is read under the forward pass's block masks: blocks 0 and 1 of pair t for t <= L-2, block 2 of pair
 * t-1 for t <= L-1.  Per sequence b: g_node_J[b,:L] and g_node_h[b,:L] are those of the sequence cut at L (pair parameters
 * [:L-1], node potentials [:L], the init potential whole); g_node_*[b,L:] are exactly 0; g_E_node_*[b,L:], g_samples[b,L:],
 * eps[b,L:], samples[b,L:], g_E_pair[b,L-1:] and J12 at t >= L-1 are never used (they may be NaN); no result of sequence b
 * depends on another sequence's length; a length outside 1..T is clamped for addressing.  g_node_logZ[b,t] = g_lognorm[b]
 * for t < L, else 0 (host side).  Returns 0, or before any HIP call: -1 B, -2 T, -3 n outside 1..SVAE_LDS_MAX_N,
 * -32 pair_batched outside {0, 1}, -31 lengths NULL, -4 S outside 1..16 with g_samples, -5 J12 NULL with T > 1,
 * -6 g_lognorm, -8 g_E_pair without E_pair / E_node_x, -10 g_samples without eps / samples, -12 / -13 outputs,
 * -24 options, -14 workspace NULL or shorter than svae_lds_ragged_perstep_workspace_bytes, -16 vjp_workspace shorter than
 * svae_lds_vjp_workspace_bytes; B = 0 returns 0 after the checks up to options. */
int svae_lds_ragged_perstep_vjp_f64(int B, int T, int n, int S, int pair_batched, unsigned options,
                                    const double* J12, const double* g_lognorm,
                                    const double* g_E_node_diagxx, const double* g_E_node_x,
                                    const double* g_E_init, const double* g_E_pair,
                                    const double* g_samples, const double* eps, const double* samples,
                                    const double* E_pair, const double* E_node_x,
                                    const int32_t* lengths, double* g_node_J, double* g_node_h,
                                    const void* workspace, size_t ws_bytes,
                                    void* vjp_workspace, size_t vjp_ws_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* SVAE_HIP_H */
