/*
 * glx.h — C ABI of libglx.so, the MI355X-native group-lasso first-order solver.
 *
 * Problem:  min_x  1/2 ||A x - b||_F^2 + mu * sum_i ||x_i||_2,   A: m x n, b: m x l, x: n x l
 * (row-major, contiguous; group i = row i of x, contiguous along l).
 *
 * This ABI replaces the bodies of the reference's solver functions, which all share the
 * signature  gl_<method>(x0, A, b, mu_0, opts) -> (x, iters, out):
 *   GLX_PROXGD  <- code/gl_ProxGD_primal.py:9-146   (proximal gradient + Armijo line search)
 *   GLX_FPROXGD <- code/gl_FProxGD_primal.py:9-161  (FISTA + backtracking)
 *   GLX_SGD     <- code/gl_SGD_primal.py:9-109      (subgradient)
 *   GLX_GD      <- code/gl_GD_primal.py:9-112       (gradient on the smoothed problem)
 *   GLX_FGD     <- code/gl_FGD_primal.py:9-163      (Nesterov on the smoothed problem)
 * and the dense products inside them (A @ x at gl_ProxGD_primal.py:25,61,129 and
 * A.T @ r at :129), which NumPy sends to host BLAS. A sixth solver has entries of its own
 * (glx_admm_*, below; it is not a glx_method and takes no session):
 *   dual ADMM   <- code/gl_ADMM_dual.py:10-103      (gl_Admm_dual; the Cholesky solves replaced by
 *                  one product with the explicit inverse K = (I + rho A A^T)^-1, caller-computed)
 *   primal ADMM <- code/gl_ADMM_primal.py:10-117    (gl_Admm_primal; glx_admm_primal_*, likewise with
 *                  an explicit inverse of rho I + A^T A, directly or through the Woodbury identity)
 *   dual ALM    <- code/gl_ALM_dual.py:10-158       (gl_Alm_dual; glx_alm_*, with the explicit inverses
 *                  K and Qn = rho (I + rho A^T A)^-1; the 500-step inner loop runs on the device)
 *
 * Conventions
 *   - Every pointer named "device" is HBM memory on the current HIP device; the library never
 *     allocates it: callers (the Python layer, through PyTorch) own A, b, x and the workspace.
 *   - `stream` is a hipStream_t passed as void* (NULL = the null stream). All calls are
 *     stream-ordered; glx_session_run() additionally synchronises the stream to read the
 *     scalars its control flow needs (line-search tests, the stop rule).
 *   - Return value: 0 on success, a GLX_E* code otherwise; glx_last_error() describes the
 *     failure (thread-local). No C++ exception crosses the ABI.
 *   - dtype is the compute type: GLX_F64 (double) or GLX_F32 (float). Scalars cross the ABI as
 *     double and are rounded to dtype where the reference's NumPy would (NEP 50 weak scalars).
 */
#ifndef GLX_H_
#define GLX_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define GLX_ABI_VERSION 2

enum glx_dtype { GLX_F32 = 0, GLX_F64 = 1 };
enum glx_method { GLX_PROXGD = 0, GLX_FPROXGD = 1, GLX_SGD = 2, GLX_GD = 3, GLX_FGD = 4 };
/* step_type option (gl_ProxGD_primal.py:78-101) */
enum glx_step { GLX_STEP_LINE_SEARCH = 0, GLX_STEP_FIXED = 1, GLX_STEP_DIMINISHING = 2,
                GLX_STEP_DIMINISHING2 = 3 };
enum glx_status { GLX_OK = 0, GLX_E_INVALID = 1, GLX_E_HIP = 2, GLX_E_RCCL = 3,
                  GLX_E_WORKSPACE = 4, GLX_E_STATE = 5 };

/* Solver options; field names and defaults follow the reference's default_opts dicts
 * (gl_ProxGD_primal.py:10-19 etc.). glx_default_opts() fills the per-method defaults. */
typedef struct glx_opts {
  int32_t maxit;                  /* iterations per continuation phase                   */
  double  thres;                  /* hard threshold / prox denominator switch (1e-3)      */
  int32_t step_type;              /* enum glx_step                                        */
  double  alpha0;                 /* initial / fixed step                                 */
  double  ftol;                   /* stop rule relative tolerance                         */
  int32_t stable_len_threshold;   /* stop after this many consecutive stable iterations   */
  double  ls_coeff;               /* line_search_attenuation_coeffi                       */
  int32_t ls_maxit;               /* maxit_line_search_iter                               */
  double  delta;                  /* smoothing parameter (GD / FGD)                       */
  int32_t continuous_subgradient; /* SGD/GD: alpha0 = 1/lambda_max(A^T A) (caller-computed:
                                     pass alpha0 accordingly; kept for ABI completeness)   */
  /* ---- build-only keys (the reference has no equivalent) ---- */
  int32_t exact_objective;        /* ProxGD: 1 = evaluate the next objective at the accepted
                                     x = prox(x - t*grad) itself (a third right-hand side in
                                     the same pass over A: A@[z | p_thr | p]), bit-faithful to
                                     the reference's evaluation order; 0 = reuse the accepted
                                     line-search residual A@z, z = x - t*G_t (ulp-level
                                     difference, SURVEY.md §8a reuse table)                   */
  int32_t profile;                /* k > 0: time every k-th A@x / A^T r launch (HIP events) */
  int64_t max_total_iters;        /* stop after this many iterations in total (0 = off)     */
  int32_t ax_variant;             /* A@x kernel variant for A/B tests (0 = auto)            */
  int32_t split_cand;             /* fp64 ProxGD / FProxGD split-candidate trial (A p = A p_thr
                                     + A e, A e gathered from a transposed copy of A): 0 = auto
                                     (on when this rank's A is >= 768 MiB; GLX_SPLIT_CAND env
                                     overrides), 1 = on at any size, 2 = off. On adds an m x n
                                     copy of A to the workspace (glx_workspace_bytes counts it) */
  int32_t dc_window;              /* device-controlled line search (ProxGD / FProxGD): 0 = auto
                                     (GLX_DC_BATCH env, else the measured default: 8 for
                                     FProxGD with a communicator, off otherwise), -1 = off,
                                     k in 1..32 = up to k iterations queued ahead of the host   */
  int32_t shard_rows;             /* ProxGD with a communicator of G > 1 ranks: 0 = auto (on),
                                     1 = on, 2 = off. On: the row-sharded schedule — the gradient
                                     is reduce-scattered, the prox / trial runs on this rank's
                                     n / G rows and the new iterate's rows are all-gathered
                                     (needs n % G == 0); off: the gradient is all-reduced and
                                     every rank runs the row-wise step on all n rows            */
  int32_t shard_model;            /* BENCHMARK ONLY (bench.py --shard-model): G > 1 with a world-1
                                     communicator runs the per-rank timing model of G ranks of the
                                     row-sharded ProxGD schedule (the trial on n / G rows, every
                                     line-search test accepted). Its iterates are NOT a solve:
                                     glx_solve refuses it and glx_session_describe says
                                     "(timing model)". 0 = off                                  */
  int32_t reserved[3];
} glx_opts;

/* One problem instance. For multi-GPU runs A and b are this rank's row shard
 * (m = local rows) and `comm` is a communicator from glx_comm_create(); x, mu and the
 * options are replicated on every rank. */
typedef struct glx_problem {
  int32_t dtype;        /* enum glx_dtype                                    */
  int32_t method;       /* enum glx_method                                   */
  int64_t m, n, l;      /* local rows of A, columns of A (= groups), columns of b/x */
  const void* A;        /* device, m x n row-major                          */
  const void* b;        /* device, m x l                                    */
  void* x;              /* device, n x l: x0 on entry, the iterate on return */
  double mu0;           /* mu_0                                             */
  void* comm;           /* glx_comm* or NULL                                */
} glx_problem;

typedef struct glx_result {
  int64_t iters;        /* k: total iterations (the reference's second return value) */
  double fval;          /* objective of the returned x (out["fval"])                 */
  double tt;            /* seconds spent in the iteration loop, stream-synchronised   */
  double* f_hist;       /* host, capacity f_cap: objective per iteration (out["f_hist"]) */
  double* f_hist_best;  /* host, capacity f_cap (out["f_hist_best"])                 */
  int64_t f_cap;
  int64_t n_fhist;      /* entries written                                           */
  int64_t ax_calls;     /* passes of A@x issued (executed-work accounting)            */
  int64_t atr_calls;    /* passes of A^T r issued                                     */
  int64_t syncs;        /* host readbacks the device queue drains behind (the host decides
                           before queuing more work; a device-controlled batch counts one) */
  int64_t ax_sources;   /* right-hand sides batched into those A@x passes (>= ax_calls) */
  double stats[8];      /* diagnostics: [0] threshold-changed entries and [1] rows summed over
                           accepted ProxGD steps, [2] accepted steps; split-candidate
                           FProxGD: [3] gathered batches, [4] dense batches, [5] nnz(e_c)
                           summed over the gathered ones, [6] A thr(x_k) restores;
                           [7] iterations whose line-search decision ran on the device  */
  int64_t record_waits; /* device-controlled batches: decision records the host read while
                           later iterations stayed queued on the device                   */
} glx_result;

typedef struct glx_session glx_session;
typedef struct glx_comm glx_comm;

int         glx_abi_version(void);
const char* glx_last_error(void);
int         glx_default_opts(int method, glx_opts* out);

/* Workspace (device bytes) a session needs for this problem and these options (includes the
 * transposed copy of A of the split-candidate trial, opts.split_cand, and the gradient-set ring
 * of device control with a communicator, opts.dc_window). Environment overrides (GLX_*) are read
 * here and at create: keep them unchanged in between. The session's whole mode is resolved here
 * as it is at create, so an option the mode refuses (opts.shard_rows = 1 with n % ranks != 0)
 * is refused here with the code and message glx_session_create gives. */
int glx_workspace_bytes(const glx_problem* prob, const glx_opts* opts, size_t* bytes);

/* Session API: the reference loop split so that a caller can time exactly K iterations.
 * create  — validates shapes, carves the workspace, copies nothing (x is used in place).
 * run     — runs up to max_steps further iterations (<=0: to completion); *done = steps run.
 *           *finished = 1 once all continuation phases are over.
 * finish  — evaluates fval of the current x and copies the histories into res.
 * destroy — frees host-side state (pinned buffers, events). */
int  glx_session_create(glx_session** out, const glx_problem* prob, const glx_opts* opts,
                        void* workspace, size_t workspace_bytes, void* stream);
int  glx_session_run(glx_session* s, int64_t max_steps, int64_t* done, int32_t* finished);
int  glx_session_finish(glx_session* s, glx_result* res);
/* launches timed and their total device time (ms) for A@x (kind 0: the dense pass) / A^T r
 * (kind 1) / the split-candidate A e gather (kind 2), sampled every opts.profile-th launch of that
 * kind; resets the accumulators. */
int  glx_session_kernel_time(glx_session* s, int kind, int64_t* launches, double* total_ms);
/* executed-work counters since create: out = {A@x passes, right-hand sides in them, A^T r
 * passes, host readbacks (glx_result.syncs)} (cumulative; the caller differences them around a
 * timed region). */
int  glx_session_counters(glx_session* s, int64_t out[4]);
/* Split-candidate trials since create by the form their A e took: out = {the gather from the
 * transposed copy of A (a launch of its own), the fused form inside the dense pass}. Both count
 * in a hybrid run (GLX_AE_HYB_ROWS); a session without the split-candidate trial reports 0, 0. */
int  glx_session_ae_forms(glx_session* s, int64_t out[2]);
/* Progress record, safe to call from ANOTHER thread while glx_session_run() is in progress (a
 * watchdog's diagnostic, round 6): out = {iterations recorded so far (k), continuation phase
 * (0..2), what the host is waiting on (0 nothing, 1 a scalar packet, 2 a device decision record),
 * collectives issued on the session's communicator (0 without one)}. */
int  glx_session_progress(glx_session* s, int64_t out[4]);
/* After glx_session_finish: what the reference's 'opt' logger prints, so a host can replay it
 * without touching the hot loop (gl_ProxGD_primal.py:54 `new mu=` per phase, :134-136 the line
 * every 100 iterations; same in gl_FProxGD_primal.py:56,149-151 and gl_SGD_primal.py:49,98-99).
 * sparsity_after[i] = sparsity of the iterate after iteration i+1's update (NaN where not
 * recorded: SGD/GD record it at every 100th iteration only); *n = entries written (with
 * sparsity_after == NULL: entries available). phase_info[p] = k at the start of phase p (-1 if
 * never entered), phase_info[3 + p] = 1 if the stop rule ended phase p (that iteration logs
 * nothing, :118-125). */
int  glx_session_trace(glx_session* s, double* sparsity_after, int64_t cap, int64_t* n,
                       int64_t phase_info[6]);
/* One-line description of the kernels this session launches (the planner's tiles and splits
 * after the session's own choices: the fused trial, the split-candidate form, the device-control
 * window), NUL-terminated, truncated to cap. */
int  glx_session_describe(glx_session* s, char* out, size_t cap);
/* The same string without a session, a device or a workspace: what a session created from this
 * problem, these options and the current environment would describe (the mode is resolved on the
 * host; A, b and x are validated as by glx_workspace_bytes and never read). */
int  glx_mode_describe(const glx_problem* prob, const glx_opts* opts, char* out, size_t cap);
/* The split-candidate trials' sparsity, one value per trial batch so far (diagnostic): ProxGD the
 * rows of e = p - p_thr (accepted trials), FProxGD nnz(e_c) of a gathered batch (flagged rows in
 * the row form) or -1 for a dense batch. *n = the count; up to cap values copied to out. */
int  glx_session_split_trace(glx_session* s, double* out, int64_t cap, int64_t* n);
void glx_session_destroy(glx_session* s);

/* One-shot solve: create + run to completion + finish + destroy. */
int glx_solve(const glx_problem* prob, const glx_opts* opts, void* workspace,
              size_t workspace_bytes, glx_result* res, void* stream);

/* ---- single kernels (test / composition surface) ---- */
/* R = A X - B (m x l); *half_sumsq_dev = 1/2 ||R||^2 (device double). */
int glx_residual(int dtype, int64_t m, int64_t n, int64_t l, const void* A, const void* X,
                 const void* B, void* R, void* half_sumsq_dev, void* workspace,
                 size_t workspace_bytes, int variant, void* stream);
/* Batched right-hand sides in one pass over A: R[i] = A X[i] - B for i < nsrc (nsrc <= 3);
 * sumsq_dev[i] = ||R[i]||^2 (device doubles, 4 slots). */
int glx_residual_batch(int dtype, int64_t m, int64_t n, int64_t l, const void* A, int nsrc,
                       const void* const* X, const void* B, void* const* R, void* sumsq_dev,
                       void* workspace, size_t workspace_bytes, int variant, void* stream);
/* G = A^T R (n x l). */
int glx_gradient(int dtype, int64_t m, int64_t n, int64_t l, const void* A, const void* R,
                 void* G, void* workspace, size_t workspace_bytes, void* stream);
/* X_out = prox_{t*mu*||.||_{1,2}}(W) with the reference's (||w_i|| < thres) + ||w_i||
 * denominator (gl_ProxGD_primal.py:65-71); sums_dev[0] = sum_i ||X_out_i||,
 * sums_dev[1] = max |X_out| (device doubles). */
int glx_prox(int dtype, int64_t n, int64_t l, const void* W, double t, double mu, double thres,
             void* X_out, void* sums_dev, void* workspace, size_t workspace_bytes, void* stream);
/* R = A X - B (m x l) and G = A^T R (n x l) (reference gl_ProxGD_primal.py:129
 * `A.T @ (A @ x - b)`). one_pass = 0: A @ X, then A^T R (two passes over A, the faster path on
 * MI355X); one_pass = 1: the fused residual-gradient kernel reads A from HBM once
 *  where the shape and device allow it (fp64, l = 32, n = 512 P with P a power
 * of two in 2..128, m a multiple of 16 * 256 / P, >= 256 CUs), else two passes. The one-pass
 * kernel is a cooperative launch (its workgroups wait for each other); if the runtime refuses it,
 * or a hand-off wait inside it times out (error flag read back: the one-pass call is synchronous),
 * R and G are recomputed with two passes. *one_pass_ran (may be NULL) = 1 when the returned R
 * and G come from the fused kernel. */
int glx_residual_gradient(int dtype, int64_t m, int64_t n, int64_t l, const void* A, const void* X,
                          const void* B, void* R, void* G, void* workspace, size_t workspace_bytes,
                          int one_pass, int* one_pass_ran, void* stream);
/* The line-search trial's batch and the next gradient (round 4, SURVEY §8f row 1 at l = 16):
 * R0 = A X0 - B, R1 = A X1 - B (the reference's A @ z and A @ p_thr, gl_ProxGD_primal.py:89-92,
 * :112) and G = A^T R1 (:129 at the candidate). one_pass = 1: one read of A by the role-split
 * kernel (kernels_rg2.hip) where the shape allows it (fp64, l = 16, n = 256 P with P a power of
 * two in 2..128, m a multiple of 64 * 256 / P, >= 256 CUs; slower than two passes on MI355X,
 * DESIGN.md (f), so the solver does not use it); a timed-out hand-off wait inside it
 * (error flag read back: the one-pass call is synchronous) or another shape runs A @ [X0 | X1],
 * then A^T R1. *one_pass_ran (may be NULL) = 1 when the outputs come from the one-pass kernel. */
int glx_residual_gradient2(int dtype, int64_t m, int64_t n, int64_t l, const void* A, const void* X0,
                           const void* X1, const void* B, void* R0, void* R1, void* G,
                           void* workspace, size_t workspace_bytes, int one_pass,
                           int* one_pass_ran, void* stream);
/* The thresholded part of the split-candidate line-search trial (round 5, SURVEY §8a row a9:
 * A e with e = p - p_thr nonzero only in the rows the hard threshold touched,
 * gl_ProxGD_primal.py:91,112,127; FProxGD's A e_c, gl_FProxGD_primal.py:92-97,136):
 *   Y (m x l) = sum over the rows k with row_masks[k] != 0 of At[k,:]^T E[k,:],  At = A^T (n x m).
 * row_masks[k] (device uint32, n + 3 readable) = the column mask of row k of E (bit c = E[k][c] != 0,
 * as the trial kernels write it). form 0: the MFMA row form (k_at_rows; FProxGD's default in the
 * solver, m % 64 == 0); form 1: the VALU column-list gather of rounds 2-4; form 2: the bitmap gather
 * (ProxGD's default in the solver since round 5, bit-identical to form 1). Forms 1, 2 need the exact
 * column masks. NOTE: these form codes are this entry point's own; they are NOT the codes of the
 * GLX_GATHER environment variable (bm / rows / lists). */
int glx_flagged_rows_product(int dtype, int64_t m, int64_t n, int64_t l, const void* At,
                             const void* E, const uint32_t* row_masks, void* Y, int form,
                             void* workspace, size_t workspace_bytes, void* stream);
/* The split-candidate trial's dense pass with A e fused in, one launch (launch_ax_egat; fp64):
 *   P  (S x m x l) = the K-split slabs of A p,
 *   Pe (S x m x l) = the K-split slabs of A e, e[k][c] = p[k][c] where zf's column bitmaps flag
 *                    (k, c) and 0 elsewhere (zf: the layout documented below, as a trial wrote it).
 * Runs only where the shape's one-source plan under GLX_AX_VARIANT / GLX_AX_S is the LDS-DMA tile
 * 92278 (l in {16, 32}, n % 32 == 0, n < 65536), else GLX_E_INVALID. *S = the K splits, *rotated =
 * 1 when row block bx walks its split's chunks from chunk bx * nch / gx (GLX_AX_ROT). With P and
 * Pe both NULL nothing is launched and only *S and *rotated are set (no device needed). Every
 * accumulator of Pe receives its entries in this order: the block's (rotated) walk over the
 * split's 32-column chunks, ascending k inside a chunk, one rounded multiply and one rounded add
 * per entry. */
int glx_fused_ae_pass(int64_t m, int64_t n, int64_t l, const void* A, const void* p,
                      const uint32_t* zf, void* P, void* Pe, int* S, int* rotated, void* stream);
/* The same dense pass alone with a given Infinity-Cache keep size (test surface): the arguments of
 * glx_fused_ae_pass plus keep_mib >= 0, the plan's ax_keep_mib (the solver's GLX_AX_KEEP_MIB; 0 = every
 * chunk of A non-temporal, as glx_fused_ae_pass plans). About keep_mib MiB of A over the grid, the
 * last chunks of every block's walk, load with the default policy; the results do not depend on it.
 * zf and Pe may both be NULL: the plain launch of the same tile (A p only). With P NULL nothing is
 * launched and only *S and *rotated are set. */
int glx_dense_pass_keep(int64_t m, int64_t n, int64_t l, const void* A, const void* p,
                        const uint32_t* zf, void* P, void* Pe, int keep_mib, int* S, int* rotated,
                        void* stream);
/* ---- the line-search trial, one kernel at a time (test surface) ----
 * The other half of an iteration: prox, hard threshold, the Armijo / backtracking sums, and in
 * the split-candidate form the masks of e and the column bitmaps the A e gather walks. Both
 * entries wrap the launchers a session uses and add no arithmetic of their own. Outputs are
 * caller-owned device buffers of n x l values of dtype; sums_dev is 6 device doubles.
 *
 * zf (may be NULL) is a caller-owned, caller-zeroed device buffer of the bytes
 * glx_trial_mask_bytes(n) gives, read as uint32 words. Layout, with npad = n rounded up to a
 * multiple of 64:
 *   words [0, npad):  the row masks, zf[k] bit c = e[k][c] != 0 (rows >= n stay as passed in);
 *   behind them, as uint16 words, the column bitmaps: word g of column c, at index
 *   c * (npad / 16) + g, holds rows 16 g .. 16 g + 15 (bit j = row 16 g + j has bit c), for
 *   c < l and the npad / 16 row groups.
 * An entry does not clear zf: a trial rewrites the words of the row groups it visits (the 16-row
 * groups below n rounded up to 16, or whole 64 / 32-row panels in the fused forms) and leaves
 * the others as they are, as in a session, which clears the buffer once at creation. zf needs
 * l in {16, 32} and n < 65536.
 *
 * The workspace of the two entries is glx_trial_workspace_bytes (glx_kernel_workspace_bytes plus
 * the per-panel counters a fused A^T R with K splits counts on); forms 0 and 2 take m = 1. */
int glx_trial_mask_bytes(int64_t n, size_t* bytes);
int glx_trial_workspace_bytes(int dtype, int64_t m, int64_t n, int64_t l, size_t* bytes);
/* ProxGD's trial (gl_ProxGD_primal.py:65-74, 89-92): p = prox_{t mu}(x - t G), G_t = (x - p) / t,
 * z = x - t G_t, pthr = p with |p| < thres zeroed; sums_dev = [sum G * G_t, sum G_t^2,
 * sum_i ||p_i||, max |p| (NaN-propagating), #{entries the threshold changed}, #{rows it changed}].
 *   form 0: the row kernel (k_prox_pgd) on the given G; A, R and m are unused.
 *   form 1: the trial in the epilogue of G = A^T R (k_atr_prox): G is written. The tile and K
 *           splits are the planner's for this shape under GLX_ATR_VARIANT / GLX_ATR_S /
 *           GLX_ATR_FUSE_SPLIT; GLX_E_INVALID where that plan does not take a fused trial.
 *   form 2: the replicated half of the row-sharded schedule (k_trial_split): p is an INPUT and
 *           x the thresholded iterate; writes pthr, z (may be NULL) and zf; no sums.
 * emode != 0 (needs zf): z receives e = p - pthr instead, zf the masks and bitmaps of e. In
 * forms 0 and 1 zf must be NULL when emode == 0; form 2 writes zf, when given, for either. */
int glx_trial_proxgd(int dtype, int64_t m, int64_t n, int64_t l, const void* A, const void* R,
                     void* G, const void* x, double t, double mu, double thres, int form, int emode,
                     void* p, void* pthr, void* z, void* sums_dev, uint32_t* zf, void* workspace,
                     size_t workspace_bytes, void* stream);
/* A residual finalize and the fused A^T R + ProxGD trial behind it (fp64; n % 64 == 0, m % 4 == 0,
 * l in {16, 32}; the four-wave 64-column panel without K splits whatever the shape's plan):
 *   the finalize: R0 = sum of source 0's slabs - B, R1 = the same of source 1 (chain 0: S slabs a
 *     source, source 1 behind source 0), or the chained forms of the split-candidate trial (S0
 *     slabs of A e, then S slabs: chain 1 R1 = slabs - B, R0 = R1 + A e; chain 2 R0 = slabs - B,
 *     R1 = R0 - A e; R0 may be NULL with a chain); fin_parts receives its four sums per
 *     256-thread block (sum R0^2, sum R1^2, 0, count(|cx| > 1e-6 max) with cx of n * l values or
 *     NULL; the max is *cmax or, cmax_parts != NULL, the max of column 3 of cmax_np partials of 6
 *     values), *fin_blocks their number (at most 1024);
 *   the trial: glx_trial_proxgd's form 1 with R = R1 (emode with zf).
 * head = 0: k_finalize_residual, then k_atr_prox. head = 1: one launch, the finalize at the head of
 * k_atr_prox; every bit equals head = 0. GLX_E_INVALID where the device cannot hold the launch's
 * n / 64 workgroups at once, GLX_E_HIP if the head's barrier times out. head_ws: 8192 bytes of
 * device memory (cleared here). workspace: glx_trial_workspace_bytes. Returns after the launch has
 * finished (it reads the barrier's abort word back). */
int glx_fin_atr_prox(int64_t m, int64_t n, int64_t l, const void* A, const void* P, int S, int S0,
                     int chain, const void* B, void* R0, void* R1, const void* cx, const double* cmax,
                     const double* cmax_parts, int cmax_np, double* fin_parts, int* fin_blocks,
                     void* G, const void* x, double t, double mu, double thres, int emode, void* p,
                     void* pthr, void* z, void* sums_dev, uint32_t* zf, int head, void* head_ws,
                     void* workspace, size_t workspace_bytes, void* stream);
/* The finalize head's co-residency guard: 1 where n / 64 + 1 workgroups fit cus * per_cu. */
int glx_fin_head_fits(int64_t n, int cus, int per_cu);
/* "fin=head" where this session runs the speculative trial's residual finalize at the head of
 * k_atr_prox (single GPU, host control, deferred reductions, the f64 four-wave panel, and a device
 * that holds all its workgroups at once) and GLX_FIN_HEAD=1 asks for it, else "fin=kernel". */
int glx_session_fin_form(glx_session* s, char* out, size_t cap);
/* FProxGD's / FGD's trial with the next combine (gl_FProxGD_primal.py:92-102, 136-145):
 * xc = prox_{t mu}(y - t G) (prox = 1) or y - t G (prox = 0, FGD),
 * vnext = thr(xk) + (xc - thr(xk)) / theta, ynext = (1 - theta_next) thr(xc) + theta_next vnext.
 * sums_dev: prox = 1: [sum G * (xc - y), sum (xc - y)^2, sum_i ||xc_i||, max |xc|];
 *           prox = 0: [.., .., sum_i (sqrt(||xc_i||^2 + delta^2) - delta), sum_i ||xc_i||, max |xc|].
 *   form 0: the row kernel (k_fista_trial). ec and zf (both or neither, prox = 1 only):
 *           ec = xc - thr(xc) and zf its masks and bitmaps.
 *   form 1: the trial in the epilogue of G = A^T R (k_atr_fista), prox = 1 only; plan as above.
 *   form 2: the replicated half (k_fista_split): xc is an INPUT; writes vnext and ynext. */
int glx_trial_fista(int dtype, int64_t m, int64_t n, int64_t l, const void* A, const void* R,
                    void* G, const void* y, const void* xk, double t, double mu, double thres,
                    double theta, double theta_next, double delta, int form, int prox, void* xc,
                    void* vnext, void* ynext, void* ec, void* sums_dev, uint32_t* zf,
                    void* workspace, size_t workspace_bytes, void* stream);
/* ---- the descent-method kernels, one launch at a time (test surface) ----
 * What SGD, GD and FGD run between the dense products, and the one-pass kernel of an l = 1
 * descent iteration. Each entry wraps the launcher a session uses and adds no arithmetic of its
 * own; buffers are caller-owned device memory of dtype, sums are device doubles. The workspace of
 * the entries that take one is glx_descent_workspace_bytes: glx_kernel_workspace_bytes plus, where
 * the one-pass kernel applies to (m, n, l), its per-workgroup gradient slabs. The row entries
 * take any m there (1 will do). */
int glx_descent_workspace_bytes(int dtype, int64_t m, int64_t n, int64_t l, size_t* bytes);
/* The SGD (mode 0, gl_SGD_primal.py:56-61, 93-96) / GD (mode 1, gl_GD_primal.py:59-63, 95-98)
 * step from the thresholded iterate xt (in / out) and the gradient g = the sum, in slab order, of
 * S >= 1 slabs of n * l values:
 *   d = (||xt_i|| < thres) + ||xt_i||  (mode 0)  or  sqrt(||xt_i||^2 + delta^2)  (mode 1),
 *   x = xt - alpha (g + mu xt / d)  (out),  xt = x with |x| < thres zeroed,
 *   sum_dev[0] = sum_i ||x_i||. x and xt must not alias. */
int glx_descent_step(int dtype, int64_t n, int64_t l, int mode, const void* g, int S, double alpha,
                     double mu, double thres, double delta, void* x, void* xt, void* sum_dev,
                     void* workspace, size_t workspace_bytes, void* stream);
/* FGD's smoothed gradient (gl_FGD_primal.py:64-72): g = sum of the S slabs of gp
 * + mu y / sqrt(||y_i||^2 + delta^2); sum_dev[0] = sum_i (sqrt(||y_i||^2 + delta^2) - delta). */
int glx_fgd_gradient(int dtype, int64_t n, int64_t l, const void* y, const void* gp, int S, double mu,
                     double delta, void* g, void* sum_dev, void* workspace, size_t workspace_bytes,
                     void* stream);
/* stats_dev = [sum_i ||x_i||, max |x| (NaN-propagating), #{|x| > 1e-6 max |x|}]: the row-norm
 * kernel, then the count reading the maximum the first just wrote, on the same partials and
 * ticket (sparsity_func of the SGD / GD log line). */
int glx_row_stats(int dtype, int64_t n, int64_t l, const void* x, void* stats_dev, void* workspace,
                  size_t workspace_bytes, void* stream);
/* xo = x with |x| < thres zeroed (count values; xo may equal x). *flag_dev = epoch when a nonzero
 * value was zeroed, else left as it is. */
int glx_threshold(int dtype, int64_t count, const void* x, void* xo, double thres, int* flag_dev,
                  int epoch, void* stream);
/* FISTA / FGD's threshold and combine (gl_FGD_primal.py:139-142): xk[|xk| < thres] = 0 in place,
 * y = a xk + b vk. */
int glx_thr_combine(int dtype, int64_t count, void* xk, const void* vk, void* y, double thres, double a,
                    double b, void* stream);
/* One pass over A (m x n) of an l = 1 descent iteration, then the column sum of its slabs:
 * G = A^T (A xt - b), sums_dev = [sum (A x - b)^2, sum (A xt - b)^2], and, when fh_dev is given
 * (it needs rn_dev), fh_dev[0] = 0.5 sums_dev[0] + fh_mu * rn_dev[0]. nt: 0 / 1 = A read with the
 * default / the non-temporal policy, -1 = as a session decides. *blocks (may be NULL) receives
 * the workgroup count. GLX_E_INVALID, with nothing written, where the kernel does not apply:
 * n no multiple of 16 / sizeof(dtype), or more than 8 vectors of 16 bytes per thread
 * (n > 4096 * 16 / sizeof(dtype)). */
int glx_descent_pass(int dtype, int64_t m, int64_t n, const void* A, const void* x, const void* xt,
                     const void* b, void* G, void* sums_dev, void* fh_dev, double fh_mu,
                     const void* rn_dev, int nt, int* blocks, void* workspace, size_t workspace_bytes,
                     void* stream);
/* Workspace bytes for the single-kernel entry points above. */
int glx_kernel_workspace_bytes(int dtype, int64_t m, int64_t n, int64_t l, size_t* bytes);
/* One-line description of the kernels (tile, split) the planner picks for this shape, for
 * A @ X with 1, 2, 3 right-hand sides and for A^T R (NUL-terminated, truncated to cap). */
int glx_plan_describe(int dtype, int64_t m, int64_t n, int64_t l, char* out, size_t cap);

/* ---- the dual ADMM solver (additive entries; the ABI version stays 2) ----
 * GLX dual ADMM <- code/gl_ADMM_dual.py:10-103, gl_Admm_dual(x0, A, b, mu, opts). Of the
 * reference's three factorising solvers this was the first built (ADMM primal and ALM dual follow
 * below). The reference solves with the Cholesky factor of I + rho A A^T at every iteration
 * (:57, :63); here the caller computes the explicit inverse K = (I + rho A A^T)^-1 once per solve
 * (m x m, always in fp64, then cast to dtype; plumbing, like alpha0 = 1 / lambda_max above) and
 * hands it in as a device pointer, so z = K v is one more dense product. Per iteration: one pass
 * over K, two over A (A^T z, A @ [x+ | u+]), small kernels, and one readback of a small record
 * (the objective's sums and the l x l Gram matrices of r and s, whose largest eigenvalues give the
 * spectral norms of the stop rule, :85-93). l <= 32. Single GPU. */
typedef struct glx_admm_opts {
  int32_t maxit;            /* gl_ADMM_dual.py:12 (100)                                       */
  int32_t converge_len;     /* :16 (20): stop after this many consecutive small iterations    */
  double  thres;            /* :13 (1e-3): both spectral norms below it count as small        */
  double  tau;              /* :14 ((1 + sqrt 5) / 2)                                         */
  double  rho;              /* :15 (1e2); K must have been built with the same value          */
  int32_t fused;            /* the row step in the epilogue of A^T z: 0 auto, 1 on (where the
                               plan's A^T R tile is built fused for dtype), 2 off (row kernel) */
  int64_t max_total_iters;  /* stop after this many iterations (0 = off)                      */
  int32_t reserved[4];
} glx_admm_opts;
int glx_admm_default_opts(glx_admm_opts* out);
/* Device bytes glx_admm_dual_solve needs (opts may be NULL: the defaults). Also enough for
 * glx_admm_dual_step at the same (dtype, m, n, l). */
int glx_admm_workspace_bytes(int dtype, int64_t m, int64_t n, int64_t l, const glx_admm_opts* opts,
                             size_t* bytes);
/* The whole solve. prob->x holds x0 on entry and the iterate on return; prob->method is ignored;
 * prob->comm must be NULL (GLX_E_INVALID otherwise, as for l = 0 or l > 32, a NULL K and a
 * workspace smaller than glx_admm_workspace_bytes). Fills res->iters, fval, tt (the loop, stream-
 * synchronised; the caller adds its K setup), f_hist, f_hist_best, n_fhist, ax_calls (passes over
 * A by A @ [x | u]), ax_sources, atr_calls, syncs (one per iteration); stats[0] = passes over K,
 * stats[1] = 1 when the row step ran fused. */
int glx_admm_dual_solve(const glx_problem* prob, const void* K_device, const glx_admm_opts* opts,
                        void* workspace, size_t workspace_bytes, glx_result* res, void* stream);
/* After glx_admm_dual_solve, on the same thread: the sparsity of the iterate after each iteration
 * (sparsity_func, :22-23, for the replayed debug line :83); *n = entries written (with
 * sparsity_after == NULL: entries available). */
int glx_admm_trace(double* sparsity_after, int64_t cap, int64_t* n);
/* One line: the tiles of the three passes (K v; A @ [x | u] and A^T z) and whether the row step is
 * fused. Resolved on the host; needs no device. opts may be NULL. */
int glx_admm_describe(int dtype, int64_t m, int64_t n, int64_t l, const glx_admm_opts* opts, char* out,
                      size_t cap);
/* ---- the dual ADMM kernels, one launch at a time (test surface) ----
 * The row step (:64-67) through the launchers the driver uses: w = x / rho - g,
 * u_out = (mu w) / max(||w_i||, mu), r_out = u_out + g, x_out = x - (tau rho) r_out;
 * sums_dev = [sum_i ||x_out_i||, max |x_out| (NaN-propagating)] (device doubles).
 *   form 0: the row kernel on the given G; A and Z are unused. Where the plan of (m, n, l) takes
 *           a fused epilogue the rows run on that epilogue's panel layout (k_admm_dual_panel, what
 *           a solve with fused = 2 launches there) and every bit, the two sums included, equals
 *           form 1's; elsewhere (any l <= 32, any n; m = 1 will do) the generic row layout
 *           (k_admm_dual).
 *   form 1: the epilogue of G = A^T Z (k_atr_admm): G is written. GLX_E_INVALID where the plan of
 *           this shape takes no fused epilogue (glx_admm_describe).
 * Workspace: glx_admm_workspace_bytes(dtype, m, n, l). */
int glx_admm_dual_step(int dtype, int64_t m, int64_t n, int64_t l, const void* A, const void* Z, void* G,
                       const void* x, double rho, double tau, double mu, int form, void* u_out,
                       void* x_out, void* r_out, void* sums_dev, void* workspace,
                       size_t workspace_bytes, void* stream);
/* gram_dev (l x l device doubles, row-major) = R^T R for R of rows x l values of dtype (l <= 32),
 * accumulated in double over fixed row slabs in a fixed order (bit-reproducible).
 * Workspace: 8 * 256 * l * l bytes. */
int glx_gram(int dtype, int64_t rows, int64_t l, const void* R, void* gram_dev, void* workspace,
             size_t workspace_bytes, void* stream);
/* Host only: *out = the largest eigenvalue of the symmetric l x l matrix G (row-major, l <= 32) by
 * cyclic Jacobi sweeps; NaN where G holds one. */
int glx_sym_lambda_max(const double* G, int l, double* out);

/* ---- the primal ADMM solver (additive entries; the ABI version stays 2) ----
 * GLX primal ADMM <- code/gl_ADMM_primal.py:10-117, gl_Admm_primal(x0, A, b, mu, opts). The
 * reference solves with the Cholesky factor of rho I + A^T A (n x n) at every iteration (:62, :78);
 * here the caller builds an explicit inverse once per solve (always in fp64, then cast to dtype)
 * and hands it in, in one of two forms of y+ = (rho I + A^T A)^-1 w, w = A^T b - z + rho x:
 *   direct   (form 1): y+ = Kn w with Kn = (rho I + A^T A)^-1 (n x n): one pass over Kn and one
 *                      over A (A @ x+) per iteration;
 *   Woodbury (form 2): y+ = (w - A^T K (A w)) / rho with K = (rho I + A A^T)^-1 (m x m) and
 *                      A w = A A^T b - A z + rho A x from the batched pass A @ [x+ | z+]: one pass
 *                      over K and two over A per iteration, the dual solver's schedule.
 * form 0 (auto) resolves to Woodbury exactly when m^2 + m n < n^2 (the bytes an iteration streams:
 * 2 m n + m^2 against n^2 + m n). Then the row step (:47-51, :80-84): p = x - (eta rho)(x - y+ -
 * z / rho), x+ = p max(||p_i|| - eta mu, 0) / ((||p_i|| < thres) + ||p_i||), z+ = z - (tau rho)(x+
 * - y+), r = x+ - y+, s = y+ - y, and one readback of a small record per iteration, as in the dual
 * solver (both Gram matrices are of n x l iterates here). l <= 32. Single GPU.
 * dtype: GLX_F64 always; GLX_F32 only where m >= n and the resolved form is direct: rho I + A^T A
 * has condition number ||A||^2 / rho (1e5 .. 1e6 at the default rho) for m < n, and an fp32 inverse
 * and fp32 iterates then never meet the stop rule. Anything else is GLX_E_INVALID. */
typedef struct glx_admm_primal_opts {
  int32_t maxit;            /* gl_ADMM_primal.py:12 (100)                                     */
  int32_t converge_len;     /* :17 (10): stop after this many consecutive small iterations    */
  double  thres;            /* :13 (1e-3): the stop rule's bound and the prox denominator's   */
  double  tau;              /* :14 ((1 + sqrt 5) / 2)                                         */
  double  rho;              /* :15 (1e-2); the inverse must have been built with this value   */
  double  eta_0;            /* :16 (100)                                                      */
  int32_t step_type;        /* :19 GLX_STEP_FIXED (eta_0), _DIMINISHING (eta_0 / sqrt k),
                               _DIMINISHING2 (eta_0 / k)                                      */
  int32_t form;             /* 0 auto, 1 direct, 2 Woodbury                                   */
  int64_t max_total_iters;  /* stop after this many iterations (0 = off)                      */
  int32_t reserved[4];
} glx_admm_primal_opts;
int glx_admm_primal_default_opts(glx_admm_primal_opts* out);
/* Device bytes glx_admm_primal_solve needs (opts may be NULL: the defaults). */
int glx_admm_primal_workspace_bytes(int dtype, int64_t m, int64_t n, int64_t l,
                                    const glx_admm_primal_opts* opts, size_t* bytes);
/* One line: "form=direct" or "form=Woodbury", then the tiles of the passes. Resolved on the host;
 * needs no device. opts may be NULL. GLX_E_INVALID for what the solve would refuse (the fp32 rule
 * included). */
int glx_admm_primal_describe(int dtype, int64_t m, int64_t n, int64_t l,
                             const glx_admm_primal_opts* opts, char* out, size_t cap);
/* The whole solve. prob->x holds x0 on entry and the iterate on return (y and z start at x0 too,
 * :53-55); prob->method is ignored; prob->comm must be NULL. K_device: Kn (n x n) for the direct
 * form, K (m x m) for Woodbury; ATb_device = A^T b (n x l); AATb_device = A A^T b (m x l),
 * required by Woodbury and unused (may be NULL) by direct. GLX_E_INVALID for a communicator,
 * l > 32, rho <= 0, eta_0 <= 0, an unknown step_type or form, a NULL or not 16-byte aligned
 * pointer, the fp32 rule above, Woodbury without AATb and a workspace smaller than
 * glx_admm_primal_workspace_bytes. Fills res as glx_admm_dual_solve does: ax_calls = iters + 1
 * (the first pass gives the objective of x0, returned when maxit = 0), atr_calls = iters
 * (Woodbury) or 0 (direct), syncs = iters; stats[0] = passes over the inverse, stats[1] = the
 * resolved form (1 direct, 2 Woodbury). glx_admm_trace serves this solver too. */
int glx_admm_primal_solve(const glx_problem* prob, const void* K_device, const void* ATb_device,
                          const void* AATb_device, const glx_admm_primal_opts* opts, void* workspace,
                          size_t workspace_bytes, glx_result* res, void* stream);
/* ---- the primal ADMM row kernel in one launch (test surface) ----
 * prod = S >= 1 slabs of n * l values, summed in slab order: the product Kn w (form 1) or
 * g = A^T K (A w) (form 2, which also reads w). With y+ = prod (form 1) or (w - prod) / rho
 * (form 2), the step above with eta given: x_out, y_out, z_out, r_out, s_out and
 * w_out = (ATb - z_out) + rho x_out, the next iteration's w;
 * sums_dev = [sum_i ||x_out_i||, max |x_out| (NaN-propagating)] (device doubles). w may be NULL in
 * form 1. Any n, l <= 32, both dtypes. Workspace: glx_kernel_workspace_bytes(dtype, 1, n, l). */
int glx_admm_primal_step(int dtype, int64_t n, int64_t l, int form, int S, const void* prod,
                         const void* x, const void* y, const void* z, const void* w, const void* ATb,
                         double rho, double tau, double eta, double mu, double thres, void* x_out,
                         void* y_out, void* z_out, void* r_out, void* s_out, void* w_out,
                         void* sums_dev, void* workspace, size_t workspace_bytes, void* stream);

/* ---- the dual ALM solver (additive entries; the ABI version stays 2) ----
 * GLX dual ALM <- code/gl_ALM_dual.py:10-158, gl_Alm_dual(x0, A, b, mu, opts). At every outer
 * iteration the reference rebuilds T = (I + rho A A^T)^-1, F = rho T A, G = I - A^T F,
 * Q = F^T F + rho G^T G and J (:33-40) and runs 500 Nesterov steps on grad = Q u + J (:53-61). Two
 * identities remove that: G = (I + rho A^T A)^-1, so Q = rho G =: Qn depends on A and rho alone, and
 * J = rho H = rho (A^T K (A x - b) - x / rho). The caller builds K = (I + rho A A^T)^-1 (m x m) and
 * Qn (n x n, symmetric) once per solve, in fp64, and hands both in. Per outer iteration: two passes
 * over K (E = K (Ax - b); z = K v), two A^T passes (A^T E, A^T z), two passes over A (A u;
 * A @ [x+ | u]), inner_iters inner steps with one pass over Qn each, enqueued back to back with no
 * host synchronisation and no graph, and one readback of the small record of the ADMM solvers.
 * l <= 32. Single GPU. GLX_F64 only: I + rho A^T A has condition number about rho ||A||^2 (1e5 ..
 * 1e6 at the default rho for m < n) and the inner loop multiplies by its inverse 500 times per outer
 * iteration; GLX_F32 is GLX_E_INVALID in every entry below. */
typedef struct glx_alm_opts {
  int32_t maxit;            /* gl_ALM_dual.py:68 (100)                                         */
  int32_t converge_len;     /* :72 (20): stop after this many consecutive small iterations     */
  double  thres;            /* :69 (1e-3): both spectral norms below it count as small         */
  double  tau;              /* :70 ((1 + sqrt 5) / 2)                                          */
  double  rho;              /* :71 (1e2); K and Qn must have been built with the same value    */
  int32_t inner_iters;      /* :53 (500), the reference's hard-coded max_iteration; >= 1       */
  double  inner_step;       /* :57 (1e-2), the reference's hard-coded t. As in the reference,
                               nothing guards inner_step * rho > 1 (the step then exceeds
                               1 / ||Qn|| and the inner loop may diverge)                      */
  int32_t fused;            /* the inner step in the epilogue of Qn y: 0 auto (on where the plan
                               of (n, n, l) admits it), 1 on (likewise), 2 off                 */
  int64_t max_total_iters;  /* stop after this many outer iterations (0 = off)                 */
  int32_t reserved[4];
} glx_alm_opts;
int glx_alm_default_opts(glx_alm_opts* out);
/* Device bytes glx_alm_dual_solve needs (opts may be NULL: the defaults). */
int glx_alm_workspace_bytes(int dtype, int64_t m, int64_t n, int64_t l, const glx_alm_opts* opts,
                            size_t* bytes);
/* One line: the tiles of the passes over K, A and Qn and whether the inner step is fused ("inner
 * step=fused ..." or "inner step=row kernel ..."). Resolved on the host; needs no device. */
int glx_alm_describe(int dtype, int64_t m, int64_t n, int64_t l, const glx_alm_opts* opts, char* out,
                     size_t cap);
/* The whole solve. prob->x holds x0 on entry and the iterate on return; prob->method is ignored.
 * GLX_E_INVALID for a communicator, l = 0 or l > 32, GLX_F32, rho <= 0, inner_iters < 1, fused
 * outside 0..2, a NULL or not 16-byte aligned pointer and a workspace smaller than
 * glx_alm_workspace_bytes. Fills res as glx_admm_dual_solve does: ax_calls = 2 iters + 1,
 * atr_calls = 2 iters, syncs = iters; stats[0] = passes over K (2 iters), stats[1] = 1 when the
 * inner step ran fused, stats[2] = inner steps run (iters * inner_iters). maxit = 0 returns x0 and
 * its objective. glx_admm_trace serves this solver too. */
int glx_alm_dual_solve(const glx_problem* prob, const void* K_device, const void* Qn_device,
                       const glx_alm_opts* opts, void* workspace, size_t workspace_bytes, glx_result* res,
                       void* stream);
/* ---- the dual ALM inner loop, one launch or one loop at a time (test surface) ----
 * Workspace of the two entries below for (n, l). */
int glx_alm_inner_workspace_bytes(int dtype, int64_t n, int64_t l, size_t* bytes);
/* One inner step: with P = Qn y, w = y - t (P + J), u_out = (mu w) / max(||w_i||, mu),
 * v = u + (u_out - u) / gamma, y_out = (1 - gamma_next) u_out + gamma_next v.
 *   form 0: the row kernel on the given P = S >= 1 slabs of n * l values summed in slab order (Qn is
 *           unused): on the epilogue's panel layout where the plan of (n, n, l) fuses
 *           (k_alm_inner_panel: every bit equals form 1's), on the generic row layout elsewhere.
 *   form 1: the epilogue of P = Qn^T y (k_atr_alm; P and S are unused). GLX_E_INVALID where the plan
 *           takes no fused epilogue (glx_alm_describe).
 * gamma_next = 0: y_out is not written. u_out may be u; y_out must not be y. */
int glx_alm_inner_step(int dtype, int64_t n, int64_t l, const void* Qn, const void* P, int S, const void* y,
                       const void* u, const void* J, double gamma, double gamma_next, double t, double mu,
                       int form, void* u_out, void* y_out, void* workspace, size_t workspace_bytes,
                       void* stream);
/* The driver's inner loop from u = y = 0: `iters` steps with gamma = 2 / (i + 1), enqueued back to
 * back; u_out (n x l) receives u. fused as in glx_alm_opts. */
int glx_alm_inner_run(int dtype, int64_t n, int64_t l, const void* Qn, const void* J, int iters, double t,
                      double mu, int fused, void* u_out, void* workspace, size_t workspace_bytes,
                      void* stream);

/* ---- the glue kernels of the three splitting solvers, one launch each (test surface) ----
 * The elementwise and finalize kernels between the dense products of glx_admm_dual_solve,
 * glx_admm_primal_solve and glx_alm_dual_solve. "S slabs" are S arrays of the element count laid end
 * to end and summed in ascending slab order from slab 0. Scalars are rounded to the dtype first.
 * The reducing entries take a workspace of glx_kernel_workspace_bytes(dtype, 1, 1, 1) bytes, 256-byte
 * aligned (GLX_E_WORKSPACE otherwise); sums_dev receives device doubles.
 *
 * glx_admm_rhs: v_out = (Ax - rho Au) - b over ml elements (k_admm_v). Ax may be Au (the dual ALM
 * solver passes Ax twice with rho = 0). */
int glx_admm_rhs(int dtype, int64_t ml, const void* Ax, const void* Au, const void* b, double rho, void* v_out,
                 void* stream);
/* glx_admm_fin (k_admm_fin): P = 2 S slabs of ml values, the first source's S then the second's.
 * au = the second source's sum; s[i] = Au[i] - au (Au as it was on entry; s may be NULL: not
 * written), then Ax[i] = the first source's sum, Au[i] = au; sums_dev[0] = sum_i (Ax[i] - b[i])^2,
 * each square rounded to the dtype and accumulated in double. */
int glx_admm_fin(int dtype, int64_t ml, int S, const void* P, const void* b, void* Ax, void* Au, void* s,
                 void* sums_dev, void* workspace, size_t workspace_bytes, void* stream);
/* glx_admm_primal_rhs: w_out = (ATb - z) + rho x over nl elements (k_admm_primal_w). */
int glx_admm_primal_rhs(int dtype, int64_t nl, const void* ATb, const void* x, const void* z, double rho,
                        void* w_out, void* stream);
/* glx_admm_primal_fin (k_admm_primal_fin): Ax[i] = the sum of the first S slabs of P and
 * sums_dev[0] = sum_i (Ax[i] - b[i])^2 as above. With AATb given (the Woodbury form) P holds S more
 * slabs: Az[i] = their sum and v[i] = (AATb[i] - Az[i]) + rho Ax[i]. AATb == NULL: Az and v are not
 * written (and may be NULL) and P holds S slabs only. */
int glx_admm_primal_fin(int dtype, int64_t ml, int S, const void* P, const void* b, const void* AATb, double rho,
                        void* Ax, void* Az, void* v, void* sums_dev, void* workspace, size_t workspace_bytes,
                        void* stream);
/* glx_alm_j: J_out = rho (h - x / rho) with h the sum of S slabs of nl values (k_alm_j). GLX_F64 only
 * (GLX_E_INVALID for GLX_F32), rho > 0. */
int glx_alm_j(int dtype, int64_t nl, int S, const void* h, const void* x, double rho, void* J_out, void* stream);
/* glx_alm_x (k_alm_x): r_out = u + g with g the sum of S slabs of n * l values,
 * x_out = x - taurho r_out (x_out may be x), sums_dev = [sum_i ||x_out_i||, max |x_out|
 * (NaN-propagating)]. GLX_F64 only; GLX_E_INVALID for l > 32, before anything is written. */
int glx_alm_x(int dtype, int64_t n, int64_t l, int S, const void* x, const void* u, const void* g, double taurho,
              void* x_out, void* r_out, void* sums_dev, void* workspace, size_t workspace_bytes, void* stream);

/* ---- optimality certificate of any iterate (DESIGN.md "Certificate") ----
 * For P(x) = 1/2 ||A x - b||_F^2 + mu sum_i ||x_i||_2 (x_i the rows of the n x l iterate) and its
 * dual D(theta) = -1/2 ||theta||_F^2 - <theta, b> over ||(A^T theta)_i||_2 <= mu: with r = A x - b,
 * g = A^T r, gmax = max_i ||g_i||_2 and s = 1 where gmax <= mu, mu / gmax elsewhere, theta = s r is
 * dual feasible and gap = P(x) - D(s r) >= P(x) - min P >= 0. One pass over A and one over A^T,
 * one readback, one stream synchronise. Single GPU: there is no communicator argument.
 *   out = [||r||^2, <r, b>, sum_i ||x_i||, gmax, kkt_max, sum_i kkt_i^2, nonzero rows, fused was
 *          used], host doubles, with kkt_i = ||g_i + mu x_i / ||x_i|| || where x_i != 0 and
 *          max(||g_i|| - mu, 0) where x_i = 0. The caller composes, in double,
 *          primal = out[0] / 2 + mu out[2], dual = -s^2 out[0] / 2 - s out[1], gap = primal - dual.
 *          gmax and kkt_max are NaN where a row feeding them holds one (so is the row count).
 *   fused: 0 auto, 1 on (the row terms in the epilogue of A^T r where the ADMM solvers' plan of
 *          (dtype, m, n, l) is built fused), 2 off (a row kernel behind the plain product); the
 *          record and rownorm_out are bit-identical between 1 and 2.
 *   G_out (n x l of dtype) and rownorm_out (n doubles: ||g_i||_2) are device pointers, or NULL.
 * GLX_E_INVALID, with a message, for a bad dtype, non-positive shapes, l > 128, fused outside 0..2,
 * NULL A, X, b or workspace, a workspace that is too small or not 256-byte aligned, mu < 0 or NaN.
 * mu = 0 is allowed. Inputs are not modified. */
int glx_certificate_workspace_bytes(int dtype, int64_t m, int64_t n, int64_t l, size_t* bytes);
/* One line: the tiles of the two passes and where the row terms run ("fused ..." or "row kernel
 * ..."). Resolved on the host; needs no device. */
int glx_certificate_describe(int dtype, int64_t m, int64_t n, int64_t l, int fused, char* out, size_t cap);
int glx_certificate(int dtype, int64_t m, int64_t n, int64_t l, const void* A, const void* X, const void* b,
                    double mu, int fused, void* G_out, double* rownorm_out, double out[8], void* workspace,
                    size_t workspace_bytes, void* stream);
/* The row terms one launch at a time (test surface), through the launchers the driver uses;
 * sums_dev = out[2..6] above as 5 device doubles; rownorm_out may be NULL.
 *   form 0: a row kernel on the given G; A and Z are unused. Where the plan of (m, n, l) takes a
 *           fused epilogue the rows run on that epilogue's panel layout (k_cert_panel) and every
 *           bit equals form 1's; elsewhere (any l <= 128, any n; m = 1 will do) the generic row
 *           layout (k_cert_row).
 *   form 1: the epilogue of G = A^T Z (k_atr_cert): G is written. GLX_E_INVALID where the plan of
 *           this shape takes no fused epilogue.
 * Workspace: glx_certificate_workspace_bytes at the same (dtype, m, n, l). */
int glx_certificate_step(int dtype, int64_t m, int64_t n, int64_t l, const void* A, const void* Z, void* G,
                         const void* x, double mu, int form, double* rownorm_out, void* sums_dev,
                         void* workspace, size_t workspace_bytes, void* stream);

/* ---- certified solve with gap-safe screening (DESIGN.md "Certified solve and screening"; additive
 * entries, the ABI version stays 2) ----
 * Solves P(x) to a stated relative duality gap: FISTA with the exact group prox and a fixed step
 * t <= 1 / lambda_max(A^T A) (caller-computed, like alpha0), stopped on the certificate above. With
 * screen != 0, every check_every iterations the certificate's dual point theta = s r and the radius
 * rho = sqrt(2 gap) give the gap-safe test  s ||g_i|| + ||a_i|| rho < mu  =>  x*_i = 0  (a_i = column
 * i of A); columns that pass leave A: the kept ones are gathered, padded with zero columns to a
 * multiple of 64, into one of two workspace buffers whenever the padded width is at most 0.9 of the
 * current one. s and rho carry a rounding guard composed on the host in float64.
 *
 * The guard (host only, needs no device): from the certificate's record of the current iterate
 * (out[8] of glx_certificate at this dtype and shape; entries 0..3 are read), mu, max_i ||a_i||,
 * sum_i ||a_i||^2 and ||b||_F to
 *   out = [s_safe, gap+, rho+]:  s_safe <= s makes s_safe r dual feasible whatever the rounding of
 *   g = A^T r; gap+ >= the true gap of (x, s_safe r); rho+ >= sqrt(2 gap+) plus the rounding of
 *   the row's own norm, so that  s_safe ||g_i|| + ||a_i|| rho+ < mu  proves x*_i = 0 with the stored
 *   row and column norms. A NaN in the record gives NaN outputs, which screen nothing. */
int glx_screen_guard(const double rec[8], double mu, int dtype, int64_t m, int64_t n, int64_t l,
                     double col_max, double col_sumsq, double b_norm, double out[3]);
/* Workspace (device bytes, 256-byte aligned) of the two one-launch entries below. */
int glx_screen_workspace_bytes(int64_t m, int64_t n, size_t* bytes);
/* norms_dev[i] = ||a_i||_2 (n device doubles) of the row-major m x n matrix A of dtype, in one
 * pass: squares accumulated in double over fixed row slabs (at most 64, a function of m) and the
 * slabs summed in slab order; stats_dev = [max_i ||a_i|| (NaN-propagating), sum_i ||a_i||^2] (device
 * doubles). Bit-reproducible. */
int glx_col_norms(int dtype, int64_t m, int64_t n, const void* A, double* norms_dev, double* stats_dev,
                  void* workspace, size_t workspace_bytes, void* stream);
/* The screening test on n rows: row i is kept unless  s row_norms[i] + col_norms[i] rho < mu  holds
 * strictly in double (one rounded product each, one rounded sum; a NaN keeps the row).
 *   mask (n bytes, may be NULL): 1 = kept;  list: the kept rows, ascending, then -1 up to
 *   count[1] (room for n rounded up to 64 entries);  count = [kept, kept rounded up to 64].
 * The list comes from an ordered scan (wave ballots, popcounts, block offsets) and is identical
 * from run to run. All pointers are device memory. */
int glx_screen_step(int64_t n, const double* row_norms, const double* col_norms, double s, double rho,
                    double mu, uint8_t* mask, int32_t* list, int32_t* count, void* workspace,
                    size_t workspace_bytes, void* stream);
/* dst (m x width, width a multiple of 64) [r, j] = src (m x src_width) [r, idx[j]], and 0 where
 * idx[j] is outside 0 .. src_width - 1 (the list's -1 tail); idx holds width device ints. src and dst
 * must not overlap. 16-byte stores where dst is 16-byte aligned. */
int glx_gather_cols(int dtype, int64_t m, int64_t src_width, const void* src, const int32_t* idx,
                    int64_t width, void* dst, void* stream);
#define GLX_CERTIFIED_MAX_HIST 64
typedef struct glx_certified_info {
  int64_t iters;         /* FISTA iterations in total                                           */
  int64_t checks;        /* certificates of the (reduced) problem taken inside the loop          */
  int64_t compactions;   /* gathers of A into a narrower buffer                                  */
  int64_t kept;          /* rows the last screening test did not prove zero (n with screen = 0)  */
  int64_t listed;        /* entries written to kept_rows_dev (0: none)                           */
  int64_t width;         /* columns of the last reduced problem (kept rounded up to 64; n without a
                            compaction)                                                          */
  int64_t rounds;        /* 1 + the times the loop resumed because the full problem's gap missed tol */
  int32_t converged;     /* the full problem's rel_gap <= tol                                    */
  int32_t fused;         /* the step ran in the epilogue of A^T r at the full width              */
  double  passes;        /* passes over A, each weighted by its width / n (the iterations' two, the
                            checks' two, a compaction's read, the column norms' one, the final
                            certificates' two)                                                   */
  double  tt;            /* seconds inside the call, stream-synchronised                         */
  double  inner_rel_gap; /* rel_gap of the reduced problem at its last check                     */
  double  cert[8];       /* glx_certificate's record of the returned x on the full problem       */
  int64_t kept_hist[GLX_CERTIFIED_MAX_HIST];   /* kept rows after each of the first 64 compactions */
} glx_certified_info;
/* Device bytes glx_certified_solve needs (screen != 0 adds the two compaction buffers: at most
 * 0.9 m n and 0.81 m n elements). */
int glx_certified_workspace_bytes(int dtype, int64_t m, int64_t n, int64_t l, int screen, size_t* bytes);
/* One line: the tiles of the two passes at the full width, where the step runs ("fused ..." or
 * "row kernel ...") and whether screening is on. Resolved on the host; needs no device. */
int glx_certified_describe(int dtype, int64_t m, int64_t n, int64_t l, int screen, char* out, size_t cap);
/* The whole solve. prob->x holds x0 on entry and the result on return; prob->method is ignored;
 * mu = prob->mu0. Checks run before the first iteration, every check_every iterations and at maxit
 * (the bound on the total). At the stop x is scattered back to n x l and the certificate of the full
 * problem on the caller's A is taken: info->cert. Where its rel_gap exceeds tol (a screened row may
 * bind the rescaling s) the loop resumes on the reduced problem with its internal target halved, at
 * most 5 times. col_norms_dev (n device doubles) with col_stats (host: [max, sum of squares]) as
 * glx_col_norms gives them, or both NULL: computed here. kept_rows_dev (may be NULL; room for n
 * rounded up to 64 device ints): its first info->listed entries receive the rows of the full problem
 * that are not proven zero at the optimum (those the last test kept; right after a compaction, the
 * columns of the reduced problem), ascending, with -1 entries for padding; info->listed = 0 (nothing
 * written) where no test ran or every row is proven zero. GLX_E_INVALID for a communicator, l > 128,
 * n >= 2^31 - 64, mu < 0 or NaN, t or tol not positive, maxit < 0, check_every < 1, a NULL or not
 * 16-byte aligned A, b or x, and a workspace that is too small or not 256-byte aligned. */
int glx_certified_solve(const glx_problem* prob, double t, double tol, int64_t maxit, int screen,
                        int check_every, const double* col_norms_dev, const double* col_stats,
                        int32_t* kept_rows_dev, void* workspace, size_t workspace_bytes,
                        glx_certified_info* info, void* stream);

/* ---- feature groups and weights (DESIGN.md "Feature groups and weights"; additive entries, the ABI
 * version stays 2) ----
 * The classical group lasso  P(x) = 1/2 ||A x - b||_F^2 + mu sum_g w_g ||x_[g]||_F : group g is the
 * contiguous row range group_ptr[g] .. group_ptr[g + 1] - 1 of the n x l iterate (the same columns of
 * A), w_g > 0 its weight. group_ptr (G + 1 int32) and weights (G doubles) are HOST arrays in every
 * entry below except glx_group_expand; they are checked before anything is launched and copied into
 * the workspace (the copy is complete on return). GLX_E_INVALID, with a message, for G < 1,
 * group_ptr[0] != 0, group_ptr[G] != n, offsets that are not strictly increasing, a weight that is
 * <= 0, NaN or infinite, l > 128, a communicator, and the row entries' pointer and workspace checks.
 * Labels that are not contiguous are the caller's to sort (glx.group_order); A is never gathered
 * for that here.
 *
 * The certificate: out = [||r||^2, <r, b>, sum_g w_g ||x_[g]||, max_g ||g_[g]|| / w_g, kkt_max,
 * sum_g kkt_g^2, nonzero groups, 0] with kkt_g = ||g_[g] + mu w_g x_[g] / ||x_[g]|| || where x_[g] != 0
 * and max(||g_[g]|| - mu w_g, 0) where it is 0; the caller composes primal, dual and gap exactly as
 * for glx_certificate (s = min(1, mu / out[3])). The A^T pass is the plain product and the group
 * terms run behind it (k_group_cert). G_out (n x l) and groupnorm_out (G doubles: ||g_[g]|| / w_g)
 * are device pointers, or NULL. */
int glx_group_certificate_workspace_bytes(int dtype, int64_t m, int64_t n, int64_t l, int64_t G, size_t* bytes);
/* One line: the tiles of the two passes and the lane layout of the group kernel for runs of up to
 * max_run rows. Resolved on the host; needs no device. */
int glx_group_certificate_describe(int dtype, int64_t m, int64_t n, int64_t l, int64_t max_run, char* out,
                                   size_t cap);
int glx_group_certificate(int dtype, int64_t m, int64_t n, int64_t l, const void* A, const void* X, const void* b,
                          double mu, int64_t G, const int32_t* group_ptr, const double* weights, void* G_out,
                          double* groupnorm_out, double out[8], void* workspace, size_t workspace_bytes,
                          void* stream);
/* The certified solve on groups: glx_certified_solve's loop, schedule and arguments. The step is the
 * plain A^T r followed by k_group_fista; with screen != 0 the test runs on groups,
 *   s ||g_[g]|| / w_g + (||A_[g]||_F / w_g) rho < mu  =>  x*_[g] = 0
 * (||A_[g]||_F bounds the spectral norm of the group's columns from above), all columns of a
 * screened group leave A at once, and the compaction rule (padded kept rows <= 0.9 of the width)
 * is the row solve's. base.kept and base.kept_hist count groups. kept_rows_dev (room for n rounded
 * up to 64 ints) and kept_groups_dev (room for G ints), either may be NULL: the rows and the groups
 * of the full problem not proven zero, ascending; base.listed / listed_groups entries are written. */
typedef struct glx_group_certified_info {
  glx_certified_info base;
  int64_t kept_groups;     /* groups the last screening test did not prove zero (G with screen = 0) */
  int64_t listed_groups;   /* entries written to kept_groups_dev (0: none)                          */
  int64_t max_run;         /* rows of the largest group                                             */
  int64_t reserved;
} glx_group_certified_info;
int glx_group_certified_workspace_bytes(int dtype, int64_t m, int64_t n, int64_t l, int64_t G, int screen,
                                        size_t* bytes);
int glx_group_certified_describe(int dtype, int64_t m, int64_t n, int64_t l, int64_t max_run, int screen,
                                 char* out, size_t cap);
int glx_group_certified_solve(const glx_problem* prob, int64_t G, const int32_t* group_ptr, const double* weights,
                              double t, double tol, int64_t maxit, int screen, int check_every,
                              const double* col_norms_dev, const double* col_stats, int32_t* kept_rows_dev,
                              int32_t* kept_groups_dev, void* workspace, size_t workspace_bytes,
                              glx_group_certified_info* info, void* stream);
/* The grouped rounding guard (host only, needs no device): glx_screen_guard's three outputs from the
 * group certificate's record, with max_g ||A_[g]||_F / w_g (gcol_max, glx_group_cnorm's maximum) in
 * place of the largest column norm, ||x||_F <= rec[2] / w_min, and the roundings of a max_run * l
 * term norm and of the stored group figures. */
int glx_group_screen_guard(const double rec[8], double mu, int dtype, int64_t m, int64_t n, int64_t l,
                           int64_t max_run, double w_min, double gcol_max, double col_sumsq, double b_norm,
                           double out[3]);
/* The group kernels one launch at a time (test surface). Workspace: glx_group_workspace_bytes(G).
 * glx_group_step: the FISTA step on S >= 1 slabs g of rows * l values (rows = n .. n + 63, the padded
 *   width; rows from n on belong to no group and come back 0 in xc, vnext, ynext): w = y - t g,
 *   xc_[g] = w_[g] max(||w_[g]|| - t mu w_g, 0) / ((||w_[g]|| < thres) + ||w_[g]||), then per element
 *   the momentum of glx_trial_fista; sums_dev = [sum g (xc - y), sum (xc - y)^2, sum_g w_g ||xc_[g]||,
 *   max |xc|] (4 device doubles).
 * glx_group_certificate_step: the group terms on a given g: sums_dev = out[2..6] of
 *   glx_group_certificate (5 device doubles); gout, groupnorm_out may be NULL.
 * glx_group_cnorm: gcn_dev[g] = sqrt(sum_{i in [g]} col_norms_dev[i]^2) / w_g in double, max_dev[0]
 *   their maximum.
 * glx_group_expand (device arrays only): kept_dev = kept_count_dev[0] groups of the current problem,
 *   ascending (glx_screen_step's list and count) -> rows_out (their rows, ascending, then -1 up to
 *   count_out[1]), the reduced problem's group_ptr_out (kept + 1), weights_out, gcn_out, and map_out =
 *   map_dev composed (map_dev NULL: identity), so it names groups of the full problem;
 *   count_out = [rows, rows rounded up to 64]. An ordered integer scan, identical from run to run. */
int glx_group_workspace_bytes(int64_t G, size_t* bytes);
int glx_group_step(int dtype, int64_t n, int64_t rows, int64_t l, int64_t G, const int32_t* group_ptr,
                   const double* weights, const void* y, const void* g, int S, const void* xk, double t, double mu,
                   double thres, double theta, double theta_next, void* xc, void* vnext, void* ynext,
                   void* sums_dev, void* workspace, size_t workspace_bytes, void* stream);
int glx_group_certificate_step(int dtype, int64_t n, int64_t l, int64_t G, const int32_t* group_ptr,
                               const double* weights, const void* x, const void* g, int S, double mu, void* gout,
                               double* groupnorm_out, void* sums_dev, void* workspace, size_t workspace_bytes,
                               void* stream);
int glx_group_cnorm(int64_t n, int64_t G, const int32_t* group_ptr, const double* weights,
                    const double* col_norms_dev, double* gcn_dev, double* max_dev, void* workspace,
                    size_t workspace_bytes, void* stream);
int glx_group_expand(const int32_t* kept_dev, const int32_t* kept_count_dev, const int32_t* group_ptr_dev,
                     const double* weights_dev, const double* gcn_dev, const int32_t* map_dev, int32_t* rows_out,
                     int32_t* group_ptr_out, double* weights_out, double* gcn_out, int32_t* map_out,
                     int32_t* count_out, void* stream);

/* ---- sample weights (DESIGN.md "Sample weights and cross-validation"; additive entries, the ABI
 * version stays 2) ----
 * Observation weights:  P_w(x) = 1/2 sum_j w_j ||(A x - b)_j||^2 + mu Omega(x),  w_j >= 0, one per row
 * j of A; Omega is the row penalty or the grouped, weighted one. Everything above carries over with
 * A~ = W^(1/2) A and b~ = W^(1/2) b in place of A and b, and neither is ever formed: A is not copied
 * and not written. The residual finalize between the two dense passes keeps the unweighted
 * r = A x - b, hands w r to the A^T pass and reduces sum w r^2 and sum w r b (k_cert_fin_w); the
 * column norms are sqrt(sum_j w_j A_ji^2) (k_col_norms_w). A 0/1 vector solves the row-subset
 * problem (a cross-validation fold), integer weights the row-duplicated one.
 *   sample_w  (device, m values of A's dtype, 16-byte aligned; may be NULL): the weights, finite and
 *             >= 0 with one > 0: the CALLER's check (glx/certificate.py check_sample_weight makes it
 *             on the host before anything is uploaded). NULL runs the sibling entry, call for call.
 *   holdout_w (the same kind of vector; may be NULL; only with sample_w): *holdout_sum receives
 *             sum_j holdout_w_j ||(A x - b)_j||^2 from the finalize's own launch (0 without it).
 * The certificate's out[0], out[1] are sum w r^2 and sum w r b; every other value and the host's
 * arithmetic are as documented for the sibling. The certified solve's final certificate of the full
 * problem is the one that takes holdout_w, so a fold's validation loss costs no pass over A.
 * col_norms_dev / col_stats of the solves are glx_col_norms_sw's. Each entry validates before any
 * launch (GLX_E_INVALID): its sibling's checks, the alignment of the two vectors, holdout_w without
 * sample_w. Workspaces: the sibling's layout with the new pieces behind it. */
int glx_certificate_sw_workspace_bytes(int dtype, int64_t m, int64_t n, int64_t l, size_t* bytes);
int glx_certificate_sw_describe(int dtype, int64_t m, int64_t n, int64_t l, int fused, char* out, size_t cap);
int glx_certificate_sw(int dtype, int64_t m, int64_t n, int64_t l, const void* A, const void* X, const void* b,
                       double mu, int fused, const void* sample_w, const void* holdout_w, void* G_out,
                       double* rownorm_out, double out[8], double* holdout_sum, void* workspace,
                       size_t workspace_bytes, void* stream);
int glx_group_certificate_sw_workspace_bytes(int dtype, int64_t m, int64_t n, int64_t l, int64_t G, size_t* bytes);
int glx_group_certificate_sw_describe(int dtype, int64_t m, int64_t n, int64_t l, int64_t max_run, char* out,
                                      size_t cap);
int glx_group_certificate_sw(int dtype, int64_t m, int64_t n, int64_t l, const void* A, const void* X,
                             const void* b, double mu, int64_t G, const int32_t* group_ptr, const double* weights,
                             const void* sample_w, const void* holdout_w, void* G_out, double* groupnorm_out,
                             double out[8], double* holdout_sum, void* workspace, size_t workspace_bytes,
                             void* stream);
int glx_certified_sw_workspace_bytes(int dtype, int64_t m, int64_t n, int64_t l, int screen, size_t* bytes);
int glx_certified_sw_describe(int dtype, int64_t m, int64_t n, int64_t l, int screen, char* out, size_t cap);
int glx_certified_solve_sw(const glx_problem* prob, const void* sample_w, const void* holdout_w, double t,
                           double tol, int64_t maxit, int screen, int check_every, const double* col_norms_dev,
                           const double* col_stats, int32_t* kept_rows_dev, void* workspace,
                           size_t workspace_bytes, glx_certified_info* info, double* holdout_sum, void* stream);
int glx_group_certified_sw_workspace_bytes(int dtype, int64_t m, int64_t n, int64_t l, int64_t G, int screen,
                                           size_t* bytes);
int glx_group_certified_sw_describe(int dtype, int64_t m, int64_t n, int64_t l, int64_t max_run, int screen,
                                    char* out, size_t cap);
int glx_group_certified_solve_sw(const glx_problem* prob, int64_t G, const int32_t* group_ptr,
                                 const double* weights, const void* sample_w, const void* holdout_w, double t,
                                 double tol, int64_t maxit, int screen, int check_every,
                                 const double* col_norms_dev, const double* col_stats, int32_t* kept_rows_dev,
                                 int32_t* kept_groups_dev, void* workspace, size_t workspace_bytes,
                                 glx_group_certified_info* info, double* holdout_sum, void* stream);
/* The weighted rounding guards (host only, need no device): glx_screen_guard / glx_group_screen_guard
 * with the weighted problem's record, column figures (glx_col_norms_sw) and b_norm = ||b~|| =
 * sqrt(sum w b^2), and one more rounding counted where w r, (w r) r, (w r) b and (w a) a are formed.
 * The unweighted guards are unchanged. */
int glx_screen_guard_sw(const double rec[8], double mu, int dtype, int64_t m, int64_t n, int64_t l,
                        double col_max, double col_sumsq, double b_norm, double out[3]);
int glx_group_screen_guard_sw(const double rec[8], double mu, int dtype, int64_t m, int64_t n, int64_t l,
                              int64_t max_run, double w_min, double gcol_max, double col_sumsq, double b_norm,
                              double out[3]);
/* The two kernels one launch at a time (test surface). Workspace: glx_screen_workspace_bytes(m, n)
 * for the column norms, (1, 1) for the finalize.
 * glx_col_norms_sw: glx_col_norms with norms_dev[i] = sqrt(sum_j sample_w_j A_ji^2); a column whose
 *   rows all weigh 0 gives exactly 0, all-ones weights give glx_col_norms' bits.
 * glx_cert_fin_sw: P = S slabs of m * l values (S = 0, P = NULL: the null product), b (m x l);
 *   r_out (may be NULL) = fl(sum of the slabs in slab order) - b, rw_out = fl(sample_w_j r),
 *   sums_dev = [sum w r^2, sum w r b, sum holdout_w r^2 (written only with holdout_w)], device
 *   doubles, each product formed as ((double) w r) r. sample_w = NULL runs the unweighted finalize
 *   instead (rw_out = r, two sums), for bit comparisons. */
int glx_col_norms_sw(int dtype, int64_t m, int64_t n, const void* A, const void* sample_w, double* norms_dev,
                     double* stats_dev, void* workspace, size_t workspace_bytes, void* stream);
int glx_cert_fin_sw(int dtype, int64_t m, int64_t l, const void* P, int S, const void* b, const void* sample_w,
                    const void* holdout_w, void* r_out, void* rw_out, double* sums_dev, void* workspace,
                    size_t workspace_bytes, void* stream);

/* ---- an unpenalised intercept (DESIGN.md "Intercept"; additive entries, the ABI version stays 2) ----
 *   P(x, c) = 1/2 sum_j w_j ||(A x + 1 c^T - b)_j||^2 + mu Omega(x),   c in R^l unpenalised,
 * with w = 1 where sample_w is NULL. c is eliminated exactly: for fixed x it is minus the weighted
 * column mean of r = A x - b, so min_c P is the problem above on the centred residual
 * r_c = r - 1 r-bar^T. Between the two dense passes the finalize becomes two launches: k_cert_csum
 * (r and its l weighted column means, combined in a fixed order by the last workgroup to arrive) and
 * k_cert_fin_c (r_c, w r_c for the A^T pass, the sums on r_c). theta = s W^(1/2) r_c satisfies the dual's
 * extra equality 1~^T theta = 0 by construction; the record keeps its layout with r_c in place of r.
 * A is neither copied nor centred.
 *   weight_sum    sigma = sum_j sample_w_j (m without sample weights), finite and > 0
 *   intercept_out l host doubles: c = -r-bar of the returned / given x
 *   holdout_sum   sum_j holdout_w_j ||(A x + c - b)_j||^2, the hold-out loss WITH the training intercept
 * The solves' col_norms_dev / col_stats are glx_col_norms_ic's: the CENTRED weighted norms and four
 * statistics. Refusals (GLX_E_INVALID, before any launch): those of the _sw entries, weight_sum not
 * finite or <= 0, intercept_out NULL. Workspaces: the _sw entry's layout with the new pieces behind it. */
int glx_certificate_ic_workspace_bytes(int dtype, int64_t m, int64_t n, int64_t l, size_t* bytes);
int glx_certificate_ic_describe(int dtype, int64_t m, int64_t n, int64_t l, int fused, char* out, size_t cap);
int glx_certificate_ic(int dtype, int64_t m, int64_t n, int64_t l, const void* A, const void* X, const void* b,
                       double mu, int fused, const void* sample_w, const void* holdout_w, double weight_sum,
                       void* G_out, double* rownorm_out, double out[8], double* holdout_sum, double* intercept_out,
                       void* workspace, size_t workspace_bytes, void* stream);
int glx_group_certificate_ic_workspace_bytes(int dtype, int64_t m, int64_t n, int64_t l, int64_t G, size_t* bytes);
int glx_group_certificate_ic_describe(int dtype, int64_t m, int64_t n, int64_t l, int64_t max_run, char* out,
                                      size_t cap);
int glx_group_certificate_ic(int dtype, int64_t m, int64_t n, int64_t l, const void* A, const void* X,
                             const void* b, double mu, int64_t G, const int32_t* group_ptr, const double* weights,
                             const void* sample_w, const void* holdout_w, double weight_sum, void* G_out,
                             double* groupnorm_out, double out[8], double* holdout_sum, double* intercept_out,
                             void* workspace, size_t workspace_bytes, void* stream);
int glx_certified_ic_workspace_bytes(int dtype, int64_t m, int64_t n, int64_t l, int screen, size_t* bytes);
int glx_certified_ic_describe(int dtype, int64_t m, int64_t n, int64_t l, int screen, char* out, size_t cap);
int glx_certified_solve_ic(const glx_problem* prob, const void* sample_w, const void* holdout_w, double weight_sum,
                           double t, double tol, int64_t maxit, int screen, int check_every,
                           const double* col_norms_dev, const double col_stats[4], int32_t* kept_rows_dev,
                           void* workspace, size_t workspace_bytes, glx_certified_info* info, double* holdout_sum,
                           double* intercept_out, void* stream);
int glx_group_certified_ic_workspace_bytes(int dtype, int64_t m, int64_t n, int64_t l, int64_t G, int screen,
                                           size_t* bytes);
int glx_group_certified_ic_describe(int dtype, int64_t m, int64_t n, int64_t l, int64_t max_run, int screen,
                                    char* out, size_t cap);
int glx_group_certified_solve_ic(const glx_problem* prob, int64_t G, const int32_t* group_ptr,
                                 const double* weights, const void* sample_w, const void* holdout_w,
                                 double weight_sum, double t, double tol, int64_t maxit, int screen, int check_every,
                                 const double* col_norms_dev, const double col_stats[4], int32_t* kept_rows_dev,
                                 int32_t* kept_groups_dev, void* workspace, size_t workspace_bytes,
                                 glx_group_certified_info* info, double* holdout_sum, double* intercept_out,
                                 void* stream);
/* The guards of the problem with an intercept (host only). col_stats = glx_col_norms_ic's four values,
 * b_norm = sqrt(sum w b^2) (uncentred), mean_sq = sum_c r-bar_c^2 of the record's certificate (the
 * squares of its intercept). out = [s_safe, gap+, rho+, slack]: row i is proven zero when
 * s_safe rn_i + cn_i rho+ < mu - slack with cn_i the centred norm. */
int glx_screen_guard_ic(const double rec[8], double mu, int dtype, int64_t m, int64_t n, int64_t l,
                        const double col_stats[4], double b_norm, double weight_sum, double mean_sq, double out[4]);
int glx_group_screen_guard_ic(const double rec[8], double mu, int dtype, int64_t m, int64_t n, int64_t l,
                              int64_t max_run, double w_min, double gcol_max, const double col_stats[4],
                              double b_norm, double weight_sum, double mean_sq, double out[4]);
/* The new kernels by themselves (test surface). Workspace: glx_intercept_workspace_bytes(m, n) for the
 * column norms, (1, 1) for the finalize.
 * glx_col_norms_ic: means_dev[i] = sum_j w_j A_ji / sigma, norms_dev[i] = sqrt(sum_j w_j (A_ji - mean_i)^2)
 *   (two launches on glx_col_norms' slabs), stats_dev = [max norm, sum norm^2, max |mean|, sum mean^2].
 * glx_cert_fin_ic: the two launches of the centring finalize on S slabs P (S = 0: the null product):
 *   rhat_out = fl(sum of the slabs) - b, means_dev = its l weighted column means, rc_out (may be NULL) =
 *   the centred residual, rw_out = fl(w rc), sums_dev = [sum w rc^2, sum w rc b, sum holdout_w rc^2 (only
 *   with holdout_w)]. sample_w = NULL: unit weights, the bits of all-ones. */
int glx_intercept_workspace_bytes(int64_t m, int64_t n, size_t* bytes);
int glx_col_norms_ic(int dtype, int64_t m, int64_t n, const void* A, const void* sample_w, double weight_sum,
                     double* norms_dev, double* means_dev, double* stats_dev, void* workspace,
                     size_t workspace_bytes, void* stream);
int glx_cert_fin_ic(int dtype, int64_t m, int64_t l, const void* P, int S, const void* b, const void* sample_w,
                    const void* holdout_w, double weight_sum, void* rhat_out, double* means_dev, void* rc_out,
                    void* rw_out, double* sums_dev, void* workspace, size_t workspace_bytes, void* stream);

/* ---- multi-GPU (row-sharded A; A^T r all-reduced, or reduce-scattered with the row-sharded step) ---- */
#define GLX_COMM_ID_BYTES 128
int  glx_comm_unique_id(uint8_t id[GLX_COMM_ID_BYTES]);
int  glx_comm_create(glx_comm** out, const uint8_t id[GLX_COMM_ID_BYTES], int nranks, int rank);
/* Host-staged transport (testing: several ranks sharing one GPU, which RCCL refuses). Each
 * all-reduce synchronises the stream, copies the buffer to pinned host memory, calls
 * fn(host_buf, count, dtype, user) — which must sum it in place across ranks and return 0 —
 * and copies it back. Not a performance path. */
typedef int (*glx_host_allreduce_fn)(void* host_buf, int64_t count, int dtype, void* user);
int  glx_comm_create_host(glx_comm** out, int nranks, int rank, glx_host_allreduce_fn fn, void* user);
/* in-place sum all-reduce of `count` elements of dtype on `stream` (exposed for tests) */
int  glx_comm_allreduce(glx_comm* c, void* buf, int64_t count, int dtype, void* stream);
/* The row-sharded schedule's collectives (round 5, exposed for tests), in place over nranks
 * chunks of `count` elements: reduce-scatter leaves in chunk `rank` the sum over ranks of that
 * chunk (other chunks undefined); all-gather sends chunk `rank` and receives every chunk. The
 * host transport runs both through the all-reduce callback (all-gather exactly: the chunks it
 * does not own are -0.0). */
int  glx_comm_reduce_scatter(glx_comm* c, void* buf, int64_t count, int dtype, void* stream);
int  glx_comm_all_gather(glx_comm* c, void* buf, int64_t count, int dtype, void* stream);
/* Progress record, safe to call from another thread (round 6): out = {collectives issued,
 * collectives the host transport completed (-1 for RCCL), kind of the last one issued (1 all-reduce,
 * 2 reduce-scatter, 3 all-gather), RCCL's asynchronous error (ncclCommGetAsyncError; 0 none, -1
 * aborted)}. A session whose host wait on RCCL sees an asynchronous error, or waits longer than
 * GLX_WAIT_TIMEOUT_S (default 300 s), aborts the communicator and fails with GLX_E_RCCL and this
 * record in glx_last_error(). */
int  glx_comm_progress(glx_comm* c, int64_t out[4]);
void glx_comm_destroy(glx_comm* c);

/* ---- the sparse-group lasso (DESIGN.md "Sparse-group lasso"; csrc/kernels_sgl.hip, csrc/group.cpp) ----
 *   P(x) = 1/2 ||A x - b||_F^2 + mu (row_ratio sum_i ||x_i||_2 + (1 - row_ratio) sum_g w_g ||x_[g]||_F)
 * with the groups of the grouped entries (host group_ptr / weights, validated the same way) and
 * row_ratio in [0, 1] (GLX_E_INVALID otherwise, NaN included). Write a = row_ratio mu and c_g =
 * (1 - row_ratio) mu w_g. The dual constraint is phi_g(1) <= c_g on A^T theta for every group, phi_g(s) =
 * sqrt(sum_{i in g} (s rho_i - a)_+^2) with rho_i = ||(A^T theta)_i||; theta = s r with s = min(1, min_g s_g),
 * s_g = sup{s : phi_g(s) <= c_g}. row_ratio = 0 takes the grouped entry's path, call for call. No entry takes
 * an intercept. Single GPU.
 *
 * glx_sgl_certificate[_sw]: out = 12 doubles. out[0..7] is the grouped record with out[2] = the penalty
 *   row_ratio sum ||x_i|| + (1 - row_ratio) sum w_g ||x_[g]||, out[3] = mu / min_g s_g (so that the grouped
 *   composition of the scale, min(1, mu / out[3]), holds; 0 where every s_g is +inf), out[4], out[5] the
 *   largest KKT distance and the sum of their squares (a nonzero row of a nonzero group: ||g_i + a x_i /
 *   ||x_i|| + c_g x_i / ||x_[g]|| ||; a zero row of one: (rho_i - a)_+; a zero group: (phi_g(1) - c_g)_+,
 *   one term), out[6] nonzero groups, out[7] nonzero rows; out[8] = min_g s_g (unclamped), out[9] = the
 *   same of the padded solve (here unpadded), out[10] = max_i rho_i, out[11] = 0. rownorm_out (may be
 *   NULL): rho_i, n doubles. _sw: sample weights as in glx_group_certificate_sw (sample_w NULL: none).
 * glx_sgl_certified_solve[_sw]: glx_group_certified_solve[_sw] with the two-level prox, the two-level
 *   gap-safe test (row: s rho_i + ||a_i|| R < a; group: phi_g(s) + ||A_[g]||_F R < c_g) under
 *   glx_sgl_screen_guard, and compactions that remove rows from inside groups. info->base counts groups in
 *   kept and kept_hist as the grouped solve does; kept_row_hist counts rows. */
typedef struct glx_sgl_certified_info {
  glx_group_certified_info base;
  double row_ratio;
  int64_t reserved[3];
  int64_t kept_row_hist[GLX_CERTIFIED_MAX_HIST];   /* kept rows after each of the first 64 compactions */
} glx_sgl_certified_info;
int glx_sgl_certificate_workspace_bytes(int dtype, int64_t m, int64_t n, int64_t l, int64_t G, size_t* bytes);
int glx_sgl_certificate_describe(int dtype, int64_t m, int64_t n, int64_t l, int weighted, char* out, size_t cap);
int glx_sgl_certificate(int dtype, int64_t m, int64_t n, int64_t l, const void* A, const void* X, const void* b,
                        double mu, double row_ratio, int64_t G, const int32_t* group_ptr, const double* weights,
                        void* G_out, double* rownorm_out, double* out, void* ws, size_t wsb, void* stream);
int glx_sgl_certificate_sw(int dtype, int64_t m, int64_t n, int64_t l, const void* A, const void* X, const void* b,
                           double mu, double row_ratio, int64_t G, const int32_t* group_ptr, const double* weights,
                           const void* sample_w, const void* holdout_w, void* G_out, double* rownorm_out,
                           double* out, double* holdout_sum, void* ws, size_t wsb, void* stream);
int glx_sgl_certified_workspace_bytes(int dtype, int64_t m, int64_t n, int64_t l, int64_t G, int screen,
                                      int weighted, size_t* bytes);
int glx_sgl_certified_describe(int dtype, int64_t m, int64_t n, int64_t l, int64_t max_run, int screen, int weighted,
                               char* out, size_t cap);
int glx_sgl_certified_solve(const glx_problem* prob, double row_ratio, int64_t G, const int32_t* group_ptr,
                            const double* weights, double t, double tol, int64_t maxit, int screen, int check_every,
                            const double* col_norms_dev, const double* col_stats, int32_t* kept_rows_dev,
                            int32_t* kept_groups_dev, void* ws, size_t wsb, glx_sgl_certified_info* info,
                            void* stream);
int glx_sgl_certified_solve_sw(const glx_problem* prob, double row_ratio, int64_t G, const int32_t* group_ptr,
                               const double* weights, const void* sample_w, const void* holdout_w, double t,
                               double tol, int64_t maxit, int screen, int check_every, const double* col_norms_dev,
                               const double* col_stats, int32_t* kept_rows_dev, int32_t* kept_groups_dev, void* ws,
                               size_t wsb, glx_sgl_certified_info* info, double* holdout_sum, void* stream);
/* The sparse-group rounding guard (host only, needs no device). rec: the record above; s_pad: min_g s_g of
 * the dual solve on the padded row norms. out = [mul, add, s_safe, gap+, rho+]: mul rho_i + add bounds the
 * exact ||a_i^T r^|| of every row (the padding of the dual solve and of the screening test), s_safe =
 * min(1, s_pad), gap+ and rho+ as in glx_group_screen_guard with ||x||_F <= rec[2] / (row_ratio +
 * (1 - row_ratio) w_min). col_max = the largest column norm. NaN propagates. _sw: the weighted figures. */
int glx_sgl_screen_guard(const double* rec, double s_pad, double mu, double row_ratio, int dtype, int64_t m,
                         int64_t n, int64_t l, int64_t max_run, double w_min, double col_max, double col_sumsq,
                         double b_norm, double* out);
int glx_sgl_screen_guard_sw(const double* rec, double s_pad, double mu, double row_ratio, int dtype, int64_t m,
                            int64_t n, int64_t l, int64_t max_run, double w_min, double col_max, double col_sumsq,
                            double b_norm, double* out);
/* One launch at a time (ws: glx_group_workspace_bytes(G)):
 * glx_sgl_step: glx_group_step with the two-level prox: w = y - t g, u_i = (1 - t a / ||w_i||)_+ w_i,
 *   q_g = sqrt(sum_{i in g} (||w_i|| - t a)_+^2), x_[g] = (1 - t c_g / q_g)_+ u_[g]; sums[2] = the penalty of
 *   xc. A zero row or group is +0.
 * glx_sgl_certificate_step: sums = [penalty, max_i rho_i, max kkt, sum kkt^2, nonzero groups, nonzero rows]
 *   (6 doubles); rownorm_out (may be NULL): rho_i = ||g_i||, n doubles; gout (may be NULL): g.
 * glx_sgl_dual_scale: two solves q = 0, 1 on p_i = mul_q rho_i + add_q: sg_dev (may be NULL, 2 G doubles)
 *   = the unclamped s_g, +inf where every p_i = 0, a / max_i p_i where cb = 0; negmin_dev[q] = -min_g s_g.
 *   s_g is the feasible end of the bracket [0, (a + c_g) / max_i p_i] after 56 halvings: a point at which
 *   the kernel evaluated phi_g <= c_g, at most (a + c_g) / max_i p_i * 2^-56 below the exact value.
 * glx_sgl_screen: keep_dev[i] = 0 where s p_i + col_norms[i] rad < a_lo or, with group_test != 0, where the
 *   row's group has sqrt(sum_i (s p_i - a_lo)_+^2) / w_g + gcn_g rad < cb_lo; p_i = mul rho_i + add;
 *   group_keep_dev (may be NULL, G): the group keeps a row; counts_dev = [such groups, kept rows]. NaN keeps.
 * glx_sgl_expand (device arrays only): keep_dev -> rows_out (the kept rows, ascending, then -1 up to
 *   count_out[3]), the reduced group_ptr_out / weights_out / gcn_out / map_out over the groups that keep a
 *   row (gcn carried over: the larger value is the safe one), count_out = [groups, rows, rows, rows
 *   rounded up to 64]. */
int glx_sgl_step(int dtype, int64_t n, int64_t rows, int64_t l, int64_t G, const int32_t* group_ptr,
                 const double* weights, const void* y, const void* g, int S, const void* xk, double t, double mu,
                 double row_ratio, double thres, double theta, double theta_next, void* xc, void* vnext, void* ynext,
                 void* sums_dev, void* ws, size_t wsb, void* stream);
int glx_sgl_certificate_step(int dtype, int64_t n, int64_t l, int64_t G, const int32_t* group_ptr,
                             const double* weights, const void* x, const void* g, int S, double mu, double row_ratio,
                             void* gout, double* rownorm_out, void* sums_dev, void* ws, size_t wsb, void* stream);
int glx_sgl_dual_scale(int64_t n, int64_t G, const int32_t* group_ptr, const double* weights,
                       const double* rownorms_dev, double a, double cb, double mul0, double add0, double mul1,
                       double add1, double* sg_dev, double* negmin_dev, void* ws, size_t wsb, void* stream);
int glx_sgl_screen(int64_t n, int64_t G, const int32_t* group_ptr, const double* weights, const double* rownorms_dev,
                   const double* col_norms_dev, const double* gcn_dev, double s, double mul, double add, double rad,
                   double a_lo, double cb_lo, int group_test, int32_t* keep_dev, int32_t* group_keep_dev,
                   double* counts_dev, void* ws, size_t wsb, void* stream);
int glx_sgl_expand(int64_t G, const int32_t* keep_dev, const int32_t* group_ptr_dev, const double* weights_dev,
                   const double* gcn_dev, const int32_t* map_dev, int32_t* rows_out, int32_t* group_ptr_out,
                   double* weights_out, double* gcn_out, int32_t* map_out, int32_t* count_out, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* GLX_H_ */
