// glx_internal.h — declarations shared by the HIP kernels and the host-side driver.
#pragma once

#include <hip/hip_ext.h>
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stddef.h>

#include <cstdlib>
#include <cstring>
#include <string>
#include <tuple>
#include <utility>
#include <vector>

#include "glx.h"
#include "glx_tiles.h"

namespace glx {

// error carried to the C ABI boundary (never crosses it)
struct Error {
  int code;
  std::string msg;
};
extern thread_local std::string g_last_error;

// Kernel-attached HIP-event timing (solver.cpp prof_begin / prof_end). A sampled A@X / A^T R /
// gather launch sets this slot; the next glx_launch on the thread hands the two events to
// hipExtLaunchKernel, which stamps them with that kernel's own start and end, and clears it.
// Round 3: hipEventRecord around the launch instead put two marker packets in the queue, each
// opening a ~6 us gap before the next kernel (profiles/r3_timeline/: the driver-form command,
// every second launch timed, ran 5 gaps per two iterations, ~3-4 % of its time).
struct LaunchTiming {
  hipEvent_t start = nullptr, stop = nullptr;
};
extern thread_local LaunchTiming g_launch_timing;

template <typename... P, std::size_t... I>
inline hipError_t ext_launch(void (*kern)(P...), dim3 g, dim3 b, uint32_t sh, hipStream_t st,
                             std::tuple<P...>& t, std::index_sequence<I...>, hipEvent_t e0,
                             hipEvent_t e1) {
  void* args[sizeof...(P) > 0 ? sizeof...(P) : 1] = {static_cast<void*>(&std::get<I>(t))...};
  return hipExtLaunchKernel(reinterpret_cast<const void*>(kern), g, b, args, sh, st, e0, e1, 0);
}
// hipLaunchKernelGGL, or the timed form when a timing slot is pending. The arguments are
// converted to the kernel's own parameter types first (hipExtLaunchKernel takes raw pointers
// to them, so an int passed for an int64_t must not reach it unconverted).
template <typename... P, typename... A>
inline void glx_launch(void (*kern)(P...), dim3 g, dim3 b, uint32_t sh, hipStream_t st, A&&... a) {
  static_assert(sizeof...(P) == sizeof...(A), "argument count");
  LaunchTiming& lt = g_launch_timing;
  if (lt.start != nullptr) {
    std::tuple<P...> t(static_cast<P>(std::forward<A>(a))...);
    const hipEvent_t e0 = lt.start, e1 = lt.stop;
    lt = LaunchTiming{};
    const hipError_t e = ext_launch(kern, g, b, sh, st, t, std::index_sequence_for<P...>{}, e0, e1);
    if (e != hipSuccess) {
      // the events were not taken: hand the slot back, so prof_end (or the session's destructor)
      // returns them to the pool instead of losing them
      lt = LaunchTiming{e0, e1};
      throw Error{GLX_E_HIP, std::string("timed kernel launch: ") + hipGetErrorString(e)};
    }
    return;
  }
  hipLaunchKernelGGL(kern, g, b, sh, st, std::forward<A>(a)...);
}

constexpr int kMaxBlocks = 1024;   // grid cap of every reducing kernel (size of a partials row)
constexpr int kMaxRedVals = 6;     // max scalars one reducing kernel produces
constexpr int kMaxL = 128;         // largest l (columns of x) supported by the row kernels
// Arrival tickets: kTicketShards per-XCD counters plus one final counter, each on its own
// 128-B line (32 unsigned words apart). Word 0 = final counter, shard s at (1 + s) * 32.
constexpr int kTicketShards = 8;
constexpr int kTicketStride = 32;
constexpr int kTicketBytes = 2048;  // >= (kTicketShards + 1) * 128, keeps 256-B alignment

// Deterministic grid-wide reduction target: each block writes its partial to
// part[v * kMaxBlocks + block]; the last block (arrival ticket) sums them in block order
// and writes out[v]. `ticket` (kTicketBytes) must be zero before the first launch; the last
// block resets it.
struct Red {
  double* part;
  unsigned* ticket;
  double* out;     // kMaxRedVals consecutive doubles (caller picks the slots)
  // device-controlled batches (solver.cpp dc_run): the whole launch is skipped, uniformly over
  // the grid (nobody touches a ticket or counter), when skip != NULL and *skip is neither 0 nor
  // skip_pass
  const int* skip = nullptr;
  int skip_pass = 0;
  // 1: every workgroup stores its NV block values at part[slot * NV + j] and returns (no tickets,
  // no out): the row-sharded trial's partials ride the all-gather (ShardPub)
  int parts_only = 0;
};

// Device-side line-search decision of a device-controlled ProxGD batch (solver.cpp dc_batch),
// run by the last block of the trial's residual finalize once the residual sums are final
// (gl_ProxGD_primal.py:86-99 Armijo test, :118-125 stop rule). ring == NULL: off.
//   state[0..3] = gx (1/2 ||A thr(x) - b||^2), f and sparsity of the last record, stable count
//   tr = the trial's six sums (k_prox_pgd / k_atr_prox), t = the trial's step
// On acceptance the next record (f, s) and the stop rule are evaluated and the state advances.
// *abort = 0 (accepted), pass (accepted, the next record stops the phase, or code 3), -1 (rejected):
// the speculative gradient queued right behind this decision runs on 0 and on this tag
// (Red::skip_pass), the rest of the batch only on 0. ring[10] = 0, 1 (stop), 2 (rejected),
// 3 (FProxGD: accepted, nnz budget exceeded).
// rec[0..10] (device) = the four residual sums, the six trial sums and the code as a double.
// The speculative kernel queued behind the decision hands rec to the host from its publisher
// workgroup (Pub), also when the decision cancels it, so the PCIe write latency stays off the
// finalize's critical path.
//
// mode 1 = FProxGD's backtracking test (gl_FProxGD_primal.py:89-103): state[0] = ||A y - b||^2 of
// the current y (not halved), the test g(xc) <= g(y) + <g, xc - y> + ||xc - y||^2 / (2t) from the
// batch's residual sums and the trial's four sums, and on acceptance state[0] = ||A y_next - b||^2.
// A gathered (split-candidate) batch also checks nnz(e_c) = out[2] against nnz_budget (>= 0): above
// it the next batches are dense on the host path (solver.cpp kFistaDenseRun), so the decision
// cancels the batch behind it like a stop (code 3: accepted, the speculative kernel runs).
struct Ctl {
  double* rec = nullptr;
  double* state = nullptr;
  int* abort = nullptr;
  const double* tr = nullptr;
  double tag = 0.0, t = 0.0, mu0 = 0.0, ftol = 0.0, nl = 1.0;
  double nnz_budget = -1.0;
  int stable_thr = 0, use_sp = 1, emode = 0;
  int mode = 0;    // 0 ProxGD, 1 FProxGD
  int pass = 0;    // nonzero; the abort word's value for "stop" (Red::skip_pass of the kernel behind)
};
constexpr int kCtlRec = 16;        // doubles per ring record
constexpr int kCtlMaxBatch = 64;   // ring records

// A scalar packet for the host (what k_publish writes) carried by a kernel launch as one extra
// workgroup (publisher_first, glx_device.h); host == NULL: none.
struct Pub {
  const double* s = nullptr;
  int ns = 0;
  double* host = nullptr;
  unsigned* host_seq = nullptr;
  unsigned seq = 0;
  const double* s2 = nullptr;   // host[off2 .. off2 + n2) come from s2 instead of s
  int off2 = 0, n2 = 0;
  const double* s3 = nullptr;   // host[off3 .. off3 + n3) come from s3 (a snapshot)
  int off3 = 0, n3 = 0;
  // Round 5, deferred reductions: workgroup partials (Red::parts_only layout: dnv values per
  // slot, dnp slots) that the publishing workgroup reduces (dmax bit j: max) into dout[0, dnv)
  // before it copies the packet, so the kernels that produced them skip their grid reduction's
  // serial tail (SessionMode::defer)
  const double* dpart[2] = {nullptr, nullptr};
  int dnp[2] = {0, 0}, dnv[2] = {0, 0};
  unsigned dmax[2] = {0u, 0u};
  double* dout[2] = {nullptr, nullptr};
};

// Launch plan of the two dense products for one (dtype, m, n, l): the tiles (records of
// glx_tiles.h, chosen at plan time; a launch never searches the table) and their splits.
struct GemmPlan {
  int esize;        // 4 or 8
  int64_t m, n, l;
  // A @ X  ->  P[ax_S][m][l] partial slabs (summed by finalize_residual)
  const AxTile* ax[4];   // per number of batched right-hand sides (index 1..3)
  int ax_S;         // K (= n) splits across workgroups with one right-hand side
  int axb_S[4];     // ... per number of right-hand sides ([1] mirrors ax_S)
  int ax_xmap;      // MFMA: group K splits by XCD (L2 locality of X)
  int ax_lb;        // VALU: column block width (1,2,4,8); ax_ncb = ceil(l / ax_lb)
  int ax_vec;       // VALU: 16-byte loads
  // A^T R  ->  Gp[atr_S][n][l]
  const AtrTile* atr;
  int atr_S;        // M (= m) splits across workgroups
  int atr_lb, atr_vec;   // VALU
  // Infinity-Cache hand-off between the two non-temporal passes (Session sets them; 0 = off):
  // the last ~that many MiB a pass reads load with the default policy (kernel arguments, so
  // every session and device gets its own value)
  int ax_keep_mib = 0, atr_keep_mib = 0;
};

// ---- the launch planner (planner.cpp, host only) ----
inline int64_t cdiv(int64_t a, int64_t b) { return (a + b - 1) / b; }
inline int64_t clampi(int64_t v, int64_t lo, int64_t hi) { return v < lo ? lo : (v > hi ? hi : v); }
constexpr int64_t kTargetWaves = 2048;   // 8 waves per CU on 256 CUs
constexpr int kMaxSplit = 64;
inline int env_int(const char* name, int dflt) {
  const char* v = std::getenv(name);
  return (v && *v) ? std::atoi(v) : dflt;
}
// One knob of the planner (planner.cpp Knobs) or of a session's mode (SessionKnobs). set(): the
// variable is present, which makes it an override: the shape-dependent choices stand back.
struct EnvInt {
  const char* s;
  explicit EnvInt(const char* name) : s(std::getenv(name)) {}
  bool set() const { return s != nullptr; }
  int or_(int dflt) const { return (s && *s) ? std::atoi(s) : dflt; }
  bool on() const { return or_(1) != 0; }   // a switch that defaults to on
  bool is(const char* v) const { return s != nullptr && std::strcmp(s, v) == 0; }   // exactly this text
  // present: its number (an empty value reads 0), else dflt
  int num(int dflt) const { return s ? std::atoi(s) : dflt; }
  double real(double dflt) const { return s ? std::atof(s) : dflt; }
};
// ax_variant: a tile code of glx_tiles.h, or 0 (GLX_AX_VARIANT, else the planner's choice)
GemmPlan make_plan(int esize, int64_t m, int64_t n, int64_t l, int ax_variant);
// make_plan, then the method-level A^T R choice of a session (the fused trial's tiles)
GemmPlan session_plan(const glx_problem& P, const glx_opts& O);
// K split (number of partial slabs per source) of an A@X launch with nsrc right-hand sides
inline int ax_split(const GemmPlan& p, int nsrc) { return nsrc > 1 ? p.axb_S[nsrc] : p.ax_S; }
inline int ax_split_max(const GemmPlan& p) {
  int s = p.ax_S;
  for (int k = 2; k <= 3; ++k) s = s > p.axb_S[k] ? s : p.axb_S[k];
  return s;
}
// largest K split any A@X variant (single or batched) plans for this shape
int max_ax_split(int esize, int64_t m, int64_t n, int64_t l);
// one-line description of the kernels and splits a plan launches (glx_plan_describe)
std::string describe_plan(const GemmPlan& p);
// what a plan can carry (the launchers' preconditions): the scalar packet, the fused A e form
// (launch_ax_egat), the derive form (launch_ax_derive), a fused trial and its reducing slots
bool ax_pub_ok(const GemmPlan& p, int nsrc);
bool ax_egat_ok(const GemmPlan& p, int esize);
bool ax_derive_ok(const GemmPlan& p, int esize);
bool atr_prox_ok(const GemmPlan& p);
int atr_prox_slots(const GemmPlan& p, bool pub);

// ---- a session's mode (session_mode.cpp, host only) ----
// Every environment variable a session's mode depends on, read once per session_mode call and
// never cached (tests change the environment between calls in one process). The planner's knobs
// are the planner's (planner.cpp Knobs: GLX_FUSED_TRIAL's presence is an override there, its
// value a switch here); the launch knobs stay with their kernels (kernels_*.hip).
struct SessionKnobs {
  EnvInt dc_batch{"GLX_DC_BATCH"}, shard_rows{"GLX_SHARD_ROWS"}, split_f32{"GLX_SPLIT_F32"},
      split_cand{"GLX_SPLIT_CAND"}, split_fista{"GLX_SPLIT_FISTA"}, split_nnz{"GLX_SPLIT_NNZ"},
      ae_fused{"GLX_AE_FUSED"}, ae_hyb_rows{"GLX_AE_HYB_ROWS"}, gemv_fused{"GLX_GEMV_FUSED"},
      unfused_spec{"GLX_UNFUSED_SPEC"}, fused_trial{"GLX_FUSED_TRIAL"}, readback{"GLX_READBACK"},
      attach_pub{"GLX_ATTACH_PUB"}, spec_grad{"GLX_SPEC_GRAD"}, spec_ax_pub{"GLX_SPEC_AX_PUB"},
      shard_derive{"GLX_SHARD_DERIVE"}, defer_red{"GLX_DEFER_RED"}, ax_keep_mib{"GLX_AX_KEEP_MIB"},
      atr_keep_mib{"GLX_ATR_KEEP_MIB"}, fin_head{"GLX_FIN_HEAD"};
};
constexpr int kMaxShardRanks = 64;   // ranks (or modelled ranks) of the row-sharded schedules
// The row-sharded schedule of ProxGD (solver.cpp iter_proxgd_shard) / FProxGD (iter_fista_shard):
// this rank's rows [row0, row0 + rows) of n, `ranks` row blocks (cranks communicator ranks; they
// differ only in the timing model)
struct ShardMode {
  bool on = false, fista = false, model = false;
  int ranks = 1, rank = 0, cranks = 1;
  int64_t rows = 0, row0 = 0;
  int nbp = 0, nbf = 0;   // k_prox_pgd's workgroups on `rows` rows, the trial finalize's
  int stv = 6;            // values per trial workgroup partial in the chunk (FProxGD: 4)
  int chunk = 0;          // doubles per rank's chunk
  bool zskip = false;     // the gathered p serves as e (bitmap / list gathers)
  bool derive = false;    // round 6: the speculative derive inside the dense pass (AxDerive)
  int64_t moff = 0;       // doubles into a rank's chunk: its row masks + column bitmaps (derive)
};
// What a session launches, resolved once from the problem, the options and the environment;
// Session<T> (solver.cpp) lays out its workspace from it and iterates by it.
struct SessionMode {
  int method = 0, esize = 8;
  int64_t m = 0, n = 0, l = 0;
  bool comm = false;              // the problem has a communicator
  GemmPlan plan{};                // session_plan with the two keep_mib values
  int64_t fh_cap = 0;             // objective history entries
  int smode = 0;                  // split-candidate trial: 0 off, 1 A e from the transposed copy of A
  int gform = 0;                  // A e: 0 bitmap gather, 1 k_at_rows, 2 lists + gather (gather_form)
  bool rows_form = false;         // gform == 1: A e by k_at_rows (round 5), gsplit slabs
  int gsplit = 1;
  bool egat = false;              // round 6: A e inside the dense pass (launch_ax_egat), gsplit = its S
  double hyb_rows = 0.0;          // round 6: > 0: the fused form per trial from this many flagged rows
  double nnz_budget = 0.0;        // nnz(e_c) above which the dense batch is cheaper
  bool emode = false;             // split-candidate ProxGD: trials write e = p - p_thr, not z
  bool fsplit = false;            // split-candidate FProxGD
  bool spin_readback = true, attach_ok = true;
  bool spec_off = false;          // GLX_SPEC_GRAD=0
  bool spec_ax_pub = true;        // GLX_SPEC_AX_PUB=0: the packet rides k_prox_pgd instead
  bool unfused_spec = false;      // one GPU, a plan without the fused trial: the communicator form
  bool fused_ok = false, fused_fista_ok = false;   // the trial is queued speculatively (ProxGD / FProxGD)
  int dc_window = 0;              // device-controlled iterations in flight (0: the host decides)
  int nsets = 2;                  // gradient sets
  bool defer = false;             // deferred reductions (single GPU)
  int gemv_blocks = 0;            // SGD / GD, l = 1: workgroups of the one-pass form (0: two passes)
  // round 8: the speculative trial's finalize may run at the head of k_atr_prox (the path asks
  // for it; the session still checks co-residency on its device, fin_head_fits)
  bool fin_head = false;
  ShardMode sh;
};
SessionMode session_mode(const glx_problem& P, const glx_opts& O);
// The co-residency guard of the finalize head: every workgroup of the launch (n / 64 panels + the
// publisher) waits for all the others, so all of them must fit on the device at once.
bool fin_head_fits(int64_t n, int cus, int per_cu);
// the kernels the session launches (glx_session_describe, glx_mode_describe)
std::string describe_mode(const SessionMode& md);

// ---- dense products (kernels_gemm.hip) ----
// A @ [X[0] | .. | X[nsrc-1]] (nsrc <= 3, each n x l) in one pass over A: partial slabs
// P[src][ax_split(p, nsrc)][m][l]; skipped entirely unless gate == NULL or *gate == epoch.
// pub.host != NULL: the launch also hands that scalar packet to the host from its first
// workgroup (needs ax_pub_ok: an LDS or LDS-DMA tile for nsrc).
template <typename T>
void launch_ax(const GemmPlan& p, int nsrc, const T* A, const T* const* X, T* P, const int* gate,
               int epoch, hipStream_t st, Pub pub = Pub{});
// an LDS-DMA A @ X tile (kernels_axdma.hip); false: not built for T and nsrc
template <typename T>
bool launch_ax_dma(const GemmPlan& p, const AxTile* tile, int nsrc, int S, const T* A, const T* const* X,
                   T* P, const int* gate, int epoch, hipStream_t st, Pub pub);
// Round 6: the split-candidate trial's A e inside its dense pass (NS's one-source f64 LDS-DMA tile
// 92278): the pass streams A p (X = the candidate p) on MFMA and, for the entries the column
// bitmaps behind zf flag (glx_device.h zf_bitmaps; there e = p), accumulates A[:, k] e[k, c] on
// VALU from the A and p chunks already in LDS: no transposed copy of A, no gather pass, no second
// source. P[S][m][l] = A p slabs, Pe[S][m][l] = the A e slabs (one per K split); the finalize's
// chain mode 2 forms A p - b and A p_thr - b = (A p - b) - A e.
struct EGat {
  const void* E = nullptr;               // unused (e is read from the staged p)
  const unsigned short* bm = nullptr;    // zf_bitmaps(zf, n): column c's u16 words at c * bstride
  int64_t bstride = 0;                   // zf_npad(n) / 16
  void* Pe = nullptr;
};
template <typename T>
bool launch_ax_egat(const GemmPlan& p, const T* A, const T* X, T* P, const int* gate, int epoch,
                    hipStream_t st, Pub pub, const EGat& eg);
// Infinity-Cache hand-off between the passes (tuning experiment; MiB of A fetched with the
// default policy at the end of a non-temporal pass; 0 = off): A@X (LDS-DMA tile) / A^T R
template <typename T>
void launch_atr(const GemmPlan& p, const T* A, const T* R, T* Gp, hipStream_t st);
// ProxGD trial fused into A^T R (needs atr_prox_ok: MFMA panels, WL 0, at most 8 K splits):
// G = A^T R, then p = prox(x - t G), p_thr, z and the six trial sums of k_prox_pgd into red
// (zf != NULL: z = e = p - p_thr and its row flags, as launch_prox_pgd).
// With S = atr_S > 1 K splits the blocks write slabs Gp[S][n][l] and the last block of each
// 64-row panel (counter pcnt[panel], zero before the first launch, reset by that block) sums
// them in slab order and runs the trial.
// head != NULL (round 8; f64, atr_prox_head_ok): the launch first runs the residual finalize that
// produces R — launch_finalize_residual's two-source forms with Red::parts_only, the same
// 256-thread blocks walked by the panel workgroups (block w, w + panels, ...), the same bits —
// while its first rows of A are in flight, and every workgroup waits for all of them before it
// reads R. Needs every workgroup of the launch resident at once (fin_head_fits).
struct FinHead {
  const double* P = nullptr;     // the slabs, as launch_finalize_residual's P with nsrc = 2
  const double* B = nullptr;
  double* R0 = nullptr;          // may be NULL with chain
  double* R1 = nullptr;          // the launch's R
  const double* cx = nullptr;    // the count's array (cn values), or NULL
  const double* cmax = nullptr;  // *cmax, or cmax_parts / cmax_np / cmax_nv as launch_finalize_residual
  const double* cmax_parts = nullptr;
  double* part = nullptr;        // 4 sums per block, Red::parts_only layout
  unsigned* ticket = nullptr;    // kTicketBytes, zero: the arrivals of this launch
  unsigned* ticket_next = nullptr;   // may be NULL: zeroed for the next launch (never `ticket`)
  int* abort = nullptr;          // set to 1 by a workgroup whose wait ran out (~1 s); it stores nothing
  int64_t ml = 0, cn = 0;
  int S = 1, S0 = 0, chain = 0, cmax_np = 0, cmax_nv = 6;
  int nvb = 0;                   // the finalize's 256-thread blocks: finalize_blocks(ml, S, S0, cn)
};
// the plan's fused trial takes a head for this finalize (f64, WL 0, one K split, at most
// kSlabLoads slabs per source)
bool atr_prox_head_ok(const GemmPlan& p, int S, int S0);
// workgroups of the head kernel one CU holds at once (hipOccupancyMaxActiveBlocksPerMultiprocessor)
// and the device's CU count; the guard itself is session_mode.cpp's fin_head_fits
void atr_prox_head_capacity(const GemmPlan& p, int* cus, int* per_cu);
template <typename T>
void launch_atr_prox(const GemmPlan& p, const T* A, const T* R, T* G, const T* x, T* pp, T* pthr,
                     T* z, double t, double mu, double thres, Red red, hipStream_t st, Pub pub = Pub{},
                     T* Gp = nullptr, unsigned* pcnt = nullptr, unsigned* zf = nullptr,
                     const FinHead* head = nullptr);
// FISTA trial fused into A^T R (same plan condition): G = A^T R, then xc, v_next, y_next and the
// four trial sums of k_fista_trial (PROX) into red (ec, zf: as launch_fista_trial).
template <typename T>
void launch_atr_fista(const GemmPlan& p, const T* A, const T* R, T* G, const T* y, const T* xk,
                      T* xc, T* vn, T* yn, double t, double mu, double thres, double theta,
                      double theta_next, Red red, hipStream_t st, Pub pub = Pub{},
                      T* Gp = nullptr, unsigned* pcnt = nullptr, T* ec = nullptr,
                      unsigned* zf = nullptr);

// Dual ADMM's row step fused into g = A^T z (same plan condition as launch_atr_prox, and the
// plan's tile built `fused` for T): G = A^T Z, then u+, x+, r of launch_admm_dual and its two sums
// into red. Gp / pcnt: the slabs and per-panel counters of K splits, as launch_atr_prox.
template <typename T>
void launch_atr_admm(const GemmPlan& p, const T* A, const T* Z, T* G, const T* x, T* un, T* xn, T* rn,
                     double rho, double taurho, double mu, Red red, hipStream_t st, T* Gp = nullptr,
                     unsigned* pcnt = nullptr);

// The unfused row step on the same plan's panel layout (one workgroup per panel, the lanes
// holding the rows the epilogue's lanes hold): g = S slabs of launch_atr under plan p, summed in
// slab order. Every bit it writes, the two sums included, equals launch_atr_admm's. Needs the
// plan condition of launch_atr_admm. gout (may be NULL) receives g.
template <typename T>
void launch_admm_dual_panel(const GemmPlan& p, const T* x, const T* g, int S, T* gout, T* un, T* xn,
                            T* rn, double rho, double taurho, double mu, Red red, hipStream_t st);

// ---- the dual ADMM solver's own kernels (kernels_admm.hip; gl_ADMM_dual.py:61-93) ----
// v = (Ax - rho Au) - b over ml values (the right-hand side of the K product, :63)
template <typename T>
void launch_admm_v(const T* Ax, const T* Au, const T* b, T* v, int64_t ml, double rho, hipStream_t st);
// The row step (:64-67) on g = the sum, in slab order, of S slabs of n * l values (gout, when
// non-null, receives it): w = x / rho - g, u+ = (mu w) / max(||w_i||, mu), r = u+ + g,
// x+ = x - (tau rho) r. out: [sum_i ||x+_i||, max |x+| (NaN-propagating)]
template <typename T>
void launch_admm_dual(const T* x, const T* g, int S, T* gout, T* un, T* xn, T* rn, int64_t n, int64_t l,
                      double rho, double taurho, double mu, Red red, hipStream_t st);
// The batched pass's finalize: P = S slabs of A x+ then S slabs of A u+ (ml values each), summed
// in slab order into Ax and Au; s = Au_old - Au_new (:68) where s != NULL (Au is read first);
// out: [sum (Ax - b)^2]
template <typename T>
void launch_admm_fin(const T* P, int S, const T* b, T* Ax, T* Au, T* s, int64_t ml, Red red,
                     hipStream_t st);
// gram (l x l doubles, row-major) = R^T R for R of rows x l (l <= 32), accumulated in double:
// gram_blocks(rows) workgroups each reduce a contiguous slab of rows, in row order, into a partial
// at part[block * l * l]; a second launch adds the partials in slab order (bit-reproducible)
int gram_blocks(int64_t rows);
template <typename T>
void launch_gram(const T* R, int64_t rows, int64_t l, double* part, double* gram, hipStream_t st);

// ---- the primal ADMM solver's own kernels (kernels_admm_primal.hip; gl_ADMM_primal.py:47-51, 78-84) ----
// w = (ATb - z) + rho x over nl values: the first iteration's right-hand side (later ones come
// from the row step)
template <typename T>
void launch_admm_primal_w(const T* ATb, const T* x, const T* z, T* w, int64_t nl, double rho, hipStream_t st);
// The row step on prod = the sum, in slab order, of S slabs of n * l values: y+ = prod (direct) or
// (w - prod) / rho (woodbury: prod = A^T K (A w)); p = x - (eta rho)((x - y+) - z / rho),
// x+ = (p max(||p_i|| - eta mu, 0)) / ((||p_i|| < thres) + ||p_i||), z+ = z - (tau rho)(x+ - y+),
// r = x+ - y+, s = y+ - y, w+ = (ATb - z+) + rho x+. Row-local: xn, yn, zn, wn may alias x, y, z, w.
// w is read by the Woodbury form only. out: [sum_i ||x+_i||, max |x+| (NaN-propagating)]
struct AdmmPrimalScalars {
  double rho, etarho, etamu, taurho, thres;
};
template <typename T>
void launch_admm_primal(bool woodbury, const T* prod, int S, const T* x, const T* y, const T* z, const T* w,
                        const T* ATb, T* xn, T* yn, T* zn, T* rn, T* sn, T* wn, int64_t n, int64_t l,
                        const AdmmPrimalScalars& sc, Red red, hipStream_t st);
// The finish of the pass over A. P = S slabs of A x+ (ml values each), summed in slab order into
// Ax; out: [sum (Ax - b)^2]. AATb != NULL (Woodbury): S slabs of A z+ follow, summed into Az, and
// v = (AATb - Az) + rho Ax, the right-hand side of the next K product.
template <typename T>
void launch_admm_primal_fin(const T* P, int S, const T* b, const T* AATb, T* Ax, T* Az, T* v, int64_t ml,
                            double rho, Red red, hipStream_t st);

// ---- the dual ALM solver's kernels (kernels_alm.hip, kernels_atr.hip; gl_ALM_dual.py:45-61, 119-124) ----
// One step of the inner Nesterov loop on P = Qn y (Qn = rho (I + rho A^T A)^-1, symmetric):
// w = y - t (P + J), u+ = (mu w) / max(||w_i||, mu), v+ = u + (u+ - u) / gamma,
// y+ = (1 - gamma_next) u+ + gamma_next v+. un may be u (rows are owned); yn == NULL (the last
// step): y+ is not written; yn must not be y. fp64 only.
//   launch_atr_alm:          the step in the epilogue of P = Qn^T y under the plan p of (n, n, l)
//                            (plan condition of launch_atr_admm); Gp / pcnt as launch_atr_prox
//   launch_alm_inner_panel:  on S slabs of P from launch_atr under p, the epilogue's lane-to-row
//                            layout: every bit equals launch_atr_alm's
//   launch_alm_inner:        on S slabs of P, any n and l <= 32 (kernels_elem.hip's row layout)
template <typename T>
void launch_atr_alm(const GemmPlan& p, const T* Qn, const T* y, const T* J, const T* u, T* un, T* yn,
                    double t, double mu, double gamma, double gamma_next, hipStream_t st,
                    T* Gp = nullptr, unsigned* pcnt = nullptr);
template <typename T>
void launch_alm_inner_panel(const GemmPlan& p, const T* P, int S, const T* y, const T* J, const T* u, T* un,
                            T* yn, double t, double mu, double gamma, double gamma_next, hipStream_t st);
template <typename T>
void launch_alm_inner(const T* P, int S, const T* y, const T* J, const T* u, T* un, T* yn, int64_t n,
                      int64_t l, double t, double mu, double gamma, double gamma_next, hipStream_t st);
// J = rho (h - x / rho) over nl values, h = the sum in slab order of S slabs of A^T E
template <typename T>
void launch_alm_j(const T* h, int S, const T* x, T* J, int64_t nl, double rho, hipStream_t st);
// r = u + g, x+ = x - (tau rho) r with g = the sum in slab order of S slabs of A^T z (xn may be x);
// out: [sum_i ||x+_i||, max |x+| (NaN-propagating)]
template <typename T>
void launch_alm_x(const T* x, const T* u, const T* g, int S, T* xn, T* rn, int64_t n, int64_t l,
                  double taurho, Red red, hipStream_t st);

// ---- the optimality certificate's kernels (kernels_cert.hip, kernels_atr.hip; DESIGN.md "Certificate") ----
// The row terms of the certificate on g = A^T r and the iterate x (cert_row, glx_device.h). out:
// [sum_i ||x_i||, max_i ||g_i||, max_i kkt_i, sum_i kkt_i^2, #{i : x_i != 0}], the max entries
// NaN-propagating. gout / G (may be NULL) receives g, rn (may be NULL) ||g_i|| as n doubles.
//   launch_atr_cert:    in the epilogue of G = A^T R under plan p (plan condition of
//                       launch_atr_admm); Gp / pcnt as launch_atr_prox
//   launch_cert_panel:  on S slabs of launch_atr under p, the epilogue's lane-to-row layout: every
//                       bit, the five sums included, equals launch_atr_cert's
//   launch_cert_row:    on S slabs of n * l values, any n and l <= kMaxL (kernels_elem.hip's layout)
template <typename T>
void launch_atr_cert(const GemmPlan& p, const T* A, const T* R, T* G, const T* x, double* rn, double mu,
                     Red red, hipStream_t st, T* Gp = nullptr, unsigned* pcnt = nullptr);
template <typename T>
void launch_cert_panel(const GemmPlan& p, const T* x, const T* g, int S, T* gout, double* rn, double mu,
                       Red red, hipStream_t st);
template <typename T>
void launch_cert_row(const T* x, const T* g, int S, T* gout, double* rn, int64_t n, int64_t l, double mu,
                     Red red, hipStream_t st);
// r = (the sum, in slab order, of the S slabs of A x at P) - b over ml values; S = 0: r = 0 - b.
// out: [sum r^2, sum r b] (accumulated in double)
template <typename T>
void launch_cert_fin(const T* P, int S, const T* b, T* r, int64_t ml, Red red, hipStream_t st);
// The same with one weight per row of A (w: m values of T; element idx is of row idx / l): r (may be
// NULL) = the unweighted residual, rw = fl(w r), out: [sum w r^2, sum w r b] and, with hold-out
// weights hv (may be NULL), a third value sum hv r^2. With w = 1 the two sums and rw are
// launch_cert_fin's bits.
template <typename T>
void launch_cert_fin_w(const T* P, int S, const T* b, const T* w, const T* hv, T* r, T* rw, int64_t ml, int64_t l,
                       Red red, hipStream_t st);
// The centring finalize of the problem with an intercept (DESIGN.md "Intercept"), two launches:
//   launch_cert_csum:  rh = (the sum of the S slabs at P) - b (S = 0: -b) and mean[c] =
//       sum_j w_j rh[j, c] / sigma, l doubles (w may be NULL: unit weights, the bits of all-ones).
//       part: cert_csum_part_bytes(); cnt: one zeroed word (reset by the kernel)
//   launch_cert_fin_c: rc (may be NULL, may be rh) = (T)((double)rh - mean[c]), rw = fl(w rc), out:
//       launch_cert_fin_w's sums on rc
size_t cert_csum_part_bytes();
template <typename T>
void launch_cert_csum(const T* P, int S, const T* b, const T* w, T* rh, int64_t m, int64_t l, double sigma,
                      double* part, unsigned* cnt, double* mean, hipStream_t st);
template <typename T>
void launch_cert_fin_c(const T* rh, const T* b, const T* w, const T* hv, const double* mean, T* rc, T* rw,
                       int64_t ml, int64_t l, Red red, hipStream_t st);

// ---- gap-safe screening (kernels_screen.hip; DESIGN.md "Certified solve and screening") ----
// norms[j] = ||A[:, j]||_2 (n doubles), accumulated in double over col_norm_slabs(m) fixed row slabs
// and summed in slab order; red.out = [max_j norms[j] (NaN-propagating), sum_j norms[j]^2]. part:
// col_norms_part_bytes; ccnt: col_norms_count_bytes, zero before the first launch (reset by the kernel).
int col_norm_slabs(int64_t m);
size_t col_norms_part_bytes(int64_t m, int64_t n);
size_t col_norms_count_bytes(int64_t n);
template <typename T>
void launch_col_norms(const T* A, int64_t m, int64_t n, double* norms, double* part, unsigned* ccnt, Red red,
                      hipStream_t st);
// norms[j] = sqrt(sum_i w[i] A[i, j]^2) (w: m values of T, >= 0): the same slabs, combine and stats
template <typename T>
void launch_col_norms_w(const T* A, const T* w, int64_t m, int64_t n, double* norms, double* part, unsigned* ccnt,
                        Red red, hipStream_t st);
// The centred norms of the problem with an intercept, two launches on the same slabs (w may be NULL):
// mean[j] = sum_i w[i] A[i, j] / sigma (n doubles; red_mean.out = [max_j |mean[j]|, sum_j mean[j]^2]),
// then norms[j] = sqrt(sum_i w[i] (A[i, j] - mean[j])^2) with red.out as launch_col_norms'
template <typename T>
void launch_col_norms_c(const T* A, const T* w, double sigma, int64_t m, int64_t n, double* norms, double* mean,
                        double* part, unsigned* ccnt, Red red_mean, Red red, hipStream_t st);
// keep[i] = !(s rn[i] + cn[i] rho < mu_lo) (a NaN keeps the row); list = the kept rows, ascending,
// then -1 up to cnt[1]; cnt = [kept, kept rounded up to 64]. mask (n bytes) may be NULL; list holds n
// rounded up to 64 ints; bal: screen_words_bytes(n); ticket: one zeroed word (reset by the kernel).
size_t screen_words_bytes(int64_t n);
void launch_screen(const double* rn, const double* cn, int64_t n, double s, double rho, double mu_lo,
                   unsigned char* mask, int* list, int* cnt, unsigned long long* bal, unsigned* ticket,
                   hipStream_t st);
// dst (m x wp, wp % 64 == 0) [r, j] = src (m x sw) [r, idx[j]], 0 where idx[j] is outside [0, sw)
template <typename T>
void launch_gather_cols(const T* src, int64_t m, int64_t sw, const int* idx, int64_t wp, T* dst, hipStream_t st);
// rows of l values: dst[j, :] = src[idx[j], :] (0 where idx[j] < 0) / dst[idx[j], :] = src[j, :]
// (where idx[j] >= 0; dst is cleared by the caller), j < wp
template <typename T>
void launch_gather_rows(const T* src, const int* idx, int64_t wp, int64_t l, T* dst, hipStream_t st);
template <typename T>
void launch_scatter_rows(const T* src, const int* idx, int64_t wp, int64_t l, T* dst, hipStream_t st);
// out[j] = map[idx[j]] (idx[j] itself where map == NULL), -1 where idx[j] < 0
void launch_compose_list(const int* map, const int* idx, int64_t wp, int* out, hipStream_t st);

// ---- feature groups and weights (kernels_group.hip, group.cpp; DESIGN.md "Feature groups and weights") ----
// Groups are the contiguous row ranges [ptr[g], ptr[g + 1]) of the n x l iterate, g < G; wts holds
// G doubles (rounded to T in the kernels); max_run = the largest range, which picks the lane layout
// (group_layout names it). nrows = the rows of the arrays (the slab stride is nrows * l): rows from
// ptr[G] on belong to no group.
//   launch_group_fista: the FISTA step on S slabs of launch_atr: w = y - t g, per group
//       xc = w max(||w|| - t mu w_g, 0) / ((||w|| < thres) + ||w||), then fista_row's momentum per
//       element; red.out = [sum g (xc - y), sum (xc - y)^2, sum_g w_g ||xc_[g]||, max |xc|]; rows past
//       ptr[G] of xc, vnext, ynext are written 0
//   launch_group_cert: red.out = [sum_g w_g ||x_[g]||, max_g ||g_[g]|| / w_g, max kkt, sum kkt^2,
//       nonzero groups]; gout (may be NULL) receives g, rn (may be NULL) ||g_[g]|| / w_g as G doubles
//   launch_group_cnorm: gcn[g] = sqrt(sum_{i in [g]} cn[i]^2) / w_g; red.out = [max_g gcn[g]]
//   launch_group_expand: klist = kcnt[0] kept groups, ascending (launch_screen's list and count) ->
//       rows_out (their rows, ascending, -1 up to ecnt[1]), the reduced ptr_out (kept + 1), w_out,
//       gcn_out, map_out (map composed: ids of the full problem; map NULL = identity),
//       ecnt = [rows, rows rounded up to 64]
std::string group_layout(int64_t max_len);
template <typename T>
void launch_group_fista(const T* y, const T* g, int S, const T* xk, T* xc, T* vnext, T* ynext, const int* ptr,
                        const double* wts, int64_t G, int64_t nrows, int64_t l, int64_t max_run, double t, double mu,
                        double thres, double theta, double theta_next, Red red, hipStream_t st);
template <typename T>
void launch_group_cert(const T* x, const T* g, int S, T* gout, double* rn, const int* ptr, const double* wts,
                       int64_t G, int64_t nrows, int64_t l, int64_t max_run, double mu, Red red, hipStream_t st);
void launch_group_cnorm(const double* cn, const int* ptr, const double* wts, int64_t G, int64_t max_run, double* gcn,
                        Red red, hipStream_t st);
void launch_group_expand(const int* klist, const int* kcnt, const int* ptr, const double* wts, const double* gcn,
                         const int* map, int* rows_out, int* ptr_out, double* w_out, double* gcn_out, int* map_out,
                         int* ecnt, hipStream_t st);

// ---- the sparse-group lasso (kernels_sgl.hip; DESIGN.md "Sparse-group lasso") ----
// mu Omega_tau(x) = a sum_i ||x_i|| + sum_g c_g ||x_[g]||_F with a = tau mu, c_g = (1 - tau) mu w_g.
//   launch_sgl_fista: launch_group_fista with the two-level prox; red.out[2] = Omega_tau(xc)
//   launch_sgl_cert: red.out = [Omega_tau(x), max_i ||g_i||, max kkt, sum kkt^2, nonzero groups, nonzero
//       rows]; rn (may be NULL) receives ||g_i|| as n doubles, gout (may be NULL) g
//   launch_sgl_dual_scale: two solves q = 0, 1 of s_g = sup{s: sqrt(sum_{i in g} (s p_i - a)_+^2) <= cb w_g}
//       on p_i = mul_q rho_i + add_q sqrt(*rr) (rr NULL: add_q): sg (may be NULL, 2 G) the unclamped s_g,
//       red.out[q] = max_g (-s_g)
//   launch_sgl_screen: keep[i] = 0 where s p_i + cn_i rad < a_lo or (group_test) the row's group has
//       sqrt(sum (s p_i - a_lo)_+^2) / w_g + gcn_g rad < cb_lo; gkeep (may be NULL) per group;
//       red.out = [groups that keep a row, kept rows]
//   launch_sgl_expand: keep -> rows_out (ascending, -1 up to ecnt[3]), the reduced ptr_out / w_out /
//       gcn_out / map_out over the groups that keep a row, ecnt = [groups, rows, rows, rows padded to 64]
std::string sgl_layout(int64_t l);
template <typename T>
void launch_sgl_fista(const T* y, const T* g, int S, const T* xk, T* xc, T* vnext, T* ynext, const int* ptr,
                      const double* wts, int64_t G, int64_t nrows, int64_t l, double t, double mu, double tau,
                      double thres, double theta, double theta_next, Red red, hipStream_t st);
template <typename T>
void launch_sgl_cert(const T* x, const T* g, int S, T* gout, double* rn, const int* ptr, const double* wts, int64_t G,
                     int64_t nrows, int64_t l, double mu, double tau, Red red, hipStream_t st);
void launch_sgl_dual_scale(const double* rho, const int* ptr, const double* wts, int64_t G, double a, double cb,
                           double mul0, double add0, double mul1, double add1, const double* rr, double* sg, Red red,
                           hipStream_t st);
void launch_sgl_screen(const double* rho, const double* cn, const double* gcn, const int* ptr, const double* wts,
                       int64_t G, double s, double mul, double add, const double* rr, double rad, double a_lo,
                       double cb_lo, int group_test, int* keep, int* gkeep, Red red, hipStream_t st);
void launch_sgl_expand(const int* keep, const int* ptr, const double* wts, const double* gcn, const int* map,
                       int64_t G, int* rows_out, int* ptr_out, double* w_out, double* gcn_out, int* map_out, int* ecnt,
                       hipStream_t st);

// The groups of a problem as the drivers pass them on: device ptr / wts as above, and the host's
// figures of the FULL problem (a reduced problem keeps them: they only have to bound its own).
struct GroupView {
  const int* ptr = nullptr;
  const double* wts = nullptr;
  int64_t G = 0;
  int64_t max_run = 1;
  double w_min = 1.0;
  // the sparse-group lasso (DESIGN.md "Sparse-group lasso"; 0: the group problem, nothing below is read)
  double row_ratio = 0.0;
  double* rho = nullptr;            // device, n doubles: the row norms of a certificate that returns none
  double pad_mul = 1.0, pad_add = 0.0;   // the guard's padding of the second dual solve (sgl_guard_pad)
  double* extra = nullptr;          // host, 4 doubles a certificate fills: [s, s of the padded solve, max rho, 0]
  int64_t* row_hist = nullptr;      // host, GLX_CERTIFIED_MAX_HIST: kept rows after each compaction
};
// glx_certificate's body (certificate.cpp): grp == NULL is the row certificate; with groups the
// A^T pass is launch_atr and the group terms follow (launch_group_cert), rownorm_out then takes G
// doubles ||g_[g]|| / w_g and fused is ignored. Throws Error.
// Sample weights as the drivers pass them on (DESIGN.md "Sample weights and cross-validation"):
// w = m device values of A's dtype, >= 0 (validated by the caller of the C entry); hold (may be
// NULL) = the hold-out weights of the same kind; sums = 3 device doubles the weighted finalize
// reduces into, carved behind the callee's workspace.
struct SampleView {
  const void* w = nullptr;
  const void* hold = nullptr;
  double* sums = nullptr;
};
// SampleView::sums behind `head` bytes of a callee's workspace: its offset and the bytes of both
inline size_t sample_off(size_t head) { return (head + 255) & ~size_t(255); }
inline size_t sample_bytes(size_t head) { return sample_off(head) + 256; }
// sw (NULL: every call and byte above): the certificate of 1/2 sum_j w_j ||(A x - b)_j||^2 + mu Omega(x):
// out[0] = sum w r^2, out[1] = sum w r b, the A^T pass runs on w r; *holdout_sum (where sw->hold)
// = sum_j hold_j ||(A x - b)_j||^2 from the same launch.
// The unpenalised intercept as the drivers pass it on (DESIGN.md "Intercept"): sigma = sum_j w_j (m
// without sample weights), mean_host = l host doubles that receive the weighted column means r-bar of
// r^ = fl(A x) - b at every certificate (the intercept is c = -r-bar), and the device pieces of the
// centring finalize, carved behind the callee's workspace (intercept_carve).
struct InterceptView {
  double sigma = 0.0;
  double* mean_host = nullptr;
  void* rhat = nullptr;       // m * l values of A's dtype
  double* mean = nullptr;     // l doubles
  double* part = nullptr;     // cert_csum_part_bytes()
  unsigned* cnt = nullptr;    // 256 bytes, zeroed by the launching driver
};
// [head | rhat | mean | part | cnt] (base == NULL: the size only); returns the bytes of all of it
size_t intercept_carve(size_t head, int es, int64_t m, int64_t l, void* base, InterceptView* out);
// the checks every intercept entry makes: weight_sum finite and > 0, intercept_out not NULL
void check_intercept(double weight_sum, const double* intercept_out);
// ic (NULL: every call and byte above): the certificate of min_c 1/2 sum_j w_j ||(A x + 1 c^T - b)_j||^2
// + mu Omega(x): the finalize is the two centring launches, out[0], out[1] are the sums on the centred
// residual r_c, the A^T pass runs on w r_c (sw == NULL: on r_c), *holdout_sum is taken on r_c.
void certificate_run(int dtype, int64_t m, int64_t n, int64_t l, const void* A, const void* X, const void* b,
                     double mu, int fused, void* G_out, double* rownorm_out, double* out, void* ws, size_t wsb,
                     void* stream, const GroupView* grp, const SampleView* sw = nullptr,
                     double* holdout_sum = nullptr, const InterceptView* ic = nullptr);
// The certified solve (screen.cpp), rows (grp == NULL) or groups: one loop, glx_certified_solve's
// arguments and checks. With groups the step is launch_atr + launch_group_fista, the screen runs on
// the G "rows" ||g_[g]|| / w_g against gcn (launch_group_cnorm, computed here) and
// launch_group_expand turns its list into rows; info->kept and kept_hist then count groups.
// kept_groups_dev (may be NULL): as kept_rows_dev, for groups; *listed_groups = the entries written.
// With sample weights (sw; its `sums` is ignored: the solve carves its own) both residual finalizes,
// ||b~||, the column figures and every certificate are the weighted problem's; col_norms_dev then
// holds the weighted norms. The final full-problem certificate takes sw->hold: *holdout_sum.
// With an intercept (ic: its sigma and mean_host; the device pieces are carved here, `intercept` sizes
// them) the finalize of an iteration and the null product's are the two centring launches, the column
// figures are the centred ones (col_stats then holds four values: launch_col_norms_c's two pairs),
// every certificate centres and the screen runs under screen_guard_ic; ic->mean_host holds the means
// of the final certificate on return.
size_t certified_bytes(int dtype, int64_t m, int64_t n, int64_t l, bool screen, int64_t G, bool weighted = false,
                       bool intercept = false, bool sgl = false);
std::string certified_describe(int dtype, int64_t m, int64_t n, int64_t l, bool screen, int64_t max_run,
                               bool sgl = false);
void certified_run(const glx_problem* prob, double t, double tol, int64_t maxit, int screen, int check_every,
                   const double* col_norms_dev, const double* col_stats, int32_t* kept_rows_dev, void* ws,
                   size_t wsb, glx_certified_info* info, void* stream, const GroupView* grp,
                   int32_t* kept_groups_dev, int64_t* listed_groups, const SampleView* sw = nullptr,
                   double* holdout_sum = nullptr, const InterceptView* ic = nullptr);
// The rounding guards, host only (screen.cpp / group.cpp); out = [s_safe, gap+, rho+]. weighted: the
// record, the column figures and bn are the sample-weighted problem's, and the roundings of w r and
// w r^2 are counted (DESIGN.md "Sample weights and cross-validation", "The guard").
double gamma_k(double k, double u);
void group_screen_guard(const double* rec, double mu, int dtype, int64_t m, int64_t n, int64_t l, int64_t max_run,
                        double w_min, double gcol_max, double csq, double bn, double* out, bool weighted = false);
// The guards of the problem with an intercept (DESIGN.md "Intercept", "The guard"); out = [s_safe, gap+,
// rho+, slack]: a row is screened when s rn + cn rho+ < mu - slack with cn the CENTRED norm. rec: the
// centred record; cstats = [max centred norm, sum centred norm^2, max |column mean|, sum column mean^2];
// bn = sqrt(sum w b^2) (uncentred); sigma = sum w; mean_sq = sum_c r-bar_c^2 of the record's certificate.
void screen_guard_ic(const double* rec, double mu, int dtype, int64_t m, int64_t n, int64_t l, const double* cstats,
                     double bn, double sigma, double mean_sq, double* out);
void group_screen_guard_ic(const double* rec, double mu, int dtype, int64_t m, int64_t n, int64_t l, int64_t max_run,
                           double w_min, double gcol_max, const double* cstats, double bn, double sigma,
                           double mean_sq, double* out);
// The sparse-group guard (group.cpp; DESIGN.md "Sparse-group lasso", "The guard"). sgl_guard_pad: pad =
// [mul, add coefficient]: mul rho^_i + add ||r^|| bounds the exact ||a_i^T r^|| for every row (cmax = the
// largest column norm). sgl_screen_guard: rec = the sparse-group record, s_pad = min_g s_g of the padded
// solve; out = [mul, add ||r^||, s_safe, gap+, rho+].
void sgl_guard_pad(int dtype, int64_t m, int64_t l, int64_t max_run, double cmax, bool weighted, double* pad);
void sgl_screen_guard(const double* rec, double s_pad, double mu, double tau, int dtype, int64_t m, int64_t n,
                      int64_t l, int64_t max_run, double w_min, double cmax, double csq, double bn, double* out,
                      bool weighted);
// the checks every weighted C entry makes of its two vectors: 16-byte aligned, hold only with w
void check_sample(const void* sample_w, const void* holdout_w);

// ---- split-candidate A e from a transposed copy of A (kernels_gather.hip) ----
// gather_ok: the shape supports it (l in {16, 32}, n < 65536); gather_split: K splits of the
// flagged-row list for m output rows (slabs P[S][m][l]).
bool gather_ok(int64_t n, int64_t l);
// round 5: the MFMA row form (k_at_rows): the shapes it takes, the solver's default (GLX_GATHER=valu:
// the column-list gather, ONE slab), and its K splits for this shape (1 where it does not apply)
bool gather_rows_ok(int64_t m, int64_t n);
int gather_form();   // GLX_GATHER: 0 bitmaps, 1 MFMA rows, 2 k_e_lists + k_at_gather, -1 unset
int gather_split(int64_t m, int64_t n);
// zf: the per-row column masks of e and, behind them, the per-column row bitmaps (glx_device.h)
size_t zf_bytes(int64_t n);
// A e from the column bitmaps behind zf (ONE slab at P; the column list lengths to gather_counts)
template <typename T>
void launch_at_gather_bm(const T* At, const T* E, unsigned* zf, int64_t m, int64_t n, int64_t l, T* P,
                         void* lists_ws, hipStream_t st, const int* skip = nullptr);
// the column bitmaps behind zf from its row masks (where no trial kernel wrote them)
void launch_zf_bitmaps(unsigned* zf, int64_t n, int64_t l, hipStream_t st);
// P[s][r][c] = sum over the flagged rows k (zf[k] != 0) of K range s, ascending:
// At[k][r] E[k][c], s < gather_split(m, n); counts[s] (gather_counts) = the flagged rows of range s
template <typename T>
void launch_at_rows(const T* At, const T* E, const unsigned* zf, int64_t m, int64_t n, int64_t l,
                    T* P, void* lists_ws, hipStream_t st, const int* skip = nullptr);
// At (n x m) = A^T
template <typename T>
void launch_transpose(const T* A, T* At, int64_t m, int64_t n, hipStream_t st);
// launch_e_lists: per column c the ascending k with bit c of zm[k] set (zm: the per-row column
// masks of e the trial kernels write), into lists_ws (gather_lists_bytes(n));
// launch_at_gather: P[r][c] = sum over column c's list of At[k][r] E[k][c] (one slab)
size_t gather_lists_bytes(int64_t n);
// the l per-column list lengths inside lists_ws (device)
const unsigned* gather_counts(const void* lists_ws, int64_t n);
void launch_e_lists(const unsigned* zm, int64_t n, int64_t l, void* lists_ws, hipStream_t st,
                    const int* skip = nullptr);
template <typename T>
void launch_at_gather(const T* At, const T* E, int64_t m, int64_t n, int64_t l, T* P, void* lists_ws,
                      hipStream_t st, const int* skip = nullptr);

// ---- fused residual + gradient in one pass over A (kernels_fused.hip) ----
// Sraw = A X (m x 32) and Gs[RG][n][32] with G = A^T (A X - B) = sum of the RG slabs in order.
// resgrad_shape_ok: fp64, l = 32, n % 512 == 0, m % (16 RG) == 0; resgrad_device_ok: all 256
// workgroups can be resident (>= 256 CUs). ws: resgrad_ws_bytes; its counters must be zeroed
// (resgrad_reset) before launch_count 1, and launch_count must grow by one per launch.
bool resgrad_shape_ok(int esize, int64_t m, int64_t n, int64_t l);
bool resgrad_device_ok();
int resgrad_groups(int64_t n);
size_t resgrad_ws_bytes(int64_t m, int64_t n);
void resgrad_reset(void* ws, int64_t m, int64_t n, hipStream_t st);
// returns false (nothing launched) when the runtime refuses the cooperative launch; *err != 0
// after the launch: a hand-off wait timed out or the XCD grouping failed, R / G are invalid
// ---- the trial's batch + the next gradient in one pass, l = 16 (kernels_rg2.hip, round 4) ----
// P0 = A X0, P1 = A X1 (one m x 16 slab each), Gs[RG][n][16] with G = A^T (P1 - B) = the sum of the
// RG slabs in order. resgrad2_shape_ok: fp64, l = 16, n = 256 P (P a power of two in 2..128),
// m % (16 kRAB RG) == 0 (kRAB = 4 A-tiles per hand-off: 64 * 256 / P), m / RG >= 32 (RG = 256 / P). Plain launch of 256 workgroups that wait for each
// other with bounded spins (*err = 1 on a timeout: outputs invalid); resgrad2_device_ok checks
// that all of them can be resident. ws: resgrad2_ws_bytes, zeroed (resgrad2_reset) before
// launch_count 1; launch_count grows by one per launch on the same workspace.
bool resgrad2_shape_ok(int esize, int64_t m, int64_t n, int64_t l);
bool resgrad2_device_ok();
int resgrad2_groups(int64_t n);
size_t resgrad2_ws_bytes(int64_t n);
void resgrad2_reset(void* ws, int64_t n, hipStream_t st);
void launch_resgrad2(const double* A, const double* X0, const double* X1, const double* B,
                     double* P0, double* P1, double* Gs, void* ws, unsigned launch_count, int64_t m,
                     int64_t n, int* err, hipStream_t st);
bool launch_resgrad(const double* A, const double* X, const double* B, double* Sraw, double* Gs,
                    void* ws, unsigned launch_count, int64_t m, int64_t n, int* err, hipStream_t st);

// ---- row / elementwise kernels (kernels_elem.hip) ----
// Gradient inputs `g` with an `S` argument are S split-K slabs of n*l values summed in slab
// order on the fly (S = 1: an already-summed array).
//
// R[src] = sum_s P[src][s] - B for src < nsrc (if gate == NULL or *gate == epoch);
// out[src] = sum R[src]^2 (out[0..2]), out[3] = count(|cx| > 1e-6 * (*cmax)) when cx != NULL;
// fh != NULL: *fh = 0.5 out[0] + fh_mu * (*fh_rn) (device-side objective history).
// gate_mode: when gated off, 0 = do nothing, 1 = recompute out[0] from R[0] (nsrc = 1).
// chain (nsrc = 2, split-candidate mode): source 0 is a correction on top of source 1,
// R[0] = (sum_s P[1][s] - B) + sum_s P[0][s]; R[0] may then be NULL (only its sum is kept).
// With chain, source 0 has S0 slabs (0: S) at P and source 1 has S slabs at P + S0 * ml.
template <typename T>
void launch_finalize_residual(const T* P, int S, const T* B, int nsrc, T* const* R, int64_t ml,
                              const int* gate, int epoch, int gate_mode, const T* cx, int64_t cn,
                              const double* cmax, double* fh, double fh_mu, const double* fh_rn,
                              Red red, hipStream_t st, const double* snap_src = nullptr,
                              double* snap_dst = nullptr, int nsnap = 0, int chain = 0, int S0 = 0,
                              Ctl ctl = Ctl{}, const double* cmax_parts = nullptr, int cmax_np = 0,
                              int cmax_nv = 6);
// (cmax_parts: *cmax is still pending as the max column (index 3) of cmax_np trial partials,
// Red::parts_only layout of cmax_nv values, reduced by every workgroup for itself)
// state[0..3] = s0..s3, *abort = 0 (one thread; the seed of a device-controlled batch)
// the decision of a device-controlled ProxGD iteration with a communicator (one thread): out =
// the all-reduced residual sums (a gradient set's tail); no-op once *c.abort != 0; the record
// goes to c.rec and to the host ring (host[0..11), then *host_seq = seq)
void launch_ctl_decide(const Ctl& c, const double* out, double* host, unsigned* host_seq,
                       unsigned seq, hipStream_t st);
void launch_ctl_seed(double* state, int* abort, double s0, double s1, double s2, double s3,
                     hipStream_t st);
template <typename T>
void launch_sum_partials(const T* Gp, int S, T* G, int64_t nl, hipStream_t st);
// ProxGD trial: p = prox(x - t g, t), G_t = (x - p)/t, z = x - t G_t, pthr = p thresholded.
// out: [sum g*G_t, sum G_t^2, sum_i ||p_i||, max |p|, #{entries of p changed by the threshold},
//       #{rows of p changed by the threshold}]
// zf != NULL (split-candidate mode): z receives e = p - p_thr instead and zf[i] = the column mask
// of row i of e (bit c = e[i][c] != 0).
template <typename T>
void launch_prox_pgd(const T* x, const T* g, int S, T* gout, T* p, T* pthr, T* z, int64_t n,
                     int64_t l, double t, double mu, double thres, Red red, hipStream_t st,
                     Pub pub = Pub{}, unsigned* zf = nullptr);
// The row-sharded trial's all-gathered sums: blk holds nranks chunks of `chunk` doubles, from
// kShardPartOff the workgroup partials (Red::parts_only) of the trial (launch_prox_pgd's out, 6
// per workgroup, nbp workgroups) and then of its finalize (launch_finalize_residual's out, 4 per
// workgroup, nbf workgroups). Combined in a
// fixed order (sums; trial slot 3: max, NaN-propagating), identical on every rank: mask & 1 ->
// tr[0, 6), mask & 2 -> rt[0, 4); with pub.host the scalar packet follows with these values.
constexpr int kShardPartOff = 16;
struct ShardPub {
  const double* blk = nullptr;
  int nranks = 1, chunk = 0, nbp = 0, nbf = 0, mask = 0;
  int tv = 6;                   // values per trial partial (ProxGD 6, FProxGD 4; the max is value 3)
  double* tr = nullptr;
  double* rt = nullptr;
  int tr_off = 0, rt_off = 0;   // their packet slots
  Pub pub{};
};
void launch_shard_combine(const ShardPub& sp, hipStream_t st);
// workgroups of launch_prox_pgd over n rows of l columns (without a packet)
int prox_blocks(int64_t n, int64_t l);
// workgroups of launch_finalize_residual for these slabs and count length
int finalize_blocks(int64_t ml, int S, int S0, int64_t cn);
int finalize_fista_blocks(int64_t ml, int S, int S0, int64_t cn);
// Row-sharded schedule (round 5, solver.cpp iter_proxgd_shard): the replicated half of a ProxGD
// trial, from the all-gathered p (n x l): pthr = p with |p| < thres zeroed; z = e = p - pthr
// (emode) or z = xt - t (xt - p) / t (launch_prox_pgd's dense z, xt = the thresholded iterate);
// zf != NULL: zf[i] = the column mask of row i of e and the column bitmaps behind the masks —
// the same bits launch_prox_pgd writes.
// z == NULL: not written. sp.blk != NULL: one more workgroup runs launch_shard_combine's work
// beside the rows.
template <typename T>
void launch_trial_split(const T* p, const T* xt, T* pthr, T* z, unsigned* zf, int64_t n, int64_t l,
                        double t, double thres, bool emode, const ShardPub& sp, hipStream_t st);
// Row-sharded FProxGD (round 6, solver.cpp iter_fista_shard): the replicated half of a FISTA
// trial from the all-gathered xc (n x l): v_next = thr(xk) + (xc - thr(xk)) / theta and
// y_next = (1 - theta') thr(xc) + theta' v_next with k_fista_trial's arithmetic (fista_row), so
// the bits equal the ones that kernel would have written for the whole of xc. sp.blk != NULL: one
// more workgroup combines the gathered sums (launch_shard_combine's work) beside the elements.
template <typename T>
void launch_fista_split(const T* xc, const T* xk, T* vnext, T* ynext, int64_t nl, double thres,
                        double theta, double theta_next, const ShardPub& sp, hipStream_t st);
// Round 6: the ProxGD half above (emode, e = p, no z) fused into the split-candidate dense pass
// A p_thr (kernels_gemm.hip k_ax_lds_drv, the 8-wave shard tile 51328 at l = 32, f64): the pass
// reads the gathered p and thresholds it on the way into LDS; nd extra workgroups write p_thr,
// ggx * l more compute the trial's A e (k_at_gather_bm's work and bits) into the slab Pe beside
// the MFMA work — column c's row list from the bitmap words every rank's k_prox_pgd wrote for its
// srows rows into its sums chunk (blk + rank * bstride + moff: srows row masks, then the column
// bitmaps; all-gathered with the sums, so ready before the pass starts; bstride 0 in the one-GPU
// timing model: rank 0's words for every rank); the publisher workgroup combines sp's sums and
// publishes the packet (pub, required). False: the plan or the shape does not take it.
struct AxDerive {
  void* pthr = nullptr;
  double thres = 0.0;
  ShardPub sp{};
  int ggx = 0;                   // gather row blocks (kDrvGatRows rows each)
  int nd = 0, thr0 = 0, gat0 = 0;   // set by the launcher: p_thr workgroups, first p_thr / A e one
  const void* At = nullptr;
  const void* E = nullptr;       // e where its masks are set (the gathered p)
  void* Pe = nullptr;
  const double* blk = nullptr;
  int64_t bstride = 0, moff = 0, srows = 0;
};
// rows of A per gather workgroup of the fused dense pass (AxDerive::ggx = ceil(m / this)), and
// its p_thr workgroups
constexpr int kDrvGatRows = 512;
constexpr int kDrvThrBlocks = 64;
template <typename T>
bool launch_ax_derive(const GemmPlan& p, const T* A, const T* Xp, T* P, hipStream_t st, Pub pub,
                      const AxDerive& d);

// FISTA (prox = true) / FGD (prox = false: identity) trial fused with the next combine:
// xc = prox(y - t g, t); vnext = thr(xk) + (xc - thr(xk))/theta;
// ynext = (1 - theta_next) thr(xc) + theta_next vnext.
// out: prox: [sum g*(xc-y), sum (xc-y)^2, sum ||xc_i||, max |xc|]
//      FGD : [sum g*(xc-y), sum (xc-y)^2, sum (sqrt(||xc_i||^2+d^2)-d), sum ||xc_i||, max |xc|]
// ec != NULL (split-candidate mode): ec = xc - thr(xc) and zf[i] = the column mask of row i of ec.
template <typename T>
void launch_fista_trial(bool prox, const T* y, const T* g, int S, T* gout, const T* xk, T* xc,
                        T* vnext, T* ynext, int64_t n, int64_t l, double t, double mu, double thres,
                        double theta, double theta_next, double delta, Red red, hipStream_t st,
                        Pub pub = Pub{}, T* ec = nullptr, unsigned* zf = nullptr);
// split-candidate FISTA batch finalize (k_finalize_fista): P = S slabs of A xc, Pe = S0 slabs of
// A e_c, sxo = A thr(xk); Ry = A y_next - b with y_next = a1 thr(xc) + b1 (thr(xk) + (xc -
// thr(xk)) / theta), sxo_out = A thr(xc). out: [sum (A xc - b)^2, sum Ry^2,
// sum counts[0..nl) (nnz of e_c, gather_counts), count as above].
template <typename T>
void launch_finalize_fista(const T* P, int S, const T* Pe, int S0, const T* B, T* Ry, const T* sxo,
                           T* sxo_out, int64_t ml, double a1, double b1, double theta, const T* cx,
                           int64_t cn, const double* cmax, const unsigned* counts, int nl, Red red,
                           hipStream_t st, Ctl ctl = Ctl{}, const double* cmax_parts = nullptr,
                           int cmax_np = 0, int cmax_nv = 4);
// plain prox of W (glx_prox): out: [sum ||x_i||, max |x|]
template <typename T>
void launch_prox_plain(const T* w, T* x, int64_t n, int64_t l, double t, double mu, double thres,
                       Red red, hipStream_t st);
// out[0] = count(|x| > 1e-6 * (*maxv))
template <typename T>
void launch_count_above(const T* x, int64_t nl, const double* maxv, Red red, hipStream_t st);
// xo = x with |x| < thres zeroed (xo may alias x); *flag = epoch if any value changed
template <typename T>
void launch_threshold(const T* x, T* xo, int64_t nl, double thres, int* flag, int epoch, hipStream_t st);
// xk[|xk| < thres] = 0 in place; y = a*xk + b*vk
template <typename T>
void launch_thr_axpby(T* xk, const T* vk, T* y, int64_t nl, double thres, double a, double b,
                      hipStream_t st);
// SGD (mode 0) / GD (mode 1) step from the thresholded iterate xt: x = xt - alpha (g + mu xt/d),
// xt = thr(x). out: [sum ||x_new_i||]
template <typename T>
void launch_descent(T* x, T* xt, const T* g, int S, int64_t n, int64_t l, double alpha, double mu,
                    double thres, double delta, int mode, Red red, hipStream_t st);
// out: [sum ||x_i||, max |x|]
template <typename T>
void launch_rownorm_max(const T* x, int64_t n, int64_t l, Red red, hipStream_t st);
// FGD: g = sum(gp slabs) + mu * y / sqrt(||y_i||^2 + delta^2);
// out: [sum (sqrt(||y_i||^2+delta^2) - delta)]
template <typename T>
void launch_fgd_grad(const T* y, const T* gp, int S, T* g, int64_t n, int64_t l, double mu,
                     double delta, Red red, hipStream_t st);
// fh[idx] = 0.5 * s[i_sumsq] + mu * s[i_reg]
void launch_record_f(const double* s, int i_sumsq, int i_reg, double mu, double* fh, int64_t idx,
                     hipStream_t st);
// l = 1 descent pass in one sweep of A (kernels_gemv.hip): Gp[blocks][n] = per-workgroup
// A^T (A xt - b) slabs, red.out[0..1] = sum (A x - b)^2, sum (A xt - b)^2, fh[0] (if non-null)
// = 0.5 out[0] + fh_mu * rn[0]. gemv_fused_blocks() = workgroups to launch, 0 = not applicable.
// nt: 0 / 1 = A read with the default / the non-temporal policy, -1 = GLX_GEMV_NT, else by size.
int gemv_fused_blocks(int esize, int64_t m, int64_t n, int64_t l);
template <typename T>
void launch_gemv_fused(int blocks, const T* A, const T* x, const T* xt, const T* b, T* Gp, int64_t m,
                       int64_t n, double* fh, double fh_mu, const double* rn, Red red,
                       hipStream_t st, int nt = -1);
// G[j] = sum_{s<S} Gp[s][j] (slab order, deterministic)
template <typename T>
void launch_sum_cols(const T* Gp, int S, T* G, int64_t n, hipStream_t st);
// host[0..ns) = s[0..ns) except host[off2..off2+n2) = s2[0..n2) when s2 != NULL, then
// *host_seq = seq (system-scope release); host memory is mapped
// the packet of `pub` with its deferred reductions first (pub.host == NULL: the reductions only)
void launch_publish_pub(const Pub& pub, hipStream_t st);
void launch_publish(const double* s, int ns, double* host, unsigned* host_seq, unsigned seq,
                    hipStream_t st, const double* s2 = nullptr, int off2 = 0, int n2 = 0);

}  // namespace glx
