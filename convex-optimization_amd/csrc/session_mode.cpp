// session_mode.cpp — what a session launches (host only): the plan, the split-candidate form, the
// speculative and device-controlled paths, row sharding. Resolved once per session from the
// problem, the options and the environment (SessionKnobs); Session<T> (solver.cpp) consumes it.
#include <algorithm>

#include "glx_comm.h"
#include "glx_internal.h"

namespace glx {
namespace {

constexpr int kDcWindow = 8;     // device-controlled line search: iterations in flight (GLX_DC_BATCH)
constexpr int kKeepMiB = 192;    // Infinity-Cache hand-off between the non-temporal passes
// round 6: flagged rows from which ProxGD's split-candidate A e takes the fused form (GLX_AE_HYB_ROWS)
constexpr double kHybRows = 2000.0;
// the row form reads one At row per flagged row: its cost passes the dense second source's
// (~0.7 of a pass at NS) near 0.65 n flagged rows
constexpr double kRowsBudget = 0.6;

// what both decisions below ask of the problem and the options
struct Ask {
  const glx_problem& P;
  const glx_opts& O;
  const SessionKnobs& k;
  bool trial_step() const { return O.step_type == GLX_STEP_LINE_SEARCH || O.step_type == GLX_STEP_FIXED; }
  bool line_search() const { return O.step_type == GLX_STEP_LINE_SEARCH && O.ls_maxit > 0; }
  double a_bytes_f64() const { return (double)P.m * (double)P.n * 8.0; }
};

// device-controlled batches' window: opts.dc_window (> 0: that window, < 0: off), else
// GLX_DC_BATCH, else the measured default (0 = the host decides every iteration): kDcWindow for
// FProxGD with a communicator, off elsewhere. Same box, 200-step windows, host control against
// window 8 (profiles/r3_dc/): ProxGD NS 2374-2382 vs 2344-2354 it/s, C2 9003-9010 vs 8894-8910,
// the comm-path shards 6922-11023 vs 6735-10612 (its speculative A@X already hides the host's
// turn); FProxGD NS 2454-2478 vs 2456-2465 (whole solve 2058-2060 vs 2036-2038), C3 3702 vs
// 3687-3703, C5's shard 1227-1231 vs 1230-1234, the 1024-row comm shard 9802-9829 vs 10517-10587
// (+7.5 %: the host path leaves the GPU idle while it decides behind the short speculative trial).
// Round 5: also kDcWindow for ProxGD on the unfused speculative form (unfused: session_mode's
// dc_unfused) when A is at most kDcSmallBytes — launch-bound shapes, where the host's turn per
// iteration is a large share: C1 (512, 1024, 2) 200-step windows 24 250 / 24 253 it/s with host
// control against 25 477 / 25 591 with window 8 (and 22 079 / 21 752 on the rounds-1-4 form;
// profiles/r5_unfused/).
constexpr double kDcSmallBytes = 64.0 * 1024 * 1024;
int dc_window_request(const Ask& a, bool unfused) {
  int w = (a.P.method == GLX_FPROXGD && a.P.comm != nullptr) ? kDcWindow : 0;
  if (unfused && a.a_bytes_f64() <= kDcSmallBytes) w = kDcWindow;
  if (a.O.dc_window != 0) w = a.O.dc_window;
  else w = a.k.dc_batch.num(w);
  return std::max(0, std::min(w, kCtlMaxBatch / 2));
}

// Row sharding, one decision for both methods: the ranks it runs on, else 0.
// Round 6: row-sharded FProxGD (iter_fista_shard) — the gradient
// reduce-scattered, k_fista_trial on this rank's n / G rows, xc's rows all-gathered and v_next,
// y_next re-derived from it on every rank (k_fista_split). Returns G where it applies, else 0.
// opts.shard_rows (GLX_SHARD_ROWS): 1 on (needs n % G == 0), 2 off, 0 auto: on where this rank's
// A is below kFistaShardMaxBytes and no device-control window is asked for. Host control only:
// the device-controlled FISTA batch (fista_dc_run) decides from all-reduced gradient tails; the
// sharded form would need its decision behind the all-gather, one more collective per queued
// iteration, so big shards (C5: 2 GiB per rank, where the replicated row work is ~2 % of an
// iteration) keep the all-reduce schedule with device control.
// Row-sharded ProxGD (round 5, iter_proxgd_shard): with a communicator of G > 1 ranks the
// gradient is reduce-scattered, the trial runs on this rank's n / G rows and p's rows are
// all-gathered (opts.shard_rows: 0 auto = on where n % G == 0, 1 on, 2 off; GLX_SHARD_ROWS,
// same codes, overrides). Host control only (a device-control window keeps the all-reduce
// schedule). opts.shard_model = G at world size 1 (bench.py --shard-model, with --force-comm):
// the per-rank timing model of G ranks — the trial on n / G rows, every line-search test
// accepted — whose iterates are NOT a solve (glx_solve refuses it; ADVICE round 5: no
// environment variable turns it on inside the library).
// dc_window: the window that takes effect (ProxGD; FProxGD decides before its window does).
constexpr double kFistaShardMaxBytes = 768.0 * 1024 * 1024;
int shard_ranks(const Ask& a, int dc_window) {
  const bool fista = a.P.method == GLX_FPROXGD;
  if (a.P.comm == nullptr || (a.P.method != GLX_PROXGD && !fista)) return 0;
  if (fista ? !a.trial_step() : dc_window != 0) return 0;
  const int want = a.k.shard_rows.num(a.O.shard_rows);
  if (a.k.shard_rows.set() && (want < 0 || want > 2))
    throw Error{GLX_E_INVALID, "GLX_SHARD_ROWS must be 0 (auto), 1 (on) or 2 (off)"};
  const int cranks = comm_size(static_cast<const glx_comm*>(a.P.comm));
  const int vr = cranks == 1 ? std::max(1, a.O.shard_model) : cranks;
  if (want == 2 || vr <= 1) return 0;
  const bool fits = vr <= kMaxShardRanks && a.P.n % vr == 0;
  if (want == 1 && !fits)
    throw Error{GLX_E_INVALID, std::string(fista ? "row-sharded FProxGD" : "row-sharded ProxGD") +
                                   " needs n % ranks == 0 and at most 64 ranks "
                                   "(opts.shard_rows = 0 / 2: the all-reduce schedule)"};
  if (!fits) return 0;   // auto: the all-reduce schedule where it does not fit
  if (fista && want == 0 && (a.a_bytes_f64() >= kFistaShardMaxBytes || a.O.dc_window > 0)) return 0;
  return vr;
}

// ------------------------------------------------------------------------------------------
// The solver's plan: the shape's GEMM plan, plus one method-level choice. fp32 ProxGD/FProxGD
// on one GPU take the 4-wave panel AᵀR with 2 K splits (code 1008) instead of the 4-panel
// tile (1114), so that the line-search trial fuses into it (atr_split_combine): the AᵀR pass
// is ≈13 µs slower but the trial launch and its boundary go. Same box: C3 (8192,16384,32)
// FProxGD 3669–3691 → 3743–3749 it/s, ProxGD 3654–3657 → 3744–3752, FProxGD at (4096,8192,16)
// 11 362–11 366 → 13 200–13 215 (profiles/r1_tuning/small_kernels/atr_f32_fused.log).
// Round 3: with the PF 8 ring (1008) instead of PF 4 the C3 pass reads 5.0 instead of 4.7 TB/s
// (A^T R 106.6–107.1 vs 113–114.5 us), FProxGD 3627–3680 → 3725–3763 it/s over 200 steps;
// S = 1 / 4 and the default load policy measured level or slower (profiles/r3_c3atr/sweep.txt).
// Split-candidate ProxGD (the fast objective mode, see iter_proxgd): 0 = off (exact mode, other
// methods, shapes the gather does not cover, or GLX_SPLIT_CAND=0 / glx_opts.split_cand = 0: the
// dense [z | p_thr] batch of round 1); 1 = A e from the transposed copy of A (kernels_gather.hip;
// costs an extra m x n copy of A in the workspace, glx_session_workspace_bytes).
// ProxGD: fp64 only. In fp32 its regrouped sum (A p_thr - b) + A e IS the recorded objective
// and moves f by ~1e-6 relative on short unconverged runs (measured 1.5e-6 on mid_384x640x16
// against the 1e-6 fp32 bar); no fp32 ProxGD configuration is on the benchmark path.
// FProxGD in fp32 (C3): the objective is A xc computed directly; only A y_next is regrouped.
// Round 4 kept it opt-in because one whole C3 solve ended 3.4e-5 from the reference's fp32 run
// against 3.4e-7 for the dense batch. Round 5 measured the band (scripts/c3_band.py,
// profiles/r5_d/c3_band.jsonl): eleven summation orders of the two forms (K splits, tiles, A e
// forms) end 3.4e-7 .. 8.7e-5 (dense) and 1.6e-5 .. 8.9e-5 (split) from the reference's fp32
// objective, all 7.0e-3 .. 7.1e-3 from its fp64 one (the reference's own fp32 run: 7.0e-3).
// Round 6: the dense batch is the fp32 default again — its default order ends
// 3.4e-7 from the reference's fp32 run, inside the 1e-6 fp32 bar, the split form's 1.6e-5 does
// not, and whole solves run level (3897 it/s both: late in a solve e_c fills and the budget runs
// dense batches; only 200-step windows gain, +17 %). GLX_SPLIT_F32=1: the split form (opt-in).
// (The size gate counts elements as fp64.)
// FProxGD with line search takes the gather form too (iter_fista: A y_next by linearity from
// A xc, A e_c and the kept A thr(x_k)); GLX_SPLIT_FISTA=0 keeps its dense [xc | y_next] batch.
// Only for A of at least kSplitMinBytes (this rank's rows): the column lists and the gather
// carry a fixed ~70 + 50 us that a short dense pass cannot hide. Measured against the dense
// batch (profiles/r2_splitgate/): NS (1 GiB) 2295 vs 2080 it/s, (4096,16384,32) 3894 vs 3832,
// but C2 (4096,8192,16) 7329 vs 8948 and the comm-path shards of 4096 / 2048 / 1024 rows
// 3543 / 6756 / 9748 vs 3623 / 6884 / 11162. GLX_SPLIT_CAND=1 forces it at any size (tests).
// Round 5 (the bitmap gather: no lists kernel, ~5 us fixed): ProxGD at l = 32 takes it from
// 64 MiB of A on this rank. Measured against the dense batch (profiles/r5_e/, profiles/r5_f/;
// 200-step windows / whole solves): (4096, 16384, 32) 4844 / 4894 vs 3987 / 4069 it/s; the
// communicator-path shards of 1024 / 2048 / 4096 rows 12114 / 8016 / 4759 vs 11122 / 6931 / 3915
// (whole solves at 1024 / 4096 rows 12082 / 4848 vs 11226 / 4015). C2 (l = 16, A in the Infinity
// Cache, where At would evict it) stays dense: 8411 / 8205 vs 9127 / 9151; FProxGD's shards too
// (whole solves 10480 / 3943 vs 10847 / 4000: e_c fills late in a solve).
constexpr double kSplitMinBytesL32 = 64.0 * 1024 * 1024;
constexpr double kSplitMinBytes = 768.0 * 1024 * 1024;
int split_mode(const Ask& a, bool fista_sharded) {
  const glx_problem& P = a.P;
  if (a.O.exact_objective != 0) return 0;
  if (P.method != GLX_PROXGD && P.method != GLX_FPROXGD) return 0;
  // fp32: FProxGD only, opt-in (GLX_SPLIT_F32=1, above)
  if (P.dtype != GLX_F64 && (P.method != GLX_FPROXGD || !a.k.split_f32.is("1"))) return 0;
  if (a.O.split_cand == 2) return 0;
  const bool env = a.O.split_cand == 0;   // GLX_SPLIT_CAND counts only where the option is auto
  if (env && a.k.split_cand.is("0")) return 0;
  const bool force = a.O.split_cand == 1 || (env && a.k.split_cand.is("1"));
  const double gate = (P.method == GLX_PROXGD && P.l == 32) ? kSplitMinBytesL32 : kSplitMinBytes;
  if (!force && a.a_bytes_f64() < gate) return 0;
  if (P.method == GLX_FPROXGD) {
    if (fista_sharded) return 0;   // the row-sharded FISTA runs the dense batch
    if (a.k.split_fista.is("0")) return 0;
    return (a.line_search() && gather_ok(P.n, P.l)) ? 1 : 0;
  }
  return gather_ok(P.n, P.l) ? 1 : 0;
}

}  // namespace

SessionMode session_mode(const glx_problem& P, const glx_opts& O) {
  const SessionKnobs k{};
  const Ask a{P, O, k};
  SessionMode md;
  md.method = P.method;
  md.esize = P.dtype == GLX_F64 ? 8 : 4;
  md.m = P.m; md.n = P.n; md.l = P.l;
  md.comm = P.comm != nullptr;
  const bool f64 = P.dtype == GLX_F64, proxgd = P.method == GLX_PROXGD, fista = P.method == GLX_FPROXGD;
  md.plan = session_plan(P, O);
  // Infinity-Cache hand-off between the two non-temporal passes: the last ~192 MiB each
  // pass reads stay in the 256 MiB Infinity Cache for the other pass. NS, same box, two
  // interleaved rounds: 2307 / 2318 it/s against 2252 / 2272 with both off, either alone
  // in between (profiles/r3_keep/). GLX_AX_KEEP_MIB / GLX_ATR_KEEP_MIB = 0: off. Kernel
  // arguments through the plan, so every session and device has its own value.
  md.plan.ax_keep_mib = std::max(0, k.ax_keep_mib.num(kKeepMiB));
  md.plan.atr_keep_mib = std::max(0, k.atr_keep_mib.num(kKeepMiB));
  const GemmPlan& plan = md.plan;
  md.fh_cap = 3 * (int64_t)O.maxit;
  if (O.max_total_iters > 0) md.fh_cap = std::min<int64_t>(md.fh_cap, O.max_total_iters);

  const int fista_ranks = fista ? shard_ranks(a, 0) : 0;
  md.smode = split_mode(a, fista_ranks > 0);
  // ProxGD's fast objective mode evaluates the candidate as A p = A p_thr + A e, e = p - p_thr
  // nonzero only where the hard threshold zeroed p (see iter_proxgd, split_mode)
  md.emode = md.smode != 0 && proxgd;
  md.fsplit = md.smode == 1 && fista;
  // A e form (round 5, scripts/ec_distribution.py over whole NS solves, profiles/r5_c/): ProxGD's
  // e has ~1.1 nonzeros per flagged row (27 % of the rows), so the VALU bitmap gather does 1/30
  // of the row form's MFMA work (whole solve 2206 against 2128 it/s for the row form, 2185 for
  // the round-4 lists); FProxGD's e_c reaches 96 % of the rows with ~7.5 nonzeros each late in
  // a solve, where the row form reads every flagged At row once (whole solves 2131-2143 against
  // 2114-2121 bitmap, 2122-2124 lists).
  const int gather_asked = gather_form();
  md.gform = gather_asked >= 0 ? gather_asked : (fista ? 1 : 0);
  if (md.gform == 1 && !gather_rows_ok(P.m, P.n)) md.gform = 0;
  md.rows_form = md.gform == 1;
  md.gsplit = md.rows_form ? gather_split(P.m, P.n) : 1;
  // Round 6: ProxGD's split-candidate trial with A e fused into the dense pass (launch_ax_egat,
  // kernels_axdma.hip: A p on MFMA, A e on VALU from the same LDS chunks; no transposed copy of A,
  // no gather launch) where the session's one-source pass is the f64 LDS-DMA tile 92278 (NS).
  // Opt-in (GLX_AE_FUSED=1): same box, 200-step windows / whole solves (profiles/r6_egat/): NS
  // 2 452-2 467 / 2 461-2 467 it/s fused against 2 454-2 470 / 2 427-2 434 with the gather — level
  // in the window, +1.5 % over a solve (the gather grows late in a solve), but the fused pass runs
  // 210-218 µs against 174-176 µs: its A e (VALU, after the chunk's MFMAs) leaves the MFMA pipe of
  // both waves of a SIMD idle. Interleaving it into the MFMA stream (straight-line, or on opposite
  // sides of the two waves' MFMAs) spilled 16-208 VGPRs at 256. Throughout a solve it stays opt-in
  // (it also halves the session's workspace: no m x n copy of A); by default the session takes it
  // per trial once many rows are flagged (hyb_rows, below).
  const bool egat_fits = md.smode == 1 && proxgd && f64 && ax_egat_ok(plan, 8);
  md.egat = egat_fits && gather_asked < 0 && k.ae_fused.is("1");
  if (md.egat) md.gsplit = ax_split(plan, 1);   // the A e slabs: one per K split of the dense pass
  // the VALU gather's budget counts nonzeros of e_c, the row form's flagged rows (round 5)
  md.nnz_budget = k.split_nnz.real(md.rows_form ? kRowsBudget : 0.35) * (double)P.n;

  md.spin_readback = !k.readback.is("sync");
  // the scalar packet rides the speculative kernel queued right behind it (one extra
  // workgroup, publisher_first) instead of a k_publish launch in front of it
  md.attach_ok = md.spin_readback && !k.attach_pub.is("0");
  md.spec_off = k.spec_grad.is("0");
  md.spec_ax_pub = !k.spec_ax_pub.is("0");
  // With a communicator the trial cannot live in the A^T r epilogue (the gradient is summed
  // over ranks first): it runs as A^T r, all-reduce, then k_prox_pgd / k_fista_trial, and is
  // queued speculatively the same way (see atr_prox).
  const bool atr_fuses = atr_prox_ok(plan);
  const bool fuse_any = (md.comm || atr_fuses) && a.trial_step() && !k.fused_trial.is("0");
  // Round 5: ProxGD on one GPU whose plan cannot fuse the trial into A^T r (l not in {16, 32},
  // n % 64 != 0, ...; C1's (512, 1024, 2)) runs the communicator path's form instead: A^T r, then
  // k_prox_pgd from its slabs, queued speculatively the same way (the packet riding k_prox_pgd),
  // so device control (dc_queue_comm) applies to these shapes too. GLX_UNFUSED_SPEC=0: off (the
  // gradient and the trial as separate host-driven steps, rounds 1-4).
  md.unfused_spec = !md.comm && proxgd && !atr_fuses && a.trial_step() && !k.unfused_spec.is("0") &&
                    !k.fused_trial.is("0");
  md.fused_ok = (fuse_any || md.unfused_spec) && proxgd;
  md.fused_fista_ok = fuse_any && fista;
  // (Round 5's folded finalize — the split-candidate trial's finalize inside its dense pass,
  // GLX_AX_FIN=1 — measured slower, 2376 against 2537-2543 it/s at NS, and was removed in round 6;
  // DESIGN.md keeps the numbers.)

  // device-controlled batches (dc_run / fista_dc_run): ProxGD / FProxGD with line search on
  // the fused speculative path; GLX_DC_BATCH = iterations in flight (0: the host decides every
  // iteration). With a communicator fp64 only (the trial sums ride the gradient all-reduce).
  // The window that takes effect for this plan: the requested one (dc_window_request) where the
  // fused speculative path, the spinning readback and, with a communicator, the attached packet
  // are all on; else 0 (the host decides). Row-sharded FProxGD: host control.
  const bool dc_form = f64 && a.line_search() && O.exact_objective == 0;
  // device control on the unfused form: as with a communicator (fp64: the finalize's sums go to
  // the gradient set's tail, read as doubles), line search, fast objective mode
  const bool dc_unfused = md.unfused_spec && dc_form;
  // device control with a communicator: ProxGD, fp64 (the trial sums ride the gradient
  // all-reduce), line search, fast objective mode
  const bool dc_comm = md.comm && (proxgd || fista) && dc_form;
  const bool unf = dc_unfused && md.attach_ok;
  if (fista_ranks == 0 && (fuse_any || unf) && (proxgd || fista) && md.spin_readback &&
      O.exact_objective == 0 && a.line_search() && (!md.comm || (dc_comm && md.attach_ok)))
    md.dc_window = dc_window_request(a, unf);
  // gradient sets: 2 (current, speculative); a ring of window + 2 only where device control with
  // a communicator actually runs (it was sized on the request, not on the window
  // that takes effect), so that the all-reduces queued behind a cancelling decision (they cannot
  // be gated) never land in the set the host resumes from
  md.nsets = (md.dc_window > 0 && (dc_comm || dc_unfused)) ? md.dc_window + 2 : 2;

  const int ranks = fista ? fista_ranks : shard_ranks(a, md.dc_window);
  ShardMode& sh = md.sh;
  if (md.comm && (fista || (proxgd && md.dc_window == 0)))
    sh.cranks = comm_size(static_cast<const glx_comm*>(P.comm));
  if (ranks > 0) {
    sh.on = true;
    sh.fista = fista;
    sh.model = sh.cranks == 1;
    sh.ranks = ranks;
    sh.rank = sh.model ? 0 : comm_rank(static_cast<const glx_comm*>(P.comm));
    sh.rows = P.n / ranks;
    sh.row0 = (int64_t)sh.rank * sh.rows;
    sh.nbp = prox_blocks(sh.rows, P.l);   // k_fista_trial's grid is k_prox_pgd's
    const int64_t ml = P.m * P.l;
    if (fista) {
      sh.nbf = finalize_blocks(ml, ax_split(plan, 2), 0, sh.rows * P.l);
      sh.stv = 4;
    } else {
      // the trial finalize's workgroups (its sources: 2 in the split / dense modes, 3 exact)
      const int fsrc = O.exact_objective != 0 ? 3 : 2;
      const bool gathered = md.emode && md.smode == 1;
      sh.nbf = finalize_blocks(ml, gathered ? ax_split(plan, 1) : ax_split(plan, fsrc), gathered ? md.gsplit : 0,
                               sh.rows * P.l);
    }
    sh.chunk = kShardPartOff + sh.stv * sh.nbp + 4 * sh.nbf;
    if (!fista) {
      // A e from the bitmap / list gathers reads e only where its masks are set, where e = p:
      // the gathered p serves as e and z is not re-derived (the row form reads whole rows)
      sh.zskip = md.emode && md.gform != 1;
      // Round 6: that derive (k_trial_split) fused into the next trial's dense pass where the
      // plan's one-source tile takes it (k_ax_lds DRV: the 8-wave shard tile, f64, l = 32) and
      // the packet rides the pass (iter_proxgd_shard's speculative step). GLX_SHARD_DERIVE=0: off.
      // With it the A e gather (AxDerive: extra workgroups of that pass): k_prox_pgd writes the
      // masks and bitmaps of its rows into the rank's sums chunk (behind the partials, moff),
      // all-gathered with them, so the gather needs nothing the pass writes.
      sh.derive = sh.zskip && md.smode == 1 && !md.egat && md.gform == 0 && ax_derive_ok(plan, md.esize) &&
                  P.n % 64 == 0 && sh.rows % 64 == 0 && P.n <= 65536 && !k.shard_derive.is("0");
      sh.moff = sh.chunk;
      if (sh.derive) sh.chunk += (int)(sh.rows / 2 + P.l * sh.rows / 64);
    }
  }

  // Round 6: ProxGD's split-candidate A e chosen per trial on one GPU under host control: the
  // bitmap gather while few rows are flagged (its cost grows with them: 12 us at ~570 rows,
  // ~50 us averaged over a solve), A e fused into the dense pass (launch_ax_egat, a near-constant
  // extra) once the last accepted trial flagged at least hyb_rows rows. NS whole solves 2 538-
  // 2 541 it/s at 1 500-2 500 rows against 2 463-2 465 with the gather throughout, the 20-step
  // window unchanged (profiles/r6_hyb/). GLX_AE_HYB_ROWS: the threshold, 0 = off (the gather
  // throughout); GLX_AE_FUSED=1 keeps the fused form throughout.
  // Round 7: the fused walk re-laid (a wave owns columns of e over the block's rows,
  // kernels_axdma.hip): the fused pass costs 9 us over the plain pass instead of 19-26. The
  // threshold swept again on one box, two interleaved rounds (profiles/r7_walk/hyb_sweep.json),
  // whole solve / 200-step window in it/s: 0 (the gather throughout) 2 472-2 480 / 2 509-2 519,
  // 250 2 621-2 629 / 2 610-2 611, 500 2 621-2 623 / 2 604-2 607, 1000 2 625-2 626 / 2 604-2 612,
  // 2000 2 607-2 624 / 2 607-2 615, the fused form throughout 2 609-2 613 / 2 605-2 615. Every
  // threshold from 250 to 2000 lies within the 0.1-1.2 % run-to-run spread of the others and the
  // fused form throughout does not win both, so kHybRows stays 2000.
  if (egat_fits && !md.egat && md.gform == 0 && !md.comm && md.dc_window == 0)
    md.hyb_rows = k.ae_hyb_rows.real(kHybRows);
  // Round 5, deferred reductions (single GPU, host control, ProxGD): the fused trial (k_atr_prox)
  // and the residual finalize leave their sums as workgroup partials (Red::parts_only) instead
  // of running the grid reduction's serial tail (two arrival counters, the last workgroup's
  // loads: ~3 us at the end of each kernel); the workgroup that publishes the next packet
  // reduces them first (Pub::dpart, defer_reduce), and the finalize takes max |p| from the
  // trial's partials itself. GLX_DEFER_RED=0: off.
  // Only where the packet that follows is carried by the next speculative kernel (carry_): a
  // standalone k_publish_pub that reduces them and then writes the packet measured 17-19 us
  // against 4 us for k_publish (profiles/r5_probe/), so the non-speculative paths keep the
  // in-kernel reduction.
  // ProxGD only: FProxGD's k_atr_fista measured no gain (NS FProxGD 2583 / 2582, C3 4527 / 4535
  // it/s over 200 steps, profiles/r5_defer3/) and lost 8 % on the rejection-heavy probe
  // (its publisher's reduction stretched the 33 us fused kernel by ~4 us); that opt-in form
  // (GLX_DEFER_RED=2) was removed in round 6.
  md.defer = !md.comm && md.dc_window == 0 && proxgd && md.spin_readback && md.attach_ok && !k.defer_red.is("0");
  // Round 8: on that path the finalize of the speculative first trial runs at the head of the
  // k_atr_prox queued behind it (launch_atr_prox's head) where the fused trial is the f64 four-wave
  // panel without K splits; later trials, FProxGD, a communicator, device control and fh recording
  // keep k_finalize_residual. The device's capacity is checked by the session (fin_head_fits).
  // Opt-in (GLX_FIN_HEAD=1; unset or 0: the separate kernel everywhere): at NS the head measured
  // level with the separate kernel, not faster — whole solves 2 495-2 557 it/s against the parent's
  // 2 498-2 560, 200-step windows 2 537-2 548 against 2 544-2 555, three interleaved rounds on one
  // box (profiles/r8_finhead/). A workgroup walks its four blocks of 19 loads per thread one after
  // the other, then pays the write-through drain, the arrival, the poll and the L1 invalidate:
  // about what the 12.9 us kernel and its boundary cost ("Round 8").
  md.fin_head = md.defer && f64 && md.fused_ok && !md.unfused_spec && a.line_search() &&
                atr_prox_head_ok(plan, 1, 1) && k.fin_head.is("1");
  // SGD / GD with l = 1: the descent pass reads A once (kernels_gemv.hip); GLX_GEMV_FUSED=0
  // selects the two-pass path (A @ [x | thr(x)], then A^T r)
  if ((P.method == GLX_SGD || P.method == GLX_GD) && !k.gemv_fused.is("0"))
    md.gemv_blocks = gemv_fused_blocks(md.esize, P.m, P.n, P.l);
  return md;
}

// n / 64 panel workgroups and the publisher against the workgroups the device holds at once
bool fin_head_fits(int64_t n, int cus, int per_cu) {
  return cus > 0 && per_cu > 0 && n / 64 + 1 <= (int64_t)cus * per_cu;
}

// the kernels this session actually launches (bench.py re-derived the plan)
std::string describe_mode(const SessionMode& md) {
  const ShardMode& sh = md.sh;
  std::string s = describe_plan(md.plan);
  if (!md.comm && md.fused_ok) s += md.unfused_spec ? " +trial (k_prox_pgd behind A^T r)" : " +trial (k_atr_prox)";
  if (!md.comm && md.fused_fista_ok) s += " +trial (k_atr_fista)";
  s += "; split=";
  if (md.smode == 0) s += "dense";
  else if (md.egat) s += "A e fused into the dense pass (k_ax_dma EG), S0=" + std::to_string(md.gsplit);
  else if (md.hyb_rows > 0.0)
    s += "gather k_at_gather_bm, A e fused into the dense pass (k_ax_dma EG) from " +
         std::to_string((int64_t)md.hyb_rows) + " flagged rows";
  else if (md.rows_form) s += "rows k_at_rows S0=" + std::to_string(md.gsplit);
  else if (md.gform == 2) s += "gather k_e_lists+k_at_gather";
  else s += "gather k_at_gather_bm";
  if (sh.on) {
    s += "; rows=sharded x" + std::to_string(sh.ranks) + (sh.model ? " (timing model)" : "") +
         " (reduce-scatter of A^T r, ";
    if (sh.fista) s += "k_fista_trial on n/" + std::to_string(sh.ranks) + " rows, all-gather of xc, k_fista_split)";
    else
      s += "k_prox_pgd on n/" + std::to_string(sh.ranks) + " rows, all-gather of p, " +
           (sh.derive ? "derive and A e in the dense pass" : "k_trial_split") + ")";
  }
  return s + "; dc_window=" + std::to_string(md.dc_window);
}

}  // namespace glx
