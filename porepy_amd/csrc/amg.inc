// amg.inc — plain-aggregation algebraic multigrid, the preconditioner of the device Krylov solvers
// for the large systems (the reference solves them directly, models/solution_strategy.py:830-884;
// results are judged against its solution).
//
// Setup, one level at a time, everything on the device and deterministic:
//   * three passes of pairwise matching on the strength graph |a_ij| ("handshake": every free row
//     picks its strongest free neighbour, mutual picks pair up; a few rounds; left-over rows join the
//     pair of their strongest matched neighbour) -> aggregates of ~8 rows;
//   * after every pass the Galerkin matrix of the piecewise-constant prolongation: coarse row I =
//     the rows of its members with the columns renamed, sorted and summed in LDS (rank sort, runs
//     summed in a fixed order);
//   * coarsest level (<= kAmgDenseMax rows): explicit inverse by Gauss-Jordan with partial pivoting.
// Vector problems (bs > 1 unknowns per cell, cell-major / component-minor) aggregate cells and keep
// the components apart: P = P_cell (x) I_bs; the strength of a cell pair is the sum of the absolute
// diagonal entries of its bs x bs block.
//
// Apply = one (1,1) cycle: damped Jacobi (omega), restriction by summing the members, coarse
// correction scaled by alpha (over-correction compensates the flat prolongation), damped Jacobi;
// the first coarse level is visited twice (second visit on its residual), V-cycle below.
// It is a fixed linear operator, so BiCGStab / CG / GMRES use it as an ordinary preconditioner.
//
// The PFV_AMG_* environment switches are read in ONE place, amg_read_switches, at the start of every setup (never
// cached: callers change the environment between setups of one process); everything else takes the values from the
// AmgSwitches it fills.  amg_maps_cfg / amg_maps_tag alone define which of them the kept aggregate maps depend on.

namespace pfv {

constexpr int kAmgDenseMax = 1024;   // largest coarsest system inverted explicitly
constexpr int kAmgCoarseTargetDefault = 160;  // stop coarsening below this many rows (PFV_AMG_COARSE_TARGET)
constexpr int kAmgMaxLevels = 14;
constexpr int64_t kAmgWTopRows = 600000;  // systems from this size on visit the first coarse level twice per cycle
constexpr int kAmgFilterPermilBlock = 50;  // ... of block systems (MPSA: bs = nd)
constexpr int kAmgFilterPermil = 30;  // strength filter of scalar systems (amg_filter): drop |a_ij| < 0.03 max_k |a_ik|; 0 = off
constexpr int kAmgRounds = 4;        // handshake rounds per matching pass (6 match no more rows that matter: same iteration counts at 197 k and 664 k cells; 3 costs 3 iterations)
constexpr int kAmgPasses = 3;        // pairwise passes per level (aggregates of ~2^passes rows)
constexpr int kAmgGentleCells = 400000;  // finest levels with at least this many cells: 2 passes per level below it
constexpr int kGalEpl = 8;           // Galerkin product: entries of a coarse row per lane in the batched gather
constexpr int kGalMaxMembers = 16;   // ... and member rows of an aggregate it handles (more: member-by-member gather)
constexpr int64_t kAmgGatherRowsDefault = 32768;  // coupled hierarchy: levels of at most this many rows over all ranks are gathered

// The switches of one setup of the plain hierarchy (and of the helpers the near-null-space hierarchy shares with it).
struct AmgSwitches {
  int bs = 1;  // block size the defaults were resolved for
  // damping of the Jacobi smoothers: PFV_AMG_OMEGA_PCT fixes it for all levels (80 was the value fitted to the benchmark
  // matrix: 70 -> 27, 80 -> 23, 90 -> 3455 iterations -- at 0.9 omega rho(D^-1 A) crosses 2 and the smoother amplifies);
  // unset, every level gets omega = PFV_AMG_OMEGA_RHO_PCT / 100 / rho_l from a power-iteration estimate of its own
  // rho(D^-1 A) (amg_estimate_omegas) when PFV_AMG_OMEGA_AUTO is on
  bool omega_auto = false;
  // (scalar systems run the row-wise safeguard, amg_safeguard_rows: any omega <= 1 is stable there and the iteration
  // count falls monotonically towards 1 -- 0.7: 28, 0.8: 26, 0.9: 24, 1.0: 22 at 197 k cells; block systems keep 0.8)
  bool safe_rows = true;  // PFV_AMG_SAFE_ROWS (block systems: switch only)
  double omega = 0.95, alpha = 1.5;  // PFV_AMG_OMEGA_PCT (default 95 with the safeguard, else 80), PFV_AMG_ALPHA_PCT
  int omega_power_steps = 10;        // PFV_AMG_OMEGA_POWER_STEPS, 2..30
  double omega_sigma = 1.8;          // PFV_AMG_OMEGA_RHO_PCT / 100
  int passes = kAmgPasses;           // PFV_AMG_PASSES, 1..6
  // PFV_AMG_PASSES_COARSE as given (-1: unset -- the default follows the size of the finest level, amg_coarsen_level,
  // which also clamps to 1..6)
  bool passes_coarse_set = false;
  int passes_coarse_raw = -1;
  int rounds = kAmgRounds, rounds_raw = kAmgRounds;  // PFV_AMG_ROUNDS: 1..12 for the matching / as given for amg_maps_cfg
  int strength_neg = 0;              // PFV_AMG_STRENGTH_NEG (AmgGraph::neg_only)
  bool fp32 = true;                  // PFV_AMG_FP32
  // PFV_AMG_FILTER_PERMIL / _BLOCK, as a fraction
  // (block systems: blocks weaker than 0.05 of the strongest of either end.  configs[3], 1.5 M dofs: 0.03 -> 263 ms per
  // step, 0.1 -> 243, against ~280 unfiltered; 0.2 costs 67 instead of 43 iterations and 0.3 diverges -- the block
  // measure is cruder than the scalar one, the default keeps a factor 4 from the first degradation)
  double filter_theta = 0.0;
  int coarse_target = kAmgCoarseTargetDefault;  // PFV_AMG_COARSE_TARGET, 1..kAmgDenseMax
  // W at the top (second visit of the first coarse level) pays on large systems, where the finest-level products
  // dominate and every saved Krylov iteration is worth ~1.6 ms (2 M cells: 89.6 vs 92.4 ms per step); below
  // kAmgWTopRows the cycle is a chain of ~5 us launches and the second visit just doubles it (197 k cells: 13.1 vs
  // 15.1 ms, 257 k: 18.2 vs 21.8 ms with the V-cycle although it needs 3-4 iterations more)
  // PFV_AMG_GAMMA as given: the default follows the size, which the coupled hierarchy learns from its gather (amg_setup
  // resolves and clamps to 1..2)
  bool gamma_set = false;
  int gamma_raw = 0;
  int gamma_levels = 1;              // PFV_AMG_GAMMA_LEVELS
  // fused launches on the small levels (neutral at 2 M cells, -2 ms per step at 200-260 k cells)
  int64_t fuse_rows = 30000;         // PFV_AMG_FUSE_ROWS
  bool fuse_cycle = true;            // PFV_AMG_FUSE_CYCLE
  // measured (profiles/r02_ab_runs.txt): -1.5 ms per step on the 2 M-cell scalar system, +5 ms on the 1.5 M-dof
  // block system of configs[3] -> lanes for scalar systems only
  bool restrict_lanes = true;        // PFV_AMG_RESTRICT_LANES
  bool reuse = true, reuse_dist = true, reuse_rebuilt = true;  // PFV_AMG_REUSE, _REUSE_DIST, _REUSE_REBUILT (amg_decide_reuse)
  // (measured on one rank over RCCL, new coefficients every step: 2 M rows 76.1 -> 74.5 ms per step with the maps
  // kept, 257 k rows 18.2 -> 18.7 ms -- there the kept aggregates cost 4 iterations and save 0.4 ms of setup: small
  // shares re-match)
  int reuse_dist_min_rows = 500000;  // PFV_AMG_REUSE_DIST_MIN_ROWS
  bool members_reuse = true, sizes_reuse = true;  // PFV_AMG_MEMBERS_REUSE, PFV_AMG_SIZES_REUSE
  // PFV_AMG_FILTER_SMOOTH, _ROWMAX_REUSE, _FILTER_LAYOUT_REUSE, _SKIP_MOVED_DIGEST (amg_setup_level0)
  bool filter_smooth = true, rowmax_reuse = true, filter_layout_reuse = true, skip_moved_digest = true;
  // how the work is launched: PFV_AMG_GALERKIN_BATCHED, _FILTER_UNROLL, _DENSE_LDS
  bool galerkin_batched = true, filter_unroll = true, dense_lds = true;
  int64_t gather_rows = kAmgGatherRowsDefault;  // PFV_AMG_GATHER_ROWS, >= 1
  bool post_ap = true;               // PFV_AMG_POST_AP: finest post-smoothing through A_s P (amg_build_ap / amg_post_ap)
  bool galerkin_ap = true;           // PFV_AMG_GALERKIN_AP: kept maps: the first coarse operator as P^T (A_s P) (amg_coarsen_level)
  // level 0 on the AP path (amg_cycle): the product leaves d = b - A_s x0 (PFV_AMG_L0_RESIDUAL), formed by 4 lanes per
  // row where the level has windows and short rows (PFV_AMG_L0_LANES4), the BiCGStab updates write the first smoothing
  // step (PFV_AMG_KRYLOV_PRESMOOTH)
  bool l0_residual = true, l0_lanes4 = true, krylov_presmooth = true;
};

static AmgSwitches amg_read_switches(int bs) {
  auto given = [](const char* name, int& v) {  // false: unset, v untouched
    const char* e = std::getenv(name);
    if (e) v = std::atoi(e);
    return e != nullptr;
  };
  auto on = [](const char* name, int dflt) { return env_int(name, dflt) != 0; };
  AmgSwitches w;
  w.bs = bs;
  w.safe_rows = on("PFV_AMG_SAFE_ROWS", bs == 1 ? 1 : 0);
  int omega_pct = w.safe_rows ? 95 : 80;
  w.omega_auto = !given("PFV_AMG_OMEGA_PCT", omega_pct) && on("PFV_AMG_OMEGA_AUTO", 0);
  w.omega = 0.01 * omega_pct;
  w.alpha = 0.01 * env_int("PFV_AMG_ALPHA_PCT", 150);
  w.omega_power_steps = std::max(2, std::min(30, env_int("PFV_AMG_OMEGA_POWER_STEPS", 10)));
  w.omega_sigma = 0.01 * env_int("PFV_AMG_OMEGA_RHO_PCT", 180);
  w.passes = std::max(1, std::min(6, env_int("PFV_AMG_PASSES", kAmgPasses)));
  w.passes_coarse_set = given("PFV_AMG_PASSES_COARSE", w.passes_coarse_raw);
  w.rounds_raw = env_int("PFV_AMG_ROUNDS", kAmgRounds);
  w.rounds = std::max(1, std::min(12, w.rounds_raw));
  w.strength_neg = env_int("PFV_AMG_STRENGTH_NEG", 0);
  w.fp32 = on("PFV_AMG_FP32", 1);
  w.filter_theta = 0.001 * env_int(bs == 1 ? "PFV_AMG_FILTER_PERMIL" : "PFV_AMG_FILTER_PERMIL_BLOCK",
                                   bs == 1 ? kAmgFilterPermil : kAmgFilterPermilBlock);
  w.coarse_target = std::max(1, std::min(kAmgDenseMax, env_int("PFV_AMG_COARSE_TARGET", kAmgCoarseTargetDefault)));
  w.gamma_set = given("PFV_AMG_GAMMA", w.gamma_raw);
  w.gamma_levels = env_int("PFV_AMG_GAMMA_LEVELS", 1);
  w.fuse_rows = env_int("PFV_AMG_FUSE_ROWS", 30000);
  w.fuse_cycle = on("PFV_AMG_FUSE_CYCLE", 1);
  w.restrict_lanes = on("PFV_AMG_RESTRICT_LANES", bs == 1 ? 1 : 0);
  w.reuse = on("PFV_AMG_REUSE", 1);
  w.reuse_dist = on("PFV_AMG_REUSE_DIST", 1);
  w.reuse_rebuilt = on("PFV_AMG_REUSE_REBUILT", 1);
  w.reuse_dist_min_rows = env_int("PFV_AMG_REUSE_DIST_MIN_ROWS", 500000);
  w.members_reuse = on("PFV_AMG_MEMBERS_REUSE", 1);
  w.sizes_reuse = on("PFV_AMG_SIZES_REUSE", 1);
  w.filter_smooth = on("PFV_AMG_FILTER_SMOOTH", 1);
  w.rowmax_reuse = on("PFV_AMG_ROWMAX_REUSE", 1);
  w.filter_layout_reuse = on("PFV_AMG_FILTER_LAYOUT_REUSE", 1);
  w.skip_moved_digest = on("PFV_AMG_SKIP_MOVED_DIGEST", 1);
  w.galerkin_batched = on("PFV_AMG_GALERKIN_BATCHED", 1);
  w.filter_unroll = on("PFV_AMG_FILTER_UNROLL", 1);
  w.dense_lds = on("PFV_AMG_DENSE_LDS", 1);
  w.gather_rows = std::max<int64_t>(1, env_int("PFV_AMG_GATHER_ROWS", (int)kAmgGatherRowsDefault));
  w.post_ap = on("PFV_AMG_POST_AP", 1);
  w.galerkin_ap = on("PFV_AMG_GALERKIN_AP", 1);
  w.l0_residual = on("PFV_AMG_L0_RESIDUAL", 1);
  w.l0_lanes4 = on("PFV_AMG_L0_LANES4", 1);
  w.krylov_presmooth = on("PFV_AMG_KRYLOV_PRESMOOTH", 1);
  return w;
}

// The parameters the aggregate maps depend on, in one word: a setup whose word differs from the one the kept maps were
// built with re-matches.  (The arithmetic is part of what the ranks of a coupled hierarchy exchange: keep it.)
static int64_t amg_maps_cfg(const AmgSwitches& w) {
  return ((((int64_t)w.passes * 16 + w.rounds_raw) * 16 + w.passes_coarse_raw + 1) * 4 + w.strength_neg) * 65536 +
         w.coarse_target * 8 + w.bs + (int64_t)(1000.0 * w.filter_theta + 0.5) * (int64_t(1) << 40);
}
// (coupled hierarchy: the matching parameters again, compared beside the word above)
static int amg_maps_tag(const AmgSwitches& w) { return w.rounds_raw * 64 + w.passes_coarse_raw + 1; }

struct AmgLevel {
  int64_t n = 0;                 // rows of this level's matrix
  int64_t m = 0;                 // its columns (= n; coupled hierarchy of a sharded solve: owned + halo unknowns)
  const CsrPattern* P = nullptr;  // this level's matrix (level 0: the system itself)
  const double* val = nullptr;
  CsrPattern P_own;
  Buf<double> val_own;
  Buf<float> val32;         // single-precision copy of val for the cycle's products (empty: use val)
  const float* v32 = nullptr;
  WinCsr win_own;           // SpMV window of this level's pattern (level 0: the caller's)
  const WinCsr* win = nullptr;
  Buf<double> dinv;
  Buf<int32_t> agg;         // [n / bs] cell -> coarse cell of the next level
  Buf<int32_t> mptr, mem;   // members (cells, ascending) of every coarse cell
  int64_t nc_cells = 0;     // coarse cells
  Buf<int32_t> pmap[6];     // the pairwise maps of the passes that built agg (kept for a values-only re-setup)
  int64_t pmap_n[6] = {0, 0, 0, 0, 0, 0};
  int pmap_count = 0;
  Buf<int32_t> pmp[6], pme[6];  // member lists of those maps (functions of the maps alone: kept with them)
  bool members_kept = false;    // mptr / mem / agg of this level belong to the kept maps (PFV_AMG_MEMBERS_REUSE)
  Buf<double> x, b, t;      // cycle vectors (level 0 uses the caller's x and b)
  Buf<double> r2, x2;       // second coarse visit (PFV_AMG_GAMMA = 2)
  Buf<double> u;            // result of the first visit of a level visited twice when its up-leg is fused (t serves the second)
  double omega = 0.8;       // damping of this level's Jacobi smoother (amg_estimate_omegas)
  double rho = 0.0;         // its estimate of rho(D^-1 A) (0: not estimated)
};

// scratch of the setup phase; lives with the hierarchy so that repeated setups (one per
// re-assembled matrix) allocate nothing
struct AmgWork {
  Buf<int32_t> match, pick, join, lead, a1, mp, me, cap, cnt, tcol, vin;
  Buf<uint32_t> kin, kout;
  Buf<int64_t> pos, tptr, cptr;
  Buf<double> tval, dense_work;
  Buf<int32_t> piv;
  Buf<unsigned long long> csum;
  CsrPattern P[2];   // intermediate Galerkin matrices of the passes of one level (ping-pong)
  Buf<double> V[2], D[2];
};

// ---- coupled hierarchy of a sharded solve (pfv_amg_setup_sharded; amg_dist.inc)
// halo plan of one level, in cells (bs unknowns per cell travel)
struct AmgPlan {
  int n_peers = 0;
  std::vector<int32_t> peers;
  std::vector<int64_t> send_ptr, recv_ptr;      // [n_peers + 1]
  std::vector<int32_t> h_send_idx, h_recv_pos;  // host copies (the next level's plan is derived from them)
  Buf<int32_t> send_idx, recv_pos;              // device: owned cells to pack / local cells (>= n_own) to fill
  int64_t n_send = 0, n_recv = 0;
  int64_t n_own = 0, n_halo = 0;                // owned / halo cells of the level
  // who owns halo cell h (position n_own + h) and under which of its own cell numbers
  std::vector<int32_t> halo_peer, halo_owner_id;
};
struct Amg;
struct AmgDist {
  ~AmgDist() {  // rows0 borrows the index arrays of the system's pattern
    rows0.indptr.p = nullptr;
    rows0.indices.p = nullptr;
  }
  CsrPattern rows0;  // the rows of the owned unknowns of the active system, all local columns
  pfv_shard_hooks hooks{};
  int rank = 0, world = 1;
  std::vector<std::unique_ptr<AmgPlan>> plan;  // plan[l]: level l < kgather
  size_t kgather = 0;                          // first gathered level: replicated on all ranks from here down
  Buf<double> sbuf, rbuf, gid;
  Buf<int32_t> aext, itmp, chalo;
  // gathered level
  std::unique_ptr<Amg> glob;
  std::vector<int64_t> gn, goff;               // rows of every rank at the gathered level, their offsets
  int64_t gN = 0, gnmax = 0;
  Buf<int64_t> gn_d, goff_d, cnt_s, cnt_r;
  Buf<double> gsend, grecv, gb, gx, gV, gval_s, gval_r;
  Buf<int32_t> glen_s, glen_r, gcol_s, gcol_r, hal_gcell;
  CsrPattern gT, gP;
  Buf<double> gTV, gD;
  Buf<int32_t> gagg, gmp, gme;
  int64_t exchanges = 0, allgathers = 0;       // since the setup
  int64_t global_rows0 = 0, global_rows_level = 0;  // rows over all ranks: finest level / the level being coarsened
};

struct Amg {
  Amg();
  ~Amg();
  std::unique_ptr<AmgDist> dist;  // set: coupled hierarchy
  bool no_filter = false;         // (the replicated hierarchy below a gathered level)
  int64_t finest_cells_parent = 0;  // ... cells of the finest level of the hierarchy it continues (0: it is its own)
  std::vector<std::unique_ptr<AmgLevel>> lev;
  size_t nlev = 0;     // levels in use (lev may hold more, kept for their buffers)
  AmgWork wk;
  int bs = 1;
  AmgSwitches sw;  // the switches of the last setup, with this hierarchy's own overrides (no_filter, coarse_target) applied
  // ... and what the cycle and pfv_amg_level read of them
  int passes = kAmgPasses;
  double omega = 0.8, alpha = 1.5;  // omega: fixed damping when PFV_AMG_OMEGA_PCT is set, else per level (AmgLevel::omega)
  bool omega_auto = true;
  Buf<double> pw_a, pw_b, pw_zero, pw_part;  // power-iteration scratch
  Buf<double> dense;   // inverse of the coarsest matrix, row-major n x n
  unsigned long long filt_layout_for = 0;  // checksum of the finest pattern filtP's row pointers were computed for
  bool filt_layout_stable = false;         // the last filtering reproduced the layout of the one before it
  CsrPattern filtP;    // strength-filtered copy of the finest matrix the hierarchy is coarsened from (amg_filter)
  Buf<double> filtV;
  double filter_theta = 0.0;
  int64_t filt_nnz = 0;
  bool filter_level0 = false;  // the cycle's finest level smooths with the filtered matrix too
  WinCsr filt_win;
  // sizes the Galerkin products read back from the device (largest gathered row, entries of the product), in the order
  // the setup forms them: valid for the next setup when the finest pattern (checksum gal_for_sum) and the aggregate maps
  // are the same -- the products then have the same patterns, and ~2 host reads per product (26 per setup of the 2 M-cell
  // system, each a stream synchronisation) are saved
  struct GalSizes { int64_t ncr, annz, nnz; int maxcap; };
  std::vector<GalSizes> gal_sizes;
  unsigned long long gal_for_sum = 0;
  bool gal_use = false;
  size_t gal_k = 0;
  int gal_route = 0;  // how the setup that recorded gal_sizes formed level 1 (0: passes, 1: from AP): the record is a sequence
                      // in call order, and the two routes make different calls (amg_gal_route)
  unsigned long long filt_win_sum = 0;  // checksum of the filtered pattern filt_win was built for (0: unknown)
  // what the saved aggregate maps belong to: size, block size, setup parameters, checksum of the
  // pattern and the context's symbolic epoch (a re-built discretization never reuses)
  bool maps_ok = false, reused = false;
  int64_t maps_n = -1, maps_nnz = -1, maps_cfg = 0;
  unsigned long long maps_sum = 0, maps_epoch = 0;
  int maps_tag = 0;  // (coupled hierarchy: the setup parameters the maps were built with, known before the gather)
  // staleness of kept maps: the aggregates follow the strength of connection of the values they were MATCHED on; with
  // coefficients that drift away from those the cycle degrades slowly.  note_iterations() remembers the count of the
  // first solve after a fresh matching and drops the maps (the next setup re-matches) when a solve on kept maps to the
  // same tolerance needs more than kAmgStaleFactor times as many.  Sharded solves: the count is the same on all ranks,
  // so every rank drops its maps in the same step -- and `maps_ok` goes through the all-ranks vote anyway.
  int iters_fresh = -1;
  int method_fresh = -1;
  double rtol_fresh = 0.0;
  int64_t stale_rematches = 0;
  void note_iterations(int iterations, double rtol, int method, bool converged) {
    if (!valid) return;
    if (!reused) {
      iters_fresh = converged ? iterations : -1;
      rtol_fresh = rtol;
      method_fresh = method;
    } else if (iters_fresh > 0 && rtol == rtol_fresh && method == method_fresh &&
               (!converged || (double)iterations > 1.3 * (double)iters_fresh + 1.0)) {
      maps_ok = false;
      ++stale_rematches;
    }
  }
  bool dense_ok = false;
  bool restrict_lanes = true;
  bool valid = false;
  // coarse visits per cycle on the first gamma_levels levels: the first coarse level is visited twice
  // (a W-cycle restricted to the top; below it the small levels are launch-bound, where every extra
  // visit costs ~55 us per level: 25 -> 18 BiCGStab iterations on the 2 M-cell system, solve -8 ms)
  int gamma = 2, gamma_levels = 1;
  int coarse_target = 0;  // > 0: stop coarsening at this many rows instead of PFV_AMG_COARSE_TARGET (block preconditioner:
                          // blocks of at most kAmgDenseMax rows get an exact dense inverse, one level)
  int64_t fuse_rows = 0;  // levels up to this many rows run the fused launches (amg_restrict_residual / amg_prolong_smooth)
  bool fuse_cycle = true;  // larger coarse levels: prolongation inside the post-smoothing product, the second visit's residual
                           // and first smoothing step in one product, its correction folded into the parent's prolongation
  bool fp32 = true;    // cycle products read single-precision matrix values (vectors stay double)
  double setup_ms = 0.0, op_complexity = 0.0;
  // AP = A_s P of level 0 (amg_build_ap): compact CSR, n rows x coarse cells of level 0, values double, columns ascending
  bool ap_ok = false;
  int64_t ap_nnz = 0;
  Buf<int32_t> ap_ptr, ap_col, ap_len;
  Buf<int64_t> ap_pos;
  Buf<double> ap_val;
  // the same rows with the sums of the double values of A_s, where the first coarse operator is formed from them
  // (amg_coarsen_level; entry order and packing of ap_val)
  bool ap64_ok = false;
  Buf<double> ap_val64, ap_row64;  // (ap_row64: the sums in the rows' slots before packing, beside wk.tval)
  bool galerkin_ap = false;  // the last setup formed level 1 as P^T (A_s P)
  const CsrPattern* sysP = nullptr;  // the matrix the last setup was given (before the filter; pfv_amg_level reads it)
  const double* sysV = nullptr;
};

// which spelling of the cycle level l takes (amg_cycle decides by it; pfv_amg_level reports it)
struct AmgPath {
  bool small = false;     // residual inside the restriction (amg_restrict_residual)
  bool twice = false;     // this level is visited twice by its parent
  bool fuse_up = false;   // prolongation inside the post-smoothing product of a small level (amg_prolong_smooth)
  bool fuse_big = false;  // ... of a larger level (MODE 4 of the products)
  bool second = false;    // this level visits the next one a second time
};
static AmgPath amg_level_path(const Amg& amg, size_t l) {
  AmgPath p;
  if (l + 1 >= amg.nlev) return p;
  const AmgLevel& L = *amg.lev[l];
  p.small = L.n <= amg.fuse_rows && !(L.win && L.win->ok);
  p.twice = amg.gamma == 2 && l >= 1 && (int)l <= amg.gamma_levels;
  p.fuse_up = p.small && l >= 1 && !p.twice;
  p.fuse_big = amg.fuse_cycle && !p.small && l >= 1;
  p.second = amg.gamma == 2 && (int)l < amg.gamma_levels && l + 2 < amg.nlev;
  return p;
}

inline Amg::Amg() = default;
inline Amg::~Amg() = default;
static bool amg_gal_cached(Amg* amg, int64_t ncr, int64_t annz, int* maxcap, int64_t* nnz) {
  if (!amg || !amg->gal_use || amg->gal_k >= amg->gal_sizes.size()) return false;
  const Amg::GalSizes& g = amg->gal_sizes[amg->gal_k];
  if (g.ncr != ncr || g.annz != annz) {  // (cannot happen on equal patterns and maps: fall back to reading for the rest)
    amg->gal_use = false;
    amg->gal_sizes.resize(amg->gal_k);
    return false;
  }
  *maxcap = g.maxcap;
  *nnz = g.nnz;
  ++amg->gal_k;
  return true;
}
static void amg_gal_record(Amg* amg, int64_t ncr, int64_t annz, int maxcap, int64_t nnz) {
  if (!amg) return;
  if (amg->gal_k < amg->gal_sizes.size()) amg->gal_sizes.resize(amg->gal_k);
  amg->gal_sizes.push_back(Amg::GalSizes{ncr, annz, nnz, maxcap});
  amg->gal_k = amg->gal_sizes.size();
}
// Before the first product of a setup: a record made on the other route does not describe this setup's calls.
static void amg_gal_route(Amg& amg, int route) {
  if (amg.gal_route != route) {
    amg.gal_use = false;
    amg.gal_sizes.clear();
    amg.gal_k = 0;
  }
  amg.gal_route = route;
}

// ---- graph access: cell i, k-th neighbour block (full bs x bs blocks, see header comment)
struct AmgGraph {
  const int32_t* ip;
  const int32_t* ix;
  const double* val;
  int bs;
  int neg_only;  // strength of connection counts only couplings of the sign an M-matrix has (-a_ij > 0)
  PFV_HD int nblk(int64_t i) const { return (ip[i * bs + 1] - ip[i * bs]) / bs; }
  PFV_HD int col(int64_t i, int k) const { return ix[ip[i * bs] + k * bs] / bs; }
  PFV_HD double w(int64_t i, int k) const {
    double s = 0.0;
    for (int a = 0; a < bs; ++a) {
      const double v = val[ip[i * bs + a] + k * bs + a];
      s += neg_only ? (v < 0.0 ? -v : 0.0) : fabs(v);
    }
    return s;
  }
};

// symmetric edge hash: ties between equally strong neighbours are broken the same way from both
// ends, so every locally dominant edge is a mutual pick (lowest-index tie-breaking would match one
// pair per grid line and round on uniform grids)
PFV_HD inline uint32_t amg_edge_hash(int64_t i, int64_t j) {
  uint64_t a = (uint64_t)(i < j ? i : j), b = (uint64_t)(i < j ? j : i);
  uint64_t z = a * 0x9E3779B97F4A7C15ull + b + 0x7F4A7C15ull;
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return (uint32_t)(z >> 32);
}

// strongest eligible neighbour of every free row; a lane group per row reads the row coalesced,
// candidates are (weight, symmetric edge hash, column) and the group's best is picked by lane 0.
// want_matched = 0: free neighbours (handshake round), 1: neighbours already in a pair (joining)
static void amg_pick_pass(pfv_ctx_impl& c, const AmgGraph g, int64_t nb, const int32_t* match, int want_matched,
                          int32_t* out) {
  stream_t s = c.stream;
  const size_t lds_pick = 16 * (8 + 4 + 4) + 16;
  wave_for<16>(s, nb, lds_pick, PFV_LAMBDA(const WaveCtx& w) {
    const int64_t i = w.item;
    if (match[i] >= 0) {
      if (w.lane0()) out[i] = -1;
      return;
    }
    double* cw = reinterpret_cast<double*>(w.lds);
    uint32_t* ch = reinterpret_cast<uint32_t*>(cw + 16);
    int32_t* cj = reinterpret_cast<int32_t*>(ch + 16);
    double bw = 0.0;
    uint32_t bh = 0;
    int best = -1;
    const int m = g.nblk(i);
    PFV_LANES(k, m) {
      const int j = g.col(i, k);
      // (coupled hierarchy: columns >= nb are cells of other ranks -- never partners)
      const bool eligible = (j != i) && j < nb && ((match[j] >= 0) == (want_matched != 0));
      if (eligible) {
        const double wt = g.w(i, k);
        if (wt > 0.0 && !(wt < bw)) {
          const uint32_t h = amg_edge_hash(i, j);
          if (wt > bw || h > bh) { bw = wt; bh = h; best = j; }
        }
      }
    }
    cw[w.lane] = bw;
    ch[w.lane] = bh;
    cj[w.lane] = best;
    w.sync();
    if (w.lane0()) {
      for (int l = 1; l < w.width; ++l) {
        if (cj[l] >= 0 && (cw[l] > bw || (cw[l] == bw && ch[l] > bh))) { bw = cw[l]; bh = ch[l]; best = cj[l]; }
      }
      out[i] = best;
    }
    w.sync();
  });
}

// one pairwise pass on the cell graph of (P, val): agg[i] in [0, nagg), returns nagg
static int64_t amg_pairwise(pfv_ctx_impl& c, const AmgSwitches& sw, AmgWork& wk, const CsrPattern& P, const double* val,
                            int bs, Buf<int32_t>& agg_out) {
  stream_t s = c.stream;
  const int64_t nb = P.nrows / bs;
  AmgGraph g{P.indptr, P.indices, val, bs, sw.strength_neg};
  int32_t* match = wk.match.ensure(nb);
  int32_t* pick = wk.pick.ensure(nb);
  int32_t* join = wk.join.ensure(nb);
  int32_t* lead = wk.lead.ensure(nb + 1);
  int64_t* pos = wk.pos.ensure(nb + 1);
  parallel_for(s, nb, PFV_LAMBDA(int64_t i) { match[i] = -1; });
  for (int round = 0; round < sw.rounds; ++round) {
    amg_pick_pass(c, g, nb, match, 0, pick);
    parallel_for(s, nb, PFV_LAMBDA(int64_t i) {
      const int p = pick[i];
      if (p >= 0 && pick[p] == (int32_t)i) match[i] = p;
    });
  }
  // left-over rows join the pair of their strongest matched neighbour
  amg_pick_pass(c, g, nb, match, 1, join);
  parallel_for(s, nb, PFV_LAMBDA(int64_t i) {
    lead[i] = (match[i] >= 0) ? ((int32_t)i < match[i] ? 1 : 0) : (join[i] < 0 ? 1 : 0);
  });
  exclusive_scan<int32_t, int64_t>(s, c.scratch, lead, pos, (size_t)nb);
  const int64_t nagg = read_scalar<int64_t>(s, pos + nb);
  int32_t* agg = agg_out.ensure(nb);
  parallel_for(s, nb, PFV_LAMBDA(int64_t i) {
    int l;
    if (match[i] >= 0) l = (int32_t)i < match[i] ? (int32_t)i : match[i];
    else if (join[i] >= 0) l = join[i] < match[join[i]] ? join[i] : match[join[i]];
    else l = (int32_t)i;
    agg[i] = (int32_t)pos[l];
  });
  return nagg;
}

// members of every aggregate, ascending (stable sort of the cells by aggregate)
static void amg_members(pfv_ctx_impl& c, AmgWork& wk, const int32_t* agg, int64_t nb, int64_t nagg,
                        Buf<int32_t>& mptr_, Buf<int32_t>& mem_) {
  stream_t s = c.stream;
  uint32_t* k = wk.kin.ensure(nb);
  uint32_t* ko = wk.kout.ensure(nb);
  int32_t* v = wk.vin.ensure(nb);
  int32_t* mem = mem_.ensure(nb);
  int32_t* mptr = mptr_.ensure(nagg + 1);
  parallel_for(s, nb, PFV_LAMBDA(int64_t i) {
    k[i] = (uint32_t)agg[i];
    v[i] = (int32_t)i;
  });
  int bits = 1;
  while ((int64_t(1) << bits) < nagg) ++bits;
  sort_pairs(s, c.scratch, k, ko, v, mem, (size_t)nb, bits);
  parallel_for(s, nagg + 1, PFV_LAMBDA(int64_t I) {
    mptr[I] = (int32_t)lower_bound_idx<uint32_t>(ko, (int)nb, (uint32_t)I);
  });
}

// Galerkin matrix of the piecewise-constant prolongation given by agg: Ac = P^T A P, and the
// inverse of its diagonal.  One lane group per coarse row: the entries of the member rows are
// gathered with renamed columns, sorted by (column, gather position) with a bitonic network in LDS,
// and every run of equal columns is summed in gather order (deterministic).
struct Amg;
static bool amg_gal_cached(Amg* amg, int64_t ncr, int64_t annz, int* maxcap, int64_t* nnz);
static void amg_gal_record(Amg* amg, int64_t ncr, int64_t annz, int maxcap, int64_t nnz);
// The fine matrix comes as its arrays: (ip, ix, val) with `annz` an upper bound of its entries that is known on the host
// (the exact count where the caller has it; the product from AP only knows the bound, amg_coarsen_level).  agg == nullptr:
// the columns are coarse unknowns already.
static void amg_galerkin_csr(pfv_ctx_impl& c, const AmgSwitches& sw, AmgWork& wk, const int32_t* ip, const int32_t* ix,
                             int64_t annz, const double* val, int bs, const int32_t* agg, const int32_t* mptr,
                             const int32_t* mem, int64_t nagg, CsrPattern& Ac, Buf<double>& valc, Buf<double>& dinvc,
                             Amg* sizes = nullptr) {
  stream_t s = c.stream;
  const int64_t ncr = nagg * bs;  // coarse rows
  int32_t* cap = wk.cap.ensure(ncr + 1);
  int32_t* cnt = wk.cnt.ensure(ncr + 1);
  int64_t* tptr = wk.tptr.ensure(ncr + 1);
  int64_t* cptr = wk.cptr.ensure(ncr + 1);
  int32_t* st = c.status.ensure(16);
  be_memset(st + 8, 0, sizeof(int32_t) * 2, s);
  parallel_for(s, ncr, PFV_LAMBDA(int64_t R) {
    const int64_t I = R / bs;
    const int a = (int)(R - I * bs);
    int m = 0;
    for (int q = mptr[I]; q < mptr[I + 1]; ++q) {
      const int64_t r = (int64_t)mem[q] * bs + a;
      m += ip[r + 1] - ip[r];
    }
    cap[R] = m;
    track_max_i32(st + 8, m);
  });
  exclusive_scan<int32_t, int64_t>(s, c.scratch, cap, tptr, (size_t)ncr);
  int maxcap_c = 0;
  int64_t nnz_c = 0;
  const bool known = amg_gal_cached(sizes, ncr, annz, &maxcap_c, &nnz_c);
  const int maxcap = known ? maxcap_c : read_scalar<int32_t>(s, st + 8);
  const int64_t ttot = annz;  // every fine row feeds exactly one coarse row (>= tptr[ncr], no need to read it)
  if (maxcap > 4096) throw Error(PFV_ERR_UNSUPPORTED, "AMG: more than 4096 entries feed one coarse row");
  int32_t* tcol = wk.tcol.ensure(std::max<int64_t>(ttot, 1));
  double* tval = wk.tval.ensure(std::max<int64_t>(ttot, 1));
  double* dinv = dinvc.ensure(std::max<int64_t>(ncr, 1));
  be_memset(dinv, 0, sizeof(double) * (size_t)ncr, s);
  const int capL = std::max(maxcap, 1);
  const int G = capL <= 64 ? 16 : (capL <= 160 ? 32 : 64);
  int capP = 2;
  while (capP < capL) capP <<= 1;
  const int nw = capP / 64 + 1;
  // LDS per coarse row: composite sort keys (column << 32 | gather position) | values | head mask
  const size_t lds = 8 * (size_t)capP + 8 * (size_t)capL + 8 * (size_t)nw + 4 * (2 * kGalMaxMembers + 1) + 64;
  // every lane of the group holds at most kGalEpl entries of the coarse row in registers
  const bool batched = capL <= kGalEpl * G && sw.galerkin_batched;
  wave_for_g(G, s, ncr, lds, PFV_LAMBDA(const WaveCtx& w) {
    const int64_t R = w.item;
    const int64_t I = R / bs;
    const int a = (int)(R - I * bs);
    unsigned long long* key = reinterpret_cast<unsigned long long*>(w.lds);
    double* v0 = reinterpret_cast<double*>(key + capP);
    unsigned long long* mask = reinterpret_cast<unsigned long long*>(v0 + capL);
    int m = 0;
    const int q0 = mptr[I], nm = mptr[I + 1] - q0;
    if (batched && nm <= kGalMaxMembers && cap[R] <= kGalEpl * w.width) {
      // Gather with the loads batched: the chain row -> column -> aggregate is three dependent global
      // loads, and walking the member rows one after the other (below) pays it once per member and
      // trip.  Here a lane first fetches the columns of all its entries, then all their aggregates.
      int32_t* mp0 = reinterpret_cast<int32_t*>(mask + nw);  // [kGalMaxMembers] first entry of the member rows
      int32_t* mof = mp0 + kGalMaxMembers;                   // [kGalMaxMembers + 1] offsets in the coarse row
      PFV_LANES(q, nm) {
        const int64_t r = (int64_t)mem[q0 + q] * bs + a;
        mp0[q] = ip[r];
        mof[q + 1] = ip[r + 1] - ip[r];
      }
      w.sync();
      if (w.lane0()) {
        mof[0] = 0;
        for (int q = 0; q < nm; ++q) mof[q + 1] += mof[q];
      }
      w.sync();
      m = mof[nm];
      int cidx[kGalEpl];
      double vv[kGalEpl];
#pragma unroll
      for (int k = 0; k < kGalEpl; ++k) {
        const int e = w.lane + k * w.width;
        cidx[k] = -1;
        vv[k] = 0.0;
        if (e < m) {
          int q = 0;
          while (q + 1 < nm && e >= mof[q + 1]) ++q;
          const int src = mp0[q] + (e - mof[q]);
          cidx[k] = ix[src];
          vv[k] = val[src];
        }
      }
      int kcs[kGalEpl];
#pragma unroll
      for (int k = 0; k < kGalEpl; ++k) {
        kcs[k] = 0;
        if (cidx[k] >= 0) {
          const int cj = cidx[k] / bs;
          kcs[k] = agg ? agg[cj] * bs + (cidx[k] - cj * bs) : cidx[k];
        }
      }
#pragma unroll
      for (int k = 0; k < kGalEpl; ++k) {
        const int e = w.lane + k * w.width;
        if (cidx[k] >= 0) {
          key[e] = ((unsigned long long)(unsigned)kcs[k] << 32) | (unsigned)e;
          v0[e] = vv[k];
        }
      }
    } else {
      for (int q = q0; q < q0 + nm; ++q) {
        const int64_t r = (int64_t)mem[q] * bs + a;
        const int p0 = ip[r], len = ip[r + 1] - p0;
        PFV_LANES(t, len) {
          const int cidx = ix[p0 + t];
          const int cj = cidx / bs;
          const unsigned long long kc = (unsigned long long)(unsigned)(agg ? agg[cj] * bs + (cidx - cj * bs) : cidx);
          key[m + t] = (kc << 32) | (unsigned)(m + t);
          v0[m + t] = val[p0 + t];
        }
        m += len;
      }
    }
    int P2 = 2;  // this row's own power of two
    while (P2 < m) P2 <<= 1;
    PFV_LANES(t, P2 - m) key[m + t] = ~0ull;
    PFV_LANES(i, P2 / 64 + 1) mask[i] = 0ull;
    w.sync();
    for (int k = 2; k <= P2; k <<= 1) {
      for (int j = k >> 1; j > 0; j >>= 1) {
        PFV_LANES(t, P2 >> 1) {
          const int lo = ((t & ~(j - 1)) << 1) | (t & (j - 1));
          const int hi = lo | j;
          const bool up = (lo & k) == 0;
          const unsigned long long x = key[lo], y = key[hi];
          if ((x > y) == up) {
            key[lo] = y;
            key[hi] = x;
          }
        }
        w.sync();
      }
    }
    PFV_LANES(e, m) {
      if (e == 0 || (key[e] >> 32) != (key[e - 1] >> 32)) atomic_or_u64(mask + (e >> 6), 1ull << (e & 63));
    }
    w.sync();
    int total = 0;
    for (int i = 0; i < m / 64 + 1; ++i) total += popcount64(mask[i]);
    const int64_t t0 = tptr[R];
    PFV_LANES(e, m) {
      const unsigned long long word = mask[e >> 6];
      if ((word >> (e & 63)) & 1ull) {
        int posn = popcount64(word & ((1ull << (e & 63)) - 1ull));
        for (int i = 0; i < (e >> 6); ++i) posn += popcount64(mask[i]);
        const unsigned long long kc = key[e] >> 32;
        double sum = v0[(unsigned)key[e]];
        for (int t = e + 1; t < m && (key[t] >> 32) == kc; ++t) sum += v0[(unsigned)key[t]];  // gather order
        tcol[t0 + posn] = (int32_t)kc;
        tval[t0 + posn] = sum;
        if ((int64_t)kc == R) dinv[R] = sum != 0.0 ? 1.0 / sum : 0.0;
      }
    }
    if (w.lane0()) cnt[R] = total;
    w.sync();
  });
  exclusive_scan<int32_t, int64_t>(s, c.scratch, cnt, cptr, (size_t)ncr);
  const int64_t nnz = known ? nnz_c : read_scalar<int64_t>(s, cptr + ncr);
  if (!known) amg_gal_record(sizes, ncr, annz, maxcap, nnz);
  if (nnz >= (int64_t(1) << 31)) throw Error(PFV_ERR_UNSUPPORTED, "AMG: coarse matrix with more than 2^31 entries");
  Ac.nrows = Ac.ncols = ncr;
  Ac.nnz = nnz;
  int32_t* cp = Ac.indptr.ensure(ncr + 1);
  int32_t* cx = Ac.indices.ensure(std::max<int64_t>(nnz, 1));
  double* cv = valc.ensure(std::max<int64_t>(nnz, 1));
  parallel_for(s, ncr + 1, PFV_LAMBDA(int64_t R) { cp[R] = (int32_t)cptr[R]; });
  wave_for<16>(s, ncr, 16, PFV_LAMBDA(const WaveCtx& w) {
    const int64_t R = w.item;
    const int64_t t0 = tptr[R], o = cptr[R];
    PFV_LANES(t, cnt[R]) {
      cx[o + t] = tcol[t0 + t];
      cv[o + t] = tval[t0 + t];
    }
  });
  Ac.max_row = maxcap;  // upper bound (saves a host read; nothing sizes itself by it)
}
static void amg_galerkin(pfv_ctx_impl& c, const AmgSwitches& sw, AmgWork& wk, const CsrPattern& A, const double* val,
                         int bs, const int32_t* agg, const int32_t* mptr, const int32_t* mem, int64_t nagg, CsrPattern& Ac,
                         Buf<double>& valc, Buf<double>& dinvc, Amg* sizes = nullptr) {
  amg_galerkin_csr(c, sw, wk, A.indptr, A.indices, A.nnz, val, bs, agg, mptr, mem, nagg, Ac, valc, dinvc, sizes);
}

static void amg_diag_inverse(pfv_ctx_impl& c, const CsrPattern& P, const double* val, double* dinv) {
  const int32_t* ip = P.indptr;
  const int32_t* ix = P.indices;
  parallel_for(c.stream, P.nrows, PFV_LAMBDA(int64_t r) {
    double d = 0.0;
    for (int e = ip[r]; e < ip[r + 1]; ++e)
      if (ix[e] == r) d += val[e];
    dinv[r] = d != 0.0 ? 1.0 / d : 0.0;
  });
}

static void amg_swap_pattern(CsrPattern& a, CsrPattern& b) {
  std::swap(a.nrows, b.nrows);
  std::swap(a.ncols, b.ncols);
  std::swap(a.nnz, b.nnz);
  std::swap(a.max_row, b.max_row);
  a.indptr.swap(b.indptr);
  a.indices.swap(b.indices);
}

// checksum of a pattern's index arrays (topology.inc: launch_pattern_checksum), read back: tells whether saved
// aggregate maps fit the matrix at hand.  The flow system's own pattern carries the one its symbolic phase left.
static unsigned long long amg_pattern_checksum(pfv_ctx_impl& c, AmgWork& wk, const CsrPattern& P) {
  if (&P == &c.pat_A && c.pat_A_checksum != 0 && c.have_symbolic) return c.pat_A_checksum;
  return read_scalar<unsigned long long>(c.stream, launch_pattern_checksum(c, wk.csum, P));
}

// diag: the diagonal of A if the caller has it (else it is extracted from the rows)
// Strength filter of the finest matrix: entries with |a_ij| < theta max_{k != i} |a_ik| are dropped and their
// values added to the diagonal (row sums -- what the operator does to constants -- are kept).  An MPFA system on
// tetrahedra carries ~67 entries per row (every cell sharing a NODE with the cell), most of them orders of magnitude
// below the face neighbours'; the pairwise matching only ever follows the strong ones, but the Galerkin products of
// the three passes sort and sum all of them (6.2 + 3 + 1.3 ms of the 20.8 ms setup at 2 M cells).  The hierarchy is
// coarsened from the filtered copy; level 0 of the cycle (smoothing, residual) keeps the full matrix, so the
// preconditioner stays a fixed linear operator close to A^-1 and the Krylov loop corrects the rest.
// strength of block kb of the cell of row r: the other rows of the cell hold the other diagonal entries of the block
struct AmgBlockStrength {
  const int32_t* ip;
  const double* val;
  int bs;
  PFV_HD double operator()(int64_t r, int kb) const {
    const int64_t i = r / bs;
    double sw = 0.0;
    for (int a = 0; a < bs; ++a) sw += fabs(val[ip[i * bs + a] + kb * bs + a]);
    return sw;
  }
};

#ifndef PFV_EMULATE
// Scalar systems on the device: the two passes of amg_filter with the loads of U chunks of a row in flight at once.
// The generic bodies below walk a row chunk by chunk, and each chunk is a chain column index -> row maximum of that
// column -> test; with ~70 entries per row that is five dependent round trips per 16-lane group and the passes ran at
// 1-2 TB/s.  Same arithmetic in the same order (per-lane sums over the chunks in order, lanes in order): same bits.
constexpr int kFilterUnroll = 5;

static void amg_filter_count_scalar(stream_t s, int64_t n, const int32_t* ip, const int32_t* ix, const double* val,
                                    const double* rmax, double theta, int32_t* cnt) {
  wave_for<16>(s, n, 16, PFV_LAMBDA(const WaveCtx& w) {
    const int64_t r = w.item;
    const int p0 = ip[r], nb = ip[r + 1] - p0;
    const double mi = rmax[r];
    int kept = 0;
    for (int c0 = 0; c0 < nb; c0 += kFilterUnroll * 16) {
      int cj[kFilterUnroll];
      double v[kFilterUnroll], rm[kFilterUnroll];
#pragma unroll
      for (int u = 0; u < kFilterUnroll; ++u) {
        const int kb = c0 + u * 16 + w.lane;
        const bool live = kb < nb;
        cj[u] = live ? ix[p0 + kb] : -1;
        v[u] = live ? val[p0 + kb] : 0.0;
      }
#pragma unroll
      for (int u = 0; u < kFilterUnroll; ++u) rm[u] = cj[u] >= 0 ? rmax[cj[u]] : 0.0;
#pragma unroll
      for (int u = 0; u < kFilterUnroll; ++u)
        if (cj[u] >= 0 && (cj[u] == (int32_t)r || fabs(v[u]) >= theta * fmin(mi, rm[u]))) ++kept;
    }
    kept += __shfl_xor(kept, 8, 16);
    kept += __shfl_xor(kept, 4, 16);
    kept += __shfl_xor(kept, 2, 16);
    kept += __shfl_xor(kept, 1, 16);
    if (w.lane0()) cnt[r] = kept;
  });
}

static void amg_filter_compact_scalar(stream_t s, int64_t n, const int32_t* ip, const int32_t* ix, const double* val,
                                      const double* rmax, double theta, const int32_t* fp, int32_t* fx, double* fv,
                                      double* dinv_out, bool spec, int32_t* bad) {
  wave_for<16>(s, n, 16 * sizeof(double) + 16, PFV_LAMBDA(const WaveCtx& w) {
    const int64_t r = w.item;
    double* lump = reinterpret_cast<double*>(w.lds);  // [16] per-lane sums of the dropped entries
    const int p0 = ip[r], nb = ip[r + 1] - p0;
    const double mi = rmax[r];
    double mylump = 0.0;
    int base = fp[r];
    const int room = fp[r + 1];
    int od = -1;       // position of the diagonal entry in the filtered row (on the lane that holds it)
    double dv = 0.0;
    const int sh = (int)threadIdx.x & 48;
    for (int c0 = 0; c0 < nb; c0 += kFilterUnroll * 16) {
      int cj[kFilterUnroll];
      double v[kFilterUnroll], rm[kFilterUnroll];
#pragma unroll
      for (int u = 0; u < kFilterUnroll; ++u) {
        const int kb = c0 + u * 16 + w.lane;
        const bool live = kb < nb;
        cj[u] = live ? ix[p0 + kb] : -1;
        v[u] = live ? val[p0 + kb] : 0.0;
      }
#pragma unroll
      for (int u = 0; u < kFilterUnroll; ++u) rm[u] = cj[u] >= 0 ? rmax[cj[u]] : 0.0;
#pragma unroll
      for (int u = 0; u < kFilterUnroll; ++u) {
        if (c0 + u * 16 >= nb) break;  // (uniform over the 16 lanes of the row)
        const bool live = cj[u] >= 0;
        const bool isdiag = cj[u] == (int32_t)r;
        bool keep = live && (isdiag || fabs(v[u]) >= theta * fmin(mi, rm[u]));
        if (live && !keep) mylump += v[u];
        const unsigned long long m = __ballot(keep);
        const unsigned m16 = (unsigned)((m >> sh) & 0xffffu);
        const int before = __popc(m16 & ((1u << w.lane) - 1u));
        const int total = __popc(m16);
        if (keep && spec && base + before + 1 > room) {  // the row keeps more than its old slot holds
          atomic_max_i32(bad, 1);
          keep = false;
        }
        if (keep) {
          const int o = base + before;
          fx[o] = cj[u];
          fv[o] = v[u];
          if (isdiag) { od = o; dv = v[u]; }
        }
        base += total;
      }
    }
    lump[w.lane] = mylump;
    w.lsync();
    if (spec && w.lane0() && base != room) atomic_max_i32(bad, 1);  // ... or fewer
    // the lane that holds the diagonal adds the dropped entries to it: per-lane sums in lane order (as the generic body)
    const unsigned long long has = __ballot(od >= 0);
    const bool any_diag = ((has >> sh) & 0xffffull) != 0ull;
    if (od >= 0) {
      double sum = 0.0;
      for (int l = 0; l < 16; ++l) sum += lump[l];
      const double d = dv + sum;
      fv[od] = d;
      if (dinv_out) dinv_out[r] = d != 0.0 ? 1.0 / d : 0.0;
    } else if (!any_diag && w.lane0() && dinv_out) {
      dinv_out[r] = 0.0;
    }
    w.lsync();
  });
}
#endif

static void amg_filter(pfv_ctx_impl& c, const AmgSwitches& sw, const CsrPattern& A, const double* val, double theta,
                       CsrPattern& F, Buf<double>& FV, AmgWork& wk, int bs = 1,
                       const std::function<void(double*)>& fill_halo = nullptr, const double* rmax_given = nullptr,
                       double* dinv_out = nullptr, bool same_layout_expected = false, bool* layout_unchanged = nullptr) {
  // Block systems (bs unknowns per cell, full bs x bs blocks): a block is kept or dropped as a whole by its strength
  // (sum of the absolute diagonal entries of the block, the measure of the matching), a dropped block is added to the
  // diagonal block of its row -- component by component, so that the action on rigid translations is kept.
  // The test is symmetric: (i, j) is dropped only if it is weak for BOTH ends, s_ij < theta min(max_k s_ik, max_k s_jk).
  // Measured against the largest entry of its own row alone, the coupling of a low-permeability cell to a
  // high-permeability neighbour is dropped from the neighbour's row while it stays the dominant entry of its own:
  // the filtered operator loses its connectivity one way, and on a log-normal field of contrast 1e7 the hierarchy
  // built from it diverged.
  stream_t s = c.stream;
  const int64_t n = A.nrows;
  const int32_t* ip = A.indptr;
  const int32_t* ix = A.indices;
  int32_t* cnt = wk.cnt.ensure(n + 1);
  int64_t* pos = wk.pos.ensure(n + 2);
  // largest off-diagonal block strength of every row's cell (coupled hierarchy: the rows of halo cells live on other
  // ranks -- fill_halo fetches their values, the test stays the symmetric one across a rank boundary)
  double* rmax = wk.tval.ensure(std::max<int64_t>(std::max(n, A.ncols), 1));
  constexpr int kMaxBs = 4;
  if (bs > kMaxBs) throw Error(PFV_ERR_UNSUPPORTED, "AMG filter: block size above 4");
  const AmgBlockStrength strength{ip, val, bs};
  // (scalar grid systems: assemble_system left the row maxima when it wrote the values -- same numbers, one pass less)
  const bool have_rmax = rmax_given != nullptr && bs == 1 && !fill_halo;
  if (have_rmax) be_d2d(rmax, rmax_given, sizeof(double) * (size_t)n, s);
  else
  wave_for<16>(s, n, 16 * sizeof(double) + 16, PFV_LAMBDA(const WaveCtx& w) {
    const int64_t r = w.item;
    const int64_t i = r / bs;
    double* mx = reinterpret_cast<double*>(w.lds);
    const int p0 = ip[r], nb = (ip[r + 1] - p0) / bs;
    double m = 0.0;
    PFV_LANES(kb, nb) {
      if (ix[p0 + kb * bs] / bs != (int32_t)i) m = fmax(m, strength(r, kb));
    }
    mx[w.lane] = m;
    w.lsync();
    if (w.lane0()) {
      double mm = 0.0;
      for (int l = 0; l < w.width; ++l) mm = fmax(mm, mx[l]);
      rmax[r] = mm;
    }
    w.lsync();
  });
  if (fill_halo) fill_halo(rmax);
  // same_layout_expected: F still holds the row pointers of the previous filtering of a matrix with THIS pattern (the
  // caller proved that by checksum).  Then the counting pass, the scan and the read of the total are skipped: the
  // compaction writes into the old layout, every row checks that it keeps exactly as many entries as its slot holds,
  // and one flag tells whether any row did not -- in which case the whole filter is redone the long way.
  const bool spec = same_layout_expected && F.nrows == n && F.ncols == A.ncols && F.nnz > 0 && F.indptr.p != nullptr;
  int32_t* bad = c.status.ensure(16) + 12;
  if (spec) be_memset(bad, 0, sizeof(int32_t), s);
#ifndef PFV_EMULATE
  const bool fast = bs == 1 && sw.filter_unroll;
#else
  const bool fast = false;
#endif
  if (!spec) {
#ifndef PFV_EMULATE
  if (fast) amg_filter_count_scalar(s, n, ip, ix, val, rmax, theta, cnt);
  else
#endif
  wave_for<16>(s, n, 16 * sizeof(int32_t) + 16, PFV_LAMBDA(const WaveCtx& w) {
    const int64_t r = w.item;
    const int64_t i = r / bs;
    int32_t* ct = reinterpret_cast<int32_t*>(w.lds);
    const int p0 = ip[r], nb = (ip[r + 1] - p0) / bs;
    const double mi = rmax[r];
    int kept = 0;
    PFV_LANES(kb, nb) {
      const int cj = ix[p0 + kb * bs] / bs;
      if (cj == (int32_t)i || strength(r, kb) >= theta * fmin(mi, rmax[(int64_t)cj * bs])) ++kept;
    }
#ifndef PFV_EMULATE
    // (sum over the 16 lanes of the row with row-local DPP-free shuffles: no LDS round trip)
    (void)ct;
    kept += __shfl_xor(kept, 8, 16);
    kept += __shfl_xor(kept, 4, 16);
    kept += __shfl_xor(kept, 2, 16);
    kept += __shfl_xor(kept, 1, 16);
    if (w.lane0()) cnt[r] = kept * bs;
#else
    ct[w.lane] = kept;
    w.lsync();
    if (w.lane0()) {
      int tot = 0;
      for (int l = 0; l < w.width; ++l) tot += ct[l];
      cnt[r] = tot * bs;
    }
    w.lsync();
#endif
  });
  exclusive_scan<int32_t, int64_t>(s, c.scratch, cnt, pos, (size_t)n);
  }
  // (counting path: does the layout equal the one F holds from the previous filtering?  Rides along with the read of
  // the total; tells the caller whether offering that layout next time is worth the try.)
  const bool compare = !spec && layout_unchanged != nullptr && F.nrows == n && F.nnz > 0 && F.indptr.p != nullptr;
  if (!spec) {
    be_memset(pos + n + 1, 0, sizeof(int64_t), s);
    if (compare) {
      const int32_t* old = F.indptr.p;
      parallel_for(s, n, PFV_LAMBDA(int64_t r) {
        if (old[r + 1] - old[r] != cnt[r]) pos[n + 1] = 1;  // (benign race: every writer stores the same value)
      });
    }
  }
  int64_t tail[2] = {F.nnz, 0};
  if (!spec) be_d2h(tail, pos + n, 2 * sizeof(int64_t), s);
  if (layout_unchanged) *layout_unchanged = spec || (compare && tail[1] == 0 && tail[0] == F.nnz);
  const int64_t nnz = tail[0];
  F.nrows = n;
  F.ncols = A.ncols;
  F.nnz = nnz;
  F.max_row = A.max_row;
  int32_t* fp = F.indptr.ensure(n + 1);
  int32_t* fx = F.indices.ensure(std::max<int64_t>(nnz, 1));
  double* fv = FV.ensure(std::max<int64_t>(nnz, 1));
  if (!spec) parallel_for(s, n + 1, PFV_LAMBDA(int64_t q) { fp[q] = (int32_t)pos[q]; });
  // 16 lanes per row, blocks in chunks of 16: order-preserving compaction (position = kept blocks before it: the
  // flags of a chunk go through LDS), the dropped values summed per lane and then in lane order (deterministic).
  // (A thread per row walking its ~67 entries twice ran 10 ms at 2 M rows: uncoalesced.)
#ifndef PFV_EMULATE
  if (fast) amg_filter_compact_scalar(s, n, ip, ix, val, rmax, theta, fp, fx, fv, dinv_out, spec, bad);
  else
#endif
  wave_for<16>(s, n, (16 + 1) * kMaxBs * sizeof(double) + 20 * sizeof(int32_t) + 16, PFV_LAMBDA(const WaveCtx& w) {
    const int64_t r = w.item;
    const int64_t i = r / bs;
    double* lump = reinterpret_cast<double*>(w.lds);        // [16][bs] per-lane sums, [16 * kMaxBs ..][bs] the diagonal block row
    double* dblk = lump + 16 * kMaxBs;
    int32_t* flag = reinterpret_cast<int32_t*>(dblk + kMaxBs);  // [16] kept flags of the chunk, [16] position of the diagonal block
    const int p0 = ip[r], nb = (ip[r + 1] - p0) / bs;
    const double mi = rmax[r];
    if (w.lane0()) flag[16] = -1;
    w.lsync();
    double mylump[kMaxBs];
    for (int b = 0; b < kMaxBs; ++b) mylump[b] = 0.0;
    int base = fp[r];
    for (int c0 = 0; c0 < nb; c0 += w.width) {
      const int kb = c0 + w.lane;
      bool keep = false;
      const bool live = kb < nb;
      bool isdiag = false;
      if (live) {
        const int cj = ix[p0 + kb * bs] / bs;
        isdiag = cj == (int32_t)i;
        keep = isdiag || strength(r, kb) >= theta * fmin(mi, rmax[(int64_t)cj * bs]);
        if (!keep)
          for (int b = 0; b < bs; ++b) mylump[b] += val[p0 + kb * bs + b];
      }
      int before = 0, total = 0;
#ifndef PFV_EMULATE
      {  // the kept flags of the row's 16 lanes: one ballot, two popcounts (the lanes of a row run their loop together)
        const unsigned long long m = __ballot(keep);
        const unsigned m16 = (unsigned)((m >> (((int)threadIdx.x & 48))) & 0xffffu);
        before = __popc(m16 & ((1u << w.lane) - 1u));
        total = __popc(m16);
      }
#else
      flag[w.lane] = keep ? 1 : 0;
      w.lsync();
      for (int l = 0; l < w.width; ++l) {
        const int fl = flag[l];
        if (l < w.lane) before += fl;
        total += fl;
      }
#endif
      if (keep && spec && base + (before + 1) * bs > fp[r + 1]) {  // the row keeps more than its old slot holds
        atomic_max_i32(bad, 1);
        keep = false;
      }
      if (keep) {
        const int o = base + before * bs;
        for (int b = 0; b < bs; ++b) {
          fx[o + b] = ix[p0 + kb * bs + b];
          fv[o + b] = val[p0 + kb * bs + b];
        }
        if (isdiag) {
          flag[16] = o;
          for (int b = 0; b < bs; ++b) dblk[b] = val[p0 + kb * bs + b];
        }
      }
      base += total * bs;
      w.lsync();
    }
    for (int b = 0; b < bs; ++b) lump[w.lane * kMaxBs + b] = mylump[b];
    w.lsync();
    if (spec && w.lane0() && base != fp[r + 1]) atomic_max_i32(bad, 1);  // ... or fewer
    if (w.lane0()) {
      const int od = flag[16];
      if (od >= 0) {
        for (int b = 0; b < bs; ++b) {
          double sum = 0.0;
          for (int l = 0; l < w.width; ++l) sum += lump[l * kMaxBs + b];
          const double dv = dblk[b] + sum;  // (the diagonal block came through LDS: no global read-after-write across lanes)
          fv[od + b] = dv;
          // the inverse diagonal of the filtered matrix rides along (what amg_diag_inverse would compute in a pass of its own)
          if (dinv_out && b == (int)(r - i * bs)) dinv_out[r] = dv != 0.0 ? 1.0 / dv : 0.0;
        }
      } else if (dinv_out) {
        dinv_out[r] = 0.0;
      }
    }
    w.lsync();
  });
  c.stats.amg_filter_layout = spec ? 1 : 0;
  if (spec && read_scalar<int32_t>(s, bad) != 0) {
    amg_filter(c, sw, A, val, theta, F, FV, wk, bs, fill_halo, rmax_given, dinv_out, false, nullptr);
    c.stats.amg_filter_layout = 2;
    if (layout_unchanged) *layout_unchanged = false;
  }
}

static void amg_estimate_omegas(pfv_ctx_impl& c, Amg& amg);
static void amg_build_ap(pfv_ctx_impl& c, Amg& amg, bool want64);
static void amg_spmv(pfv_ctx_impl& c, const Amg& amg, const AmgLevel& L, const double* x, double* y,
                     const double* smooth_b);
static double* amg_cycle(pfv_ctx_impl& c, Amg& amg, size_t l, const double* b, double* x, bool x_is_presmoothed = false,
                         int visit = 0);
static void amg_setup(pfv_ctx_impl& c, Amg& amg, const CsrPattern& A, const double* val, int bs,
                      const double* diag = nullptr, const WinCsr* win0 = nullptr);
static void amg_restrict(pfv_ctx_impl& c, const Amg& amg, const AmgLevel& L, const AmgLevel& Ln, const double* b,
                         const double* t, bool next_smooths);

// Row-wise safeguard of the Jacobi smoother (PFV_AMG_SAFE_ROWS, default on): with r_i = sum_{j != i} |a_ij| / |a_ii| the
// Gershgorin disc of row i of D^-1 A reaches 1 + r_i.  M-matrix rows have r_i <= 1 (rho <= 2: every omega < 1 damps);
// MPFA rows on simplices carry positive off-diagonal entries and r_i up to ~2, which is what makes a fitted global omega
// a cliff (0.8 -> 23 iterations, 0.9 -> 3455 on the 2 M-cell system).  Rows with r_i > 1 get the diagonal
// a_ii (1 + r_i) / 2 in the smoother: all discs then end at 2, the smoother is stable for every omega <= 1 on every
// matrix, and M-matrix rows are untouched.
static void amg_safeguard_rows(pfv_ctx_impl& c, const CsrPattern& P, const double* val, double* dinv) {
  const int32_t* ip = P.indptr;
  const int32_t* ix = P.indices;
  wave_for<16>(c.stream, P.nrows, 16 * sizeof(double) + 16, PFV_LAMBDA(const WaveCtx& w) {
    const int64_t r = w.item;
    double* sh = reinterpret_cast<double*>(w.lds);
    const int p0 = ip[r], len = ip[r + 1] - p0;
    double off = 0.0;
    PFV_LANES(k, len) {
      if (ix[p0 + k] != (int32_t)r) off += fabs(val[p0 + k]);
    }
    sh[w.lane] = off;
    w.lsync();
    if (w.lane0()) {
      double sum = 0.0;
      for (int l = 0; l < w.width; ++l) sum += sh[l];
      const double di = dinv[r];
      const double ri = sum * fabs(di);  // sum |a_ij| / |a_ii|
      if (ri > 1.0 && ri < 1.0e300) dinv[r] = di * 2.0 / (1.0 + ri);
    }
    w.lsync();
  });
}

#include "amg_dist.inc"

// Explicit inverse of a small matrix (the coarsest level, at most kAmgDenseMax rows) into `dense` (row-major n x n);
// false when a pivot vanished (the caller then falls back to smoothing sweeps)
static bool amg_dense_invert(pfv_ctx_impl& c, const AmgSwitches& sw, AmgWork& wk, const CsrPattern& P, const double* v,
                             Buf<double>& dense) {
  stream_t s = c.stream;
  const int n = (int)P.nrows, ld = n | 1;
  double* D = wk.dense_work.ensure((size_t)n * ld + 3 * (size_t)n);
  double* rsc = D + (size_t)n * ld + 2 * (size_t)n;  // row scales
  int32_t* ipiv = wk.piv.ensure(n + 4);
  const int32_t* ip = P.indptr;
  const int32_t* ix = P.indices;
  be_memset(D, 0, sizeof(double) * ((size_t)n * ld + 3 * (size_t)n), s);
  // rows scaled to unit 1-norm before the inversion, (S D)^-1 S = D^-1: the pivot test of node_gj_lds is an
  // absolute one made for such rows -- on the raw Galerkin matrix of a system in SI units (entries ~1e-15) every
  // pivot counted as singular and the level silently fell back to Jacobi sweeps (solver behaviour depended on
  // the units of the matrix)
  parallel_for(s, n, PFV_LAMBDA(int64_t r) {
    double sum = 0.0;
    for (int e = ip[r]; e < ip[r + 1]; ++e) sum += fabs(v[e]);
    const double sc = (sum > 0.0 && sum < 1.0e300) ? 1.0 / sum : 1.0;
    rsc[r] = sc;
    for (int e = ip[r]; e < ip[r + 1]; ++e) D[(size_t)r * ld + ix[e]] += v[e] * sc;
  });
  int32_t* st = c.status.ensure(16);
  be_memset(st, 0, sizeof(int32_t), s);
  // one workgroup on a matrix in global memory: every pivot step is a round of dependent accesses -- 1024 threads
  // keep four times the loads of 256 in flight (the strength filter leaves coarsest levels of ~500 rows: 1.6 ms)
  auto invert = PFV_LAMBDA(const WaveCtx& w) {
    NodeLds G;
    G.A = D;
    G.rowk = D + (size_t)n * ld;
    G.colk = G.rowk + n;
    G.ipiv = ipiv;
    node_gj_lds(w, G, n, ld, 0, st);
  };
  // the matrix staged in LDS when it fits (n <= ~136: 143 KB of the 160): a pivot step is then a few LDS round trips
  // instead of a chain of dependent global accesses -- the 132-row coarsest level of the 2 M-cell system took 1.2 ms
  // per step in global memory, a tenth of the whole step at 200 k cells
  const size_t lds_need = sizeof(double) * ((size_t)n * ld + 2 * (size_t)n) + 64;
  auto invert_lds = PFV_LAMBDA(const WaveCtx& w) {
    double* A = reinterpret_cast<double*>(w.lds);
    PFV_LANES(q, n * ld) A[q] = D[q];
    w.sync();
    NodeLds G;
    G.A = A;
    G.rowk = A + (size_t)n * ld;
    G.colk = G.rowk + n;
    G.ipiv = ipiv;
    node_gj_lds(w, G, n, ld, 0, st);
    w.sync();
    PFV_LANES(q, n * ld) D[q] = A[q];
    w.sync();
  };
  if (lds_need <= 150 * 1024 && sw.dense_lds) {
    if (n > 128) block_for<1024>(s, 1, lds_need, invert_lds);
    else block_for<256>(s, 1, lds_need, invert_lds);
  } else if (n > 128) block_for<1024>(s, 1, 0, invert);
  else block_for<256>(s, 1, 0, invert);
  if (read_scalar<int32_t>(s, st) == 0) {
    double* inv = dense.ensure((size_t)n * n);
    parallel_for(s, (int64_t)n * n, PFV_LAMBDA(int64_t q) {
      const int64_t r = q / n, cc = q - r * n;
      inv[q] = D[(size_t)r * ld + cc] * rsc[cc];
    });
    return true;
  }
  return false;
}

// x = inv b with the explicit inverse of amg_dense_invert (one wavefront per row, lane sums in lane order)
static void amg_dense_apply(pfv_ctx_impl& c, const double* inv, int64_t n, const double* b, double* x) {
  wave_for(c.stream, n, 64 * sizeof(double) + 16, PFV_LAMBDA(const WaveCtx& w) {
    double* sh = reinterpret_cast<double*>(w.lds);
    const int64_t r = w.item;
    double a = 0.0;
    PFV_LANES(j, (int)n) a += inv[r * n + j] * b[j];
    sh[w.lane] = a;
    w.sync();
    if (w.lane0()) {
      double sum = 0.0;
      for (int j = 0; j < w.width; ++j) sum += sh[j];
      x[r] = sum;
    }
    w.sync();
  });
}

// ---- the setup, phase by phase (amg_setup at the end reads top to bottom)

static AmgLevel& amg_level(Amg& amg, size_t l) {  // level objects persist for their buffers
  while (amg.lev.size() <= l) amg.lev.push_back(std::make_unique<AmgLevel>());
  return *amg.lev[l];
}

// Values-only re-setup: when the matrix has the pattern the last hierarchy was built for (same
// symbolic phase, same sizes, same checksum of the index arrays, same parameters) the aggregates
// are kept and only the Galerkin products are redone -- the matching passes, a third of the setup,
// are skipped.  Aggregates follow the strength of connection of the values they were built from:
// right for the successive matrices of a nonlinear iteration; PFV_AMG_REUSE=0 always re-matches.
// Returns the decision; csum: checksum of A's index arrays (0: not taken).
// Coupled hierarchy: kept when the pattern of EVERY rank's rows is proved equal to the one its maps were built for.
// This rank's answer goes through the gather of amg_dist_vote -- all ranks take the same branch, the exchanges of the
// setup stay matched (what made the sharded path on one rank 12 instead of 6 ms of setup).  `maps_cfg == cfg` is part
// of what every rank votes on: a rank-local difference can then only turn the common decision to "re-match", never
// send ranks down different branches of the setup's collectives.
static bool amg_decide_reuse(pfv_ctx_impl& c, Amg& amg, const CsrPattern& A, unsigned long long& csum) {
  const AmgSwitches& w = amg.sw;
  AmgDist* D = amg.dist.get();
  csum = 0;
  bool mine = false;
  if (w.reuse && (!D || w.reuse_dist)) {
    csum = amg_pattern_checksum(c, amg.wk, A);
    mine = amg.maps_ok && amg.maps_n == A.nrows && amg.maps_nnz == A.nnz && amg.maps_cfg == amg_maps_cfg(w) &&
           amg.maps_sum == csum &&
           // a re-built symbolic phase only invalidates the maps if its pattern differs: equal sizes, parameters and
           // checksum of the index arrays prove the pattern equal (PFV_AMG_REUSE_REBUILT=0: the epoch must match too)
           (amg.maps_epoch == c.symbolic_epoch || w.reuse_rebuilt) &&
           (!D || (A.nrows >= w.reuse_dist_min_rows && amg.maps_tag == amg_maps_tag(w)));
  }
  return D ? amg_dist_vote(c, *D, A.nrows, mine) : mine;
}

// full bs x bs blocks are assumed (true for div_nd @ stress); verify the row lengths at least
static void amg_check_full_blocks(pfv_ctx_impl& c, const CsrPattern& A, int bs) {
  stream_t s = c.stream;
  const int32_t* ip = A.indptr;
  int32_t* st = c.status.ensure(16);
  be_memset(st + 10, 0, sizeof(int32_t), s);
  parallel_for(s, A.nrows / bs, PFV_LAMBDA(int64_t i) {
    const int len = ip[i * bs + 1] - ip[i * bs];
    bool bad = (len % bs) != 0;
    for (int a = 1; a < bs; ++a) bad = bad || (ip[i * bs + a + 1] - ip[i * bs + a]) != len;
    if (bad) atomic_max_i32(st + 10, 1);
  });
  if (read_scalar<int32_t>(s, st + 10))
    throw Error(PFV_ERR_UNSUPPORTED, "AMG: the matrix is not made of full blocks of the given block size");
}

// Level 0: the system itself or, with the filter on (PFV_AMG_FILTER_SMOOTH), its strength-filtered copy with the kept
// layout and SpMV window; the inverse diagonal.  Returns the checksum of the finest pattern the hierarchy is coarsened
// from (0: unknown).
static unsigned long long amg_setup_level0(pfv_ctx_impl& c, Amg& amg, const CsrPattern& A, const double* val,
                                           const double* diag, const WinCsr* win0, unsigned long long csum) {
  stream_t s = c.stream;
  const AmgSwitches& w = amg.sw;
  AmgDist* D = amg.dist.get();
  const int bs = amg.bs;
  AmgLevel& L0 = amg_level(amg, 0);
  L0.n = A.nrows;
  L0.m = std::max(A.ncols, A.nrows);
  L0.P = &A;
  L0.val = val;
  L0.win = win0;
  amg.filt_nnz = 0;
  // PFV_AMG_FILTER_SMOOTH (with the filter on): the WHOLE cycle, its finest level included, works on the filtered
  // operator -- the smoothing and residual products of level 0 then stream a third of the entries (they are the
  // largest kernel of the step), the Krylov loop keeps the full matrix.  M ~ A_s^-1 with A_s spectrally close to A.
  amg.filter_level0 = amg.filter_theta > 0.0 && w.filter_smooth;
  if (!amg.filter_level0) {  // (coarse levels get dinv from the Galerkin kernel, the filtered finest level from the filter)
    double* dv = L0.dinv.ensure(L0.n);
    if (diag) {
      parallel_for(s, L0.n, PFV_LAMBDA(int64_t i) { dv[i] = diag[i] != 0.0 ? 1.0 / diag[i] : 0.0; });
    } else {
      amg_diag_inverse(c, A, val, dv);
    }
    return csum;
  }
  const double* rmax_given = (c.sys_rowmax_for == val && A.nrows == c.nc && w.rowmax_reuse) ? c.sys_rowmax.p : nullptr;
  // (layout of the filtered rows kept from the previous setup when A's pattern is the one it was computed for)
  // -- offered only after a filtering that REPRODUCED the layout before it (coefficients that do not change
  // between setups: a linear problem stepped in time, repeated solves); values that move every time never pay
  // for a failed try more than once
  const bool same_pattern = !D && csum != 0 && amg.filt_layout_for == csum;
  const bool same_layout = same_pattern && amg.filt_layout_stable && w.filter_layout_reuse;
  if (!same_pattern) amg.filtP.nrows = 0;  // (nothing to compare the new layout with)
  bool unchanged = false;
  // (the diagonal of the filtered matrix carries the lumped entries: dinv comes from the filter, not from `diag`)
  amg_filter(c, w, A, val, amg.filter_theta, amg.filtP, amg.filtV, amg.wk, bs, amg_fill_halo0(c, D, bs), rmax_given,
             L0.dinv.ensure(L0.n), same_layout, &unchanged);
  amg.filt_layout_stable = unchanged;
  amg.filt_layout_for = D ? 0ull : csum;
  amg.filt_nnz = amg.filtP.nnz;
  L0.P = &amg.filtP;
  L0.val = amg.filtV.p;
  L0.win = nullptr;
  if (amg.filtP.nnz < 200000) return 0ull;
  // the windows are a function of the filtered PATTERN: kept when it is the one they were built for (which
  // entries survive the filter depends on the values, so this is checked on the filtered index arrays themselves)
  // (a local structure: every rank decides for itself, also under the coupled hierarchy)
  // (not asked when this filtering has just been seen to differ from the previous one on the same pattern of A --
  // values that move: the digest, three passes over the filtered indices and a read-back, could only say "no")
  const bool moved = same_pattern && !unchanged && w.skip_moved_digest;
  const unsigned long long fsum = (env_int("PFV_WIN_REUSE", 1) != 0 && !moved)
                                      ? read_scalar<unsigned long long>(s, launch_pattern_checksum(c, amg.wk.csum, amg.filtP))
                                      : 0ull;
  // (PFV_SPMV_WINDOW=0 switches a kept window off too, not only the building of a new one)
  const bool keep = fsum != 0 && amg.filt_win.ok && amg.filt_win_sum == fsum && amg.filt_win.nrows == amg.filtP.nrows &&
                    amg.filt_win.nnz == amg.filtP.nnz && env_int("PFV_SPMV_WINDOW", 1) != 0;
  if (!keep) {
    // (the filtered rows are subsets of A's rows: their windows come out of A's windows without hashing or
    // sorting -- spmv_win.inc: win_derive; from scratch where A has none)
    if (!(win0 && win_derive(c, amg.filtP, *win0, amg.filt_win))) win_build(c, amg.filtP, amg.filt_win);
    amg.filt_win_sum = amg.filt_win.ok ? fsum : 0ull;
  }
  L0.win = &amg.filt_win;
  return fsum;
}

// cycle vectors and the single-precision copy of the values of level l
static void amg_level_buffers(pfv_ctx_impl& c, const Amg& amg, AmgLevel& L, size_t l) {
  if (l > 0) {
    L.x.ensure(L.m);
    L.b.ensure(L.n);
  }
  L.t.ensure(L.m);
  L.v32 = nullptr;
  if (amg.fp32) {
    float* v32 = L.val32.ensure(L.P->nnz);
    const double* v64 = L.val;
    parallel_for(c.stream, L.P->nnz, PFV_LAMBDA(int64_t e) { v32[e] = (float)v64[e]; });
    L.v32 = v32;
  }
  L.nc_cells = 0;
}

// Coarsening of level l: several pairwise passes, composing the aggregate maps (L.agg, member lists, L.nc_cells); the
// intermediate Galerkin matrices ping-pong between the two slots of the workspace.  Returns the slot that holds the
// matrix of level l + 1, or -1 when the coarsening stalled (this level is then the coarsest).
static int amg_coarsen_level(pfv_ctx_impl& c, Amg& amg, size_t l, bool reuse) {
  stream_t s = c.stream;
  const AmgSwitches& w = amg.sw;
  AmgWork& wk = amg.wk;
  AmgDist* D = amg.dist.get();
  const int bs = amg.bs;
  AmgLevel& L = *amg.lev[l];
  const int64_t cells = L.n / bs;
  const CsrPattern* curP = L.P;
  const double* curV = L.val;
  if (l == 0 && amg.filter_theta > 0.0 && !amg.filter_level0) {  // the filter for the matching only
    amg_filter(c, w, *L.P, L.val, amg.filter_theta, amg.filtP, amg.filtV, wk, bs, amg_fill_halo0(c, D, bs));
    amg.filt_nnz = amg.filtP.nnz;
    curP = &amg.filtP;
    curV = amg.filtV.p;
  }
  int32_t* aggL = L.agg.ensure(cells);
  int64_t cur_cells = cells;
  int slot = -1;
  // Below the finest level a deep hierarchy coarsens more gently (aggregates of 4 instead of 8): one
  // level more, but 15 instead of 18 BiCGStab iterations on the 2 M-cell system (step 100.6 -> 96 ms);
  // hierarchies of small systems (4 levels or fewer) gain nothing and keep the faster coarsening.
  // (coupled hierarchy: the size that counts is the one of the whole system, and the replicated part below the
  // gathered level continues the parent's policy -- its own level 0 is a coarse level)
  const int64_t finest_cells = amg.finest_cells_parent > 0 ? amg.finest_cells_parent
                                                            : (D ? D->global_rows0 : amg.lev[0]->n) / bs;
  const int coarse_default = finest_cells >= kAmgGentleCells ? std::min(2, amg.passes) : amg.passes;
  const int passes_here = (l == 0 && amg.finest_cells_parent <= 0)
                              ? amg.passes
                              : std::max(1, std::min(6, w.passes_coarse_set ? w.passes_coarse_raw : coarse_default));
  if (!reuse) L.pmap_count = 0;
  if (!reuse) L.members_kept = false;
  // (the member lists of a kept map are kept with it: a sort of cur_cells pairs per pass otherwise -- with the
  // composed map and the level's own member lists below 1.3 ms of kernels and ~200 launches of a setup on kept maps)
  const bool members_reuse = reuse && L.members_kept && w.members_reuse;
  // Level 0 on kept maps and member lists: nothing reads the intermediate matrices of the passes (the matching that
  // would is skipped), and the last product is P^T A_s P = P^T (A_s P) with P the composed map -- and AP = A_s P is
  // built for the cycle anyway (amg_build_ap), its columns coarse unknowns already, sorted and summed per aggregate.
  // So level 1 is ONE product over AP (its double-precision sums, ap_val64) with the member lists of the composed map,
  // instead of three over A_s and its pair matrices: a coarse row gathers ~72 entries instead of ~166 at 2 M
  // tetrahedra.  Same pattern as the pass route; values differ by the order of the additions.  The entries of AP are
  // known on the device only: the scratch of the product is sized by nnz(A_s).
  if (l == 0 && !D && members_reuse && L.pmap_count > 0 && w.galerkin_ap && curP == L.P && curV == L.val &&
      !(L.pmap_n[L.pmap_count - 1] > 0.85 * cells)) {
    const int64_t nc = L.pmap_n[L.pmap_count - 1];
    L.nc_cells = nc;
    amg_build_ap(c, amg, true);
    if (amg.ap_ok && amg.ap64_ok) {
      amg_gal_route(amg, 1);
      amg_galerkin_csr(c, w, wk, amg.ap_ptr, amg.ap_col, L.P->nnz, amg.ap_val64, bs, nullptr, L.mptr, L.mem, nc, wk.P[0],
                       wk.V[0], wk.D[0], &amg);
      amg.galerkin_ap = true;
      return 0;
    }
    L.nc_cells = 0;  // (AP not built, or without its double sums: the passes)
  }
  if (l == 0 && !D) amg_gal_route(amg, 0);
  for (int pass = 0; pass < (reuse ? L.pmap_count : passes_here); ++pass) {
    int64_t nagg;
    if (reuse) {
      nagg = L.pmap_n[pass];
    } else {
      nagg = amg_pairwise(c, w, wk, *curP, curV, bs, wk.a1);
      if (nagg >= cur_cells) break;  // nothing left to merge
      be_d2d(L.pmap[pass].ensure(cur_cells), wk.a1.p, sizeof(int32_t) * (size_t)cur_cells, s);
      L.pmap_n[pass] = nagg;
      L.pmap_count = pass + 1;
    }
    const int32_t* a1p = L.pmap[pass].p;
    if (!members_reuse) amg_members(c, wk, a1p, cur_cells, nagg, L.pmp[pass], L.pme[pass]);
    const int nslot = slot < 0 ? 0 : 1 - slot;
    const int32_t* amap = D ? amg_dist_extend_map(c, *D, l, a1p, cur_cells, nagg) : a1p;
    amg_galerkin(c, w, wk, *curP, curV, bs, amap, L.pmp[pass], L.pme[pass], nagg, wk.P[nslot], wk.V[nslot], wk.D[nslot],
                 D ? nullptr : &amg);
    if (D) wk.P[nslot].ncols = (nagg + D->plan[l]->n_halo) * bs;
    if (members_reuse) {
      // (aggL holds the composition of the kept maps already)
    } else if (slot < 0) {
      parallel_for(s, cells, PFV_LAMBDA(int64_t i) { aggL[i] = a1p[i]; });
    } else {
      parallel_for(s, cells, PFV_LAMBDA(int64_t i) { aggL[i] = a1p[aggL[i]]; });
    }
    slot = nslot;
    curP = &wk.P[slot];
    curV = wk.V[slot].p;
    cur_cells = nagg;
    if (nagg * bs <= w.coarse_target) break;
  }
  if (D && slot < 0) {
    amg_dist_identity_level(c, amg, *D, l, *curP, curV, aggL, cells);
    slot = 0;
  }
  if (!D && (slot < 0 || cur_cells > 0.85 * cells)) return -1;
  L.nc_cells = cur_cells;
  if (!(members_reuse && L.pmap_count > 0)) amg_members(c, wk, aggL, cells, cur_cells, L.mptr, L.mem);
  L.members_kept = L.pmap_count > 0;
  return slot;
}

// AP = A_s P of level 0, for the post-smoothing step of the cycle (amg_post_ap): with x0 the pre-smoothed iterate and
// t = A_s x0 still in memory, A_s (x0 + alpha P xs) = t + alpha (A_s P) xs -- the second sweep over A_s becomes a sweep
// over AP, whose row r holds one entry per distinct aggregate among the columns of row r of A_s.
// Values: the single-precision values the cycle's products read, summed per aggregate in double in entry order (a sum
// of a few dozen floats is exact in double), so the operator differs from the two-launch form by the order of double
// additions only.  Deterministic: keys ranked, every run summed in entry order, columns ascending.
// Two kernels and a scan, no host read: rows are formed in the slots [fp[r], fp[r + 1]) of the Galerkin scratch (a row
// of AP is never longer than its row of A_s; the scratch has that size since the first product of this level), their
// lengths are scanned, and the rows are packed -- the slots use a third of their lines' bytes, and the post-smoothing
// kernel, which runs twice per Krylov iteration, would fetch them all.
// Scalar, non-distributed hierarchies with a single-precision copy whose level 0 takes the two-launch restriction.
// A failed allocation leaves the cycle on its two-launch form.
constexpr int kApKeys = 128;  // entries of a row ranked in LDS (longer rows: one lane inserts them one by one)
constexpr int kApChunk = 8;   // ... entries per unrolled trip of the ranking loops
// want64: also ap_val64, the sums of the DOUBLE values of A_s over the same runs in the same entry order, ranked and
// packed by the same two kernels -- the input of the Galerkin product that forms level 1 from AP (amg_coarsen_level).
// Its rows are formed in a buffer of their own (the value slots of the passes change hands with the levels' matrices:
// one of them grown to nnz(A_s) here would be allocated anew by every setup).  When the storage cannot be had, AP is
// built for the cycle alone (ap64_ok stays false: the passes form level 1).
static void amg_build_ap(pfv_ctx_impl& c, Amg& amg, bool want64) {
  stream_t s = c.stream;
  amg.ap_ok = amg.ap64_ok = false;
  amg.ap_nnz = 0;
  AmgLevel& L = *amg.lev[0];
  if (!amg.sw.post_ap || amg.bs != 1 || amg.dist || amg.no_filter || amg.finest_cells_parent > 0 || !L.v32 ||
      L.nc_cells <= 0 || L.n != L.m || (L.n <= amg.fuse_rows && !(L.win && L.win->ok)))
    return;
  const int64_t n = L.n, fnnz = L.P->nnz;
  int32_t *sx, *al, *cp, *cx;
  int64_t* pos;
  double *sv, *cv, *sv64 = nullptr, *cv64 = nullptr;
  try {
    sx = amg.wk.tcol.ensure(std::max<int64_t>(fnnz, 1));
    sv = amg.wk.tval.ensure(std::max<int64_t>(fnnz, 1));
    al = amg.ap_len.ensure(n + 1);
    pos = amg.ap_pos.ensure(n + 1);
    cp = amg.ap_ptr.ensure(n + 1);
    cx = amg.ap_col.ensure(std::max<int64_t>(fnnz, 1));
    cv = amg.ap_val.ensure(std::max<int64_t>(fnnz, 1));
  } catch (const Error&) {
#ifndef PFV_EMULATE
    (void)hipGetLastError();  // (the failed allocation is not an error of the launches that follow)
#endif
    amg.ap_col.release();
    amg.ap_val.release();
    amg.ap_val64.release();
    amg.ap_row64.release();
    return;
  }
  if (want64) {
    try {
      sv64 = amg.ap_row64.ensure(std::max<int64_t>(fnnz, 1));
      cv64 = amg.ap_val64.ensure(std::max<int64_t>(fnnz, 1));
    } catch (const Error&) {
#ifndef PFV_EMULATE
      (void)hipGetLastError();
#endif
      amg.ap_val64.release();
      amg.ap_row64.release();
      want64 = false;
    }
  }
  const int32_t* fp = L.P->indptr;
  const int32_t* ix = L.P->indices;
  const float* v32 = L.v32;
  const double* v64 = L.val;
  const int32_t* agg = L.agg;
  auto rank_rows = PFV_LAMBDA(const WaveCtx& w, auto with64) {
    constexpr bool W64 = decltype(with64)::value;
    const int64_t r = w.item;
    const int p0 = fp[r], len = fp[r + 1] - p0;
    if (len > kApKeys) {
      if (w.lane0()) {  // sorted insertion, sums in entry order
        int cnt = 0;
        for (int e = 0; e < len; ++e) {
          const int32_t k = agg[ix[p0 + e]];
          const double v = (double)v32[p0 + e];
          const double vd = W64 ? v64[p0 + e] : 0.0;
          int q = 0;
          while (q < cnt && sx[p0 + q] < k) ++q;
          if (q < cnt && sx[p0 + q] == k) {
            sv[p0 + q] += v;
            if constexpr (W64) sv64[p0 + q] += vd;
          } else {
            for (int m = cnt; m > q; --m) {
              sx[p0 + m] = sx[p0 + m - 1];
              sv[p0 + m] = sv[p0 + m - 1];
              if constexpr (W64) sv64[p0 + m] = sv64[p0 + m - 1];
            }
            sx[p0 + q] = k;
            sv[p0 + q] = 0.0 + v;
            if constexpr (W64) sv64[p0 + q] = 0.0 + vd;
            ++cnt;
          }
        }
        al[r] = cnt;
      }
      return;
    }
    // What the kernel is bound by is the instructions of its comparisons, so it makes as few as it can.  Only the FIRST
    // entry of every aggregate is ranked and summed (~8 of the 18 entries of a row on tetrahedra): a first pass marks
    // them in a bit mask (entry e against the entries before it), they are compacted by the population counts of the
    // mask, and the ranking loop runs over the compacted list -- one trip of the lane group where the whole row took two.
    // (The loops over the row run in chunks of kApChunk without early exits: the LDS reads of a chunk are in flight
    // together -- entry by entry with a break, every read waited for the one before it.  An entry that is not the
    // first of its aggregate carries bit 31, which takes it out of "first entries with a smaller key" by the unsigned
    // comparison alone, and kApChunk sentinels of all ones behind the row need no test of the bounds.)
    unsigned long long* mask = reinterpret_cast<unsigned long long*>(w.lds);  // [2] bit e: entry e is the first of its aggregate
    uint32_t* kh = reinterpret_cast<uint32_t*>(mask + 2);                 // [kApKeys + kApChunk] aggregate of every entry | bit 31
    int32_t* fst = reinterpret_cast<int32_t*>(kh + kApKeys + kApChunk);   // [kApKeys] the first entries, in entry order
    float* vs = reinterpret_cast<float*>(fst + kApKeys + kApChunk);       // [kApKeys + kApChunk]
    double* vd = reinterpret_cast<double*>(vs + kApKeys + kApChunk);      // [kApKeys + kApChunk] (with64 only)
    static_assert(kApKeys <= 128, "the mask of first entries has two words");
    PFV_LANES(e, len) {
      kh[e] = (uint32_t)agg[ix[p0 + e]];
      vs[e] = v32[p0 + e];
      if constexpr (W64) vd[e] = v64[p0 + e];
    }
    PFV_LANES(u, kApChunk) kh[len + u] = 0xffffffffu;
    PFV_LANES(i, 2) mask[i] = 0ull;
    w.lsync();
    PFV_LANES(e, len) {
      const uint32_t k = kh[e];
      int dup = 0;
      for (int q0 = 0; q0 < e; q0 += kApChunk) {
#pragma unroll
        for (int u = 0; u < kApChunk; ++u) dup |= (q0 + u < e && kh[q0 + u] == k) ? 1 : 0;
      }
      if (!dup) atomic_or_u64(mask + (e >> 6), 1ull << (e & 63));
    }
    w.lsync();
    const unsigned long long m0 = mask[0], m1 = mask[1];
    const int nf = popcount64(m0) + popcount64(m1);
    PFV_LANES(e, len) {
      const unsigned long long word = e < 64 ? m0 : m1;
      const unsigned long long bit = 1ull << (e & 63);
      if (word & bit) fst[popcount64(word & (bit - 1ull)) + (e < 64 ? 0 : popcount64(m0))] = e;
      else kh[e] |= 0x80000000u;
    }
    w.lsync();
    PFV_LANES(j, nf) {
      const uint32_t k = kh[fst[j]];
      int rank = 0;
      double sum = 0.0, sum64 = 0.0;
      for (int q0 = 0; q0 < len; q0 += kApChunk) {
#pragma unroll
        for (int u = 0; u < kApChunk; ++u) {
          const uint32_t kq = kh[q0 + u];
          const float vq = vs[q0 + u];
          rank += kq < k ? 1 : 0;
          // (for a first entry no earlier one has its key: the whole row in entry order is its run in entry order)
          if ((kq & 0x7fffffffu) == k) sum += (double)vq;
          if constexpr (W64) {
            const double dq = vd[q0 + u];
            if ((kq & 0x7fffffffu) == k) sum64 += dq;
          }
        }
      }
      sx[p0 + rank] = (int32_t)k;
      sv[p0 + rank] = sum;
      if constexpr (W64) sv64[p0 + rank] = sum64;
    }
    if (w.lane0()) al[r] = nf;
    w.lsync();
  };
  const size_t lds32 = (kApKeys + kApChunk) * (2 * sizeof(int32_t) + sizeof(float)) + 16;
  if (want64) {
    wave_for<16>(s, n, lds32 + (kApKeys + kApChunk) * sizeof(double),
                 PFV_LAMBDA(const WaveCtx& w) { rank_rows(w, std::true_type{}); });
  } else {
    wave_for<16>(s, n, lds32, PFV_LAMBDA(const WaveCtx& w) { rank_rows(w, std::false_type{}); });
  }
  exclusive_scan<int32_t, int64_t>(s, c.scratch, al, pos, (size_t)n);
  wave_for<8>(s, n, 16, PFV_LAMBDA(const WaveCtx& w) {
    const int64_t r = w.item;
    const int p0 = fp[r];
    const int64_t o = pos[r];
    PFV_LANES(q, al[r]) {
      cx[o + q] = sx[p0 + q];
      cv[o + q] = sv[p0 + q];
      if (cv64) cv64[o + q] = sv64[p0 + q];
    }
    if (w.lane0()) {
      cp[r] = (int32_t)o;
      if (r + 1 == n) cp[n] = (int32_t)pos[n];
    }
  });
  amg.ap_ok = true;
  amg.ap64_ok = want64;
}

// y = tt + omega D^-1 (b - (t + alpha AP xs)) with tt = x0 + alpha P xs, xs = xc (+ xc2), x0 = x on entry and t = A_s x0:
// the post-smoothing step of level 0 in one launch, in place (a row reads only its own x0[r]).  xs is a vector of the
// first coarse level (2 MB at 2 M cells: the gather stays in L2, no window).
#ifndef PFV_EMULATE
// A workgroup takes 256 rows.  Their entries are one contiguous stretch of AP (~2 000 at 7-8 per row), so they are
// streamed by a thread per ENTRY -- every lane of every load busy -- and the products go to LDS; then a thread per ROW
// adds its stretch of products in entry order and finishes the row, its six scalars read by full wavefronts.  (Eight
// lanes per row, as the short-row products do it, issued 13 memory instructions per 8 rows with an eighth of the lanes
// active in half of them, and ran 145 us on 160 MB: bound by the issue of loads, not by bytes.)  Rows of any length:
// the stretch goes through LDS in chunks of CH products.
// RES: t holds d = b - A_s x0 (the residual form of the level's product): y = tt + omega D^-1 (d - alpha AP xs), and
// neither b nor a separate t is read.
template <int CH, bool RES>
__global__ void __launch_bounds__(256) k_amg_post_ap(int64_t nrows, const int32_t* __restrict__ ap,
                                                     const int32_t* __restrict__ ax, const double* __restrict__ av,
                                                     const int32_t* __restrict__ agg, const double* __restrict__ xc,
                                                     const double* __restrict__ xc2, const double* __restrict__ t,
                                                     const double* __restrict__ b, const double* __restrict__ dinv,
                                                     double omega, double alpha, double* x) {
  __shared__ double prod[CH];
  const int64_t row0 = (int64_t)blockIdx.x * 256;
  const int64_t row1 = row0 + 256 < nrows ? row0 + 256 : nrows;
  const int64_t row = row0 + threadIdx.x;
  const bool live = row < nrows;
  const int a0 = ap[row0], e0 = ap[row1];
  int a = 0, e = 0;
  double x0 = 0.0, tr = 0.0, br = 0.0, dr = 0.0, xr = 0.0;
  if (live) {
    a = ap[row];
    e = ap[row + 1];
    const int k = agg[row];
    x0 = x[row];
    tr = t[row];
    if (!RES) br = b[row];
    dr = dinv[row];
    xr = xc[k];
    if (xc2) xr += xc2[k];
  }
  double sum = 0.0;
  for (int c0 = a0; c0 < e0; c0 += CH) {
    constexpr int U = CH / 256;
    int k[U];
    double v[U], xs[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int p = c0 + u * 256 + (int)threadIdx.x;
      const bool ok = p < e0;
      k[u] = ok ? ax[p] : -1;
      v[u] = ok ? av[p] : 0.0;
    }
#pragma unroll
    for (int u = 0; u < U; ++u) {
      xs[u] = k[u] >= 0 ? xc[k[u]] : 0.0;
      if (xc2 && k[u] >= 0) xs[u] += xc2[k[u]];
    }
#pragma unroll
    for (int u = 0; u < U; ++u) prod[u * 256 + threadIdx.x] = v[u] * xs[u];
    __syncthreads();
    const int lo = a > c0 ? a : c0, hi = e < c0 + CH ? e : c0 + CH;
    for (int p = lo; p < hi; ++p) sum += prod[p - c0];  // entry order
    __syncthreads();
  }
  if (live) {
    const double tt = x0 + alpha * xr;
    x[row] = RES ? tt + omega * dr * (tr - alpha * sum) : tt + omega * dr * (br - (tr + alpha * sum));
  }
}
#endif
// b == nullptr: t holds d = b - A_s x0 (PFV_AMG_L0_RESIDUAL)
static void amg_post_ap(pfv_ctx_impl& c, const Amg& amg, const AmgLevel& L, const double* b, const double* t,
                        const double* xc, const double* xc2, double* x) {
  stream_t s = c.stream;
  const int64_t n = L.n;
  const int32_t* ap = amg.ap_ptr;
  const int32_t* ax = amg.ap_col;
  const double* av = amg.ap_val;
  const int32_t* agg = L.agg;
  const double* dinv = L.dinv;
  const double omega = L.omega, alpha = amg.alpha;
#ifdef PFV_EMULATE
  parallel_for(s, n, PFV_LAMBDA(int64_t r) {
    double sum = 0.0;
    for (int p = ap[r]; p < ap[r + 1]; ++p) sum += av[p] * (xc2 ? xc[ax[p]] + xc2[ax[p]] : xc[ax[p]]);
    const int k = agg[r];
    const double tt = x[r] + alpha * (xc2 ? xc[k] + xc2[k] : xc[k]);
    x[r] = b ? tt + omega * dinv[r] * (b[r] - (t[r] + alpha * sum)) : tt + omega * dinv[r] * (t[r] - alpha * sum);
  });
#else
  const unsigned blocks = (unsigned)((n + 255) / 256);
  if (b)
    PFV_LAUNCH(HIP_KERNEL_NAME(k_amg_post_ap<2048, false>), dim3(blocks), dim3(256), 0, s, n, ap, ax, av, agg, xc, xc2, t, b,
               dinv, omega, alpha, x);
  else
    PFV_LAUNCH(HIP_KERNEL_NAME(k_amg_post_ap<2048, true>), dim3(blocks), dim3(256), 0, s, n, ap, ax, av, agg, xc, xc2, t, b,
               dinv, omega, alpha, x);
  PFV_HIP_CHECK(hipGetLastError());
#endif
}

// The closing work: the coarsest level (explicit inverse when small enough; coupled hierarchy: the gathered level and
// the replicated hierarchy below it), the damping, the row safeguard, and what the kept maps belong to.
static void amg_setup_finish(pfv_ctx_impl& c, Amg& amg, const CsrPattern& A, double nnz_sum, unsigned long long csum,
                             unsigned long long level0_sum) {
  const AmgSwitches& w = amg.sw;
  AmgDist* D = amg.dist.get();
  AmgLevel& Lc = *amg.lev[amg.nlev - 1];
  if (D) {
    amg_build_global(c, amg, *D, Lc, *D->plan[amg.nlev - 1]);
  } else if (Lc.n <= kAmgDenseMax) {
    amg.dense_ok = amg_dense_invert(c, w, amg.wk, *Lc.P, Lc.val, amg.dense);
  }
  amg.op_complexity = nnz_sum / (double)A.nnz;
  for (size_t k = 0; k < amg.nlev; ++k) {
    amg.lev[k]->omega = amg.omega;
    amg.lev[k]->rho = 0.0;
  }
  if (w.safe_rows) {
    for (size_t k = 0; k < amg.nlev; ++k) {
      AmgLevel& Lk = *amg.lev[k];
      if (k + 1 < amg.nlev || !amg.dense_ok) amg_safeguard_rows(c, *Lk.P, Lk.val, Lk.dinv);
    }
  }
  if (amg.omega_auto && !D) amg_estimate_omegas(c, amg);
  amg.valid = true;
  if (env_int("PFV_DEBUG_AMG", 0)) {
    std::fprintf(stderr, "amg_setup: filter theta %.3f (nnz %lld -> %lld), levels:", amg.filter_theta, (long long)A.nnz,
                 (long long)amg.filt_nnz);
    for (size_t k = 0; k < amg.nlev; ++k)
      std::fprintf(stderr, " %lld/%lld(w%.3f)", (long long)amg.lev[k]->n, (long long)amg.lev[k]->P->nnz, amg.lev[k]->omega);
    const AmgLevel& L0 = *amg.lev[0];
    std::fprintf(stderr, " reuse %d window0 %d\n", (int)amg.reused, (L0.win && L0.win->ok) ? L0.win->wmax : -1);
  }
  amg.gal_for_sum = D ? 0ull : level0_sum;
  if (w.reuse && (!D || csum != 0)) {
    amg.maps_ok = true;
    amg.maps_n = A.nrows;
    amg.maps_nnz = A.nnz;
    amg.maps_cfg = amg_maps_cfg(w);
    amg.maps_sum = csum;
    amg.maps_epoch = c.symbolic_epoch;
    amg.maps_tag = amg_maps_tag(w);
  }
}

static void amg_setup(pfv_ctx_impl& c, Amg& amg, const CsrPattern& A, const double* val, int bs,
                      const double* diag, const WinCsr* win0) {
  stream_t s = c.stream;
  Timer tm;
  tm.start(s);
  AmgDist* D = amg.dist.get();  // coupled hierarchy of a sharded solve (amg_dist.inc): A = owned rows x (owned + halo)
  amg.bs = bs;
  amg.valid = amg.dense_ok = amg.ap_ok = amg.ap64_ok = amg.galerkin_ap = false;
  amg.ap_nnz = 0;
  amg.sysP = &A;
  amg.sysV = val;
  if (A.nrows % bs) throw Error(PFV_ERR_ARGUMENT, "AMG: system size is not a multiple of the block size");
  AmgSwitches& w = amg.sw = amg_read_switches(bs);
  if (amg.no_filter) w.filter_theta = 0.0;  // (a gathered coarse level: already the product of a filtered one)
  if (amg.coarse_target > 0) w.coarse_target = std::min(kAmgDenseMax, amg.coarse_target);
  amg.omega_auto = w.omega_auto;
  amg.omega = w.omega;
  amg.alpha = w.alpha;
  amg.passes = w.passes;
  amg.fp32 = w.fp32;
  amg.filter_theta = w.filter_theta;
  amg.gamma_levels = w.gamma_levels;
  amg.fuse_rows = w.fuse_rows;
  amg.fuse_cycle = w.fuse_cycle;
  amg.restrict_lanes = w.restrict_lanes;
  unsigned long long csum = 0;
  const bool reuse = amg_decide_reuse(c, amg, A, csum);
  // (coupled hierarchy: the shape of the cycle must be the same on every rank -- decided from the gathered size)
  const int64_t rows_for_shape = D ? D->global_rows0 / D->world : A.nrows;
  amg.gamma = std::max(1, std::min(2, w.gamma_set ? w.gamma_raw : (rows_for_shape >= kAmgWTopRows ? 2 : 1)));
  amg.maps_ok = false;
  amg.reused = reuse;
  if (bs > 1) amg_check_full_blocks(c, A, bs);
  unsigned long long level0_sum = amg_setup_level0(c, amg, A, val, diag, win0, csum);
  // sizes of the Galerkin products known from the previous setup?  (same finest pattern the hierarchy is coarsened from
  // -- the filtered one where the filter is on --, same aggregate maps)
  amg.gal_use = reuse && !D && level0_sum != 0 && amg.gal_for_sum == level0_sum && w.sizes_reuse;
  amg.gal_k = 0;
  if (!amg.gal_use) amg.gal_sizes.clear();
  double nnz_sum = 0.0;
  size_t l = 0;
  while (true) {
    AmgLevel& L = amg_level(amg, l);
    nnz_sum += (double)L.P->nnz;
    amg_level_buffers(c, amg, L, l);
    if (D ? (l >= 1 && l == D->kgather) : (L.n <= w.coarse_target || (int)l + 1 >= kAmgMaxLevels)) break;
    const int slot = amg_coarsen_level(c, amg, l, reuse);
    if (slot < 0) break;  // coarsening stalled: this level is the coarsest
    if (l == 0 && !amg.ap_ok) amg_build_ap(c, amg, false);  // (kept maps: built before the product that reads it)
    AmgLevel& Ln = amg_level(amg, l + 1);
    Ln.n = L.nc_cells * bs;
    // the last intermediate matrix becomes the new level (its old buffers go back to the slot)
    amg_swap_pattern(Ln.P_own, amg.wk.P[slot]);
    Ln.val_own.swap(amg.wk.V[slot]);
    Ln.dinv.swap(amg.wk.D[slot]);
    Ln.P = &Ln.P_own;
    Ln.val = Ln.val_own.p;
    Ln.win = nullptr;
    Ln.m = Ln.n;
    if (D) {
      amg_dist_rename_halo(c, *D, l, L.agg, L.nc_cells, bs, Ln);
      amg_dist_decide_gather(c, *D, l, Ln.n, w.gather_rows);
    }
    if (Ln.n > w.coarse_target && Ln.P_own.nnz >= 200000) {  // worth it only for the big levels
      win_build(c, Ln.P_own, Ln.win_own);
      Ln.win = &Ln.win_own;
    }
    ++l;
  }
  amg.nlev = l + 1;
  amg_setup_finish(c, amg, A, nnz_sum, csum, level0_sum);
  // (entries of AP: a read for the statistics only, where the setup waits for its own end anyway)
  if (amg.ap_ok) amg.ap_nnz = read_scalar<int64_t>(s, amg.ap_pos.p + amg.lev[0]->n);
  c.stats.amg_ap_nnz = amg.ap_nnz;
  c.stats.amg_galerkin_ap = amg.galerkin_ap ? 1 : 0;
  amg.setup_ms = tm.stop(s);
}


// ---- the cycle's matrix products: y = A x, or the damped-Jacobi update y = x + omega D^-1 (b - A x)
// in one pass.  The preconditioner only has to be a fixed linear operator close to A^-1, so the
// matrix values are streamed in single precision (8 instead of 12 bytes per entry; the vectors and
// the accumulation stay double) -- the Krylov loop around it works on the double matrix.
#ifndef PFV_EMULATE
// MODE 0: y = A x;  1: y = x + omega dinv (b - A x);  4 / 5: the fused forms of the cycle (SpmvFuse, spmv_win.inc);
// 6: y = b - A x
template <int L, int U, class VT, int MODE>
__global__ void __launch_bounds__(256) k_amg_spmv(int64_t nrows, const int32_t* __restrict__ indptr,
                                                  const int32_t* __restrict__ indices,
                                                  const VT* __restrict__ val, const double* __restrict__ x,
                                                  double* __restrict__ y, const double* __restrict__ b,
                                                  const double* __restrict__ dinv, double omega, const SpmvFuse F) {
  const int lane = threadIdx.x % L;
  const int64_t row = (int64_t)blockIdx.x * (256 / L) + threadIdx.x / L;
  if (row >= nrows) return;
  const int a = indptr[row], e = indptr[row + 1];
  double sum = 0.0;
  for (int p = a + lane; p < e; p += L * U) {
    int col[U];
    double v[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int pp = p + u * L;
      const bool ok = pp < e;
      const int pc = ok ? pp : a;
      col[u] = indices[pc];
      const double vv = (double)val[pc];
      v[u] = ok ? vv : 0.0;
    }
#pragma unroll
    for (int u = 0; u < U; ++u) sum += v[u] * (MODE == 4 ? spmv_prolonged(F, x, col[u]) : x[col[u]]);
  }
#pragma unroll
  for (int o = L / 2; o > 0; o >>= 1) sum += __shfl_down(sum, o, L);
  if (lane == 0) {
    if (MODE == 1) y[row] = x[row] + omega * dinv[row] * (b[row] - sum);
    else if (MODE == 4) y[row] = spmv_prolonged(F, x, row) + omega * dinv[row] * (b[row] - sum);
    else if (MODE == 5) {
      const double res = b[row] - sum;
      y[row] = res;
      F.y2[row] = omega * dinv[row] * res;
    } else if (MODE == 6) y[row] = b[row] - sum;
    else y[row] = sum;
  }
}
template <int L, class VT, int MODE>
static void launch_amg_spmv(stream_t s, int U, int64_t nrows, const int32_t* ip, const int32_t* ix, const VT* val,
                            const double* x, double* y, const double* b, const double* dinv, double omega,
                            const SpmvFuse& F) {
  const unsigned blocks = (unsigned)((nrows + 256 / L - 1) / (256 / L));
  if (U <= 2)
    PFV_LAUNCH(HIP_KERNEL_NAME(k_amg_spmv<L, 2, VT, MODE>), dim3(blocks), dim3(256), 0, s, nrows, ip, ix,
                       val, x, y, b, dinv, omega, F);
  else if (U <= 4)
    PFV_LAUNCH(HIP_KERNEL_NAME(k_amg_spmv<L, 4, VT, MODE>), dim3(blocks), dim3(256), 0, s, nrows, ip, ix,
                       val, x, y, b, dinv, omega, F);
  else
    PFV_LAUNCH(HIP_KERNEL_NAME(k_amg_spmv<L, 6, VT, MODE>), dim3(blocks), dim3(256), 0, s, nrows, ip, ix,
                       val, x, y, b, dinv, omega, F);
}
#endif

template <class VT, int MODE>
static void amg_spmv_t(pfv_ctx_impl& c, const CsrPattern& P, const VT* val, const double* x, double* y,
                       const double* b, const double* dinv, double omega, const SpmvFuse& F = SpmvFuse{}) {
  stream_t s = c.stream;
  const int64_t nrows = P.nrows;
  if (nrows == 0) return;
  const int32_t* ip = P.indptr;
  const int32_t* ix = P.indices;
#ifdef PFV_EMULATE
  parallel_for(s, nrows, PFV_LAMBDA(int64_t r) {
    double sum = 0.0;
    for (int p = ip[r]; p < ip[r + 1]; ++p) sum += (double)val[p] * (MODE == 4 ? spmv_prolonged(F, x, ix[p]) : x[ix[p]]);
    if (MODE == 1) y[r] = x[r] + omega * dinv[r] * (b[r] - sum);
    else if (MODE == 4) y[r] = spmv_prolonged(F, x, r) + omega * dinv[r] * (b[r] - sum);
    else if (MODE == 5) {
      const double res = b[r] - sum;
      y[r] = res;
      F.y2[r] = omega * dinv[r] * res;
    } else if (MODE == 6) y[r] = b[r] - sum;
    else y[r] = sum;
  });
#else
  const double avg = (double)P.nnz / (double)nrows;
  const int L = avg <= 20 ? 8 : (avg <= 160 ? 16 : 32);
  const int U = std::max(1, std::min(6, (int)std::ceil(1.1 * avg / L)));
  if (L == 8) launch_amg_spmv<8, VT, MODE>(s, U, nrows, ip, ix, val, x, y, b, dinv, omega, F);
  else if (L == 16) launch_amg_spmv<16, VT, MODE>(s, U, nrows, ip, ix, val, x, y, b, dinv, omega, F);
  else launch_amg_spmv<32, VT, MODE>(s, U, nrows, ip, ix, val, x, y, b, dinv, omega, F);
  PFV_HIP_CHECK(hipGetLastError());
#endif
}
// y = A_l x  (smooth_b == nullptr)   or   y = x + omega D^-1 (smooth_b - A_l x)
static void amg_spmv(pfv_ctx_impl& c, const Amg& amg, const AmgLevel& L, const double* x, double* y,
                     const double* smooth_b) {
  const double* dinv = L.dinv;
#ifndef PFV_EMULATE
  if (L.win && L.win->ok) {
    Reduce R{};
    if (L.v32) {
      if (smooth_b) spmv_win<float, 1>(c, *L.P, *L.win, L.v32, x, y, smooth_b, dinv, L.omega, R);
      else spmv_win<float, 0>(c, *L.P, *L.win, L.v32, x, y, nullptr, nullptr, 0.0, R);
    } else {
      if (smooth_b) spmv_win<double, 1>(c, *L.P, *L.win, L.val, x, y, smooth_b, dinv, L.omega, R);
      else spmv_win<double, 0>(c, *L.P, *L.win, L.val, x, y, nullptr, nullptr, 0.0, R);
    }
    return;
  }
#endif
  if (L.v32) {
    if (smooth_b) amg_spmv_t<float, 1>(c, *L.P, L.v32, x, y, smooth_b, dinv, L.omega);
    else amg_spmv_t<float, 0>(c, *L.P, L.v32, x, y, nullptr, nullptr, 0.0);
  } else {
    if (smooth_b) amg_spmv_t<double, 1>(c, *L.P, L.val, x, y, smooth_b, dinv, L.omega);
    else amg_spmv_t<double, 0>(c, *L.P, L.val, x, y, nullptr, nullptr, 0.0);
  }
}
// the fused products of the cycle on level L (MODE 4 / 5, see k_spmv_win): b = the level's right-hand side
template <int MODE>
static void amg_spmv_fused(pfv_ctx_impl& c, const AmgLevel& L, const double* x, double* y, const double* b,
                           const SpmvFuse& F) {
  const double* dinv = L.dinv;
#ifndef PFV_EMULATE
  if (L.win && L.win->ok) {
    Reduce R{};
    if (L.v32) spmv_win<float, MODE>(c, *L.P, *L.win, L.v32, x, y, b, dinv, L.omega, R, nullptr, 0, F);
    else spmv_win<double, MODE>(c, *L.P, *L.win, L.val, x, y, b, dinv, L.omega, R, nullptr, 0, F);
    return;
  }
#endif
  if (L.v32) amg_spmv_t<float, MODE>(c, *L.P, L.v32, x, y, b, dinv, L.omega, F);
  else amg_spmv_t<double, MODE>(c, *L.P, L.val, x, y, b, dinv, L.omega, F);
}
// d = b - A_s x on level 0 of the AP path: MODE 6 of the lane-group products.  Windowed rows of up to 22 entries on
// average (the filtered operator of a flow system: 18) take FOUR lanes per row: a 64-row block is one pass of its 256
// threads where 8 lanes make two, 18 entries fill 18 of 20 lane slots where 8 x 3 fill 18 of 24, and the shuffle tree
// has two steps -- 100.8 -> 86.6 us on the 2 M-cell grid (5 or 6 chunks per lane alike; 3 chunks, i.e. a second trip for
// most rows: 88.8).  Another summation order than the 8-lane form: a switch of its own.
static void amg_residual_l0(pfv_ctx_impl& c, const Amg& amg, const AmgLevel& L, const double* x, const double* b,
                            double* d) {
#ifndef PFV_EMULATE
  const double avg = (double)L.P->nnz / (double)std::max<int64_t>(L.n, 1);
  if (amg.sw.l0_lanes4 && L.win && L.win->ok && L.v32 && avg <= 22.0) {
    const int U = std::max(1, std::min(6, (int)std::ceil(1.1 * avg / 4)));
    launch_spmv_win_u<4, float, 6>(c.stream, U, *L.win, L.P->indptr.p, L.v32, x, d, b, L.dinv, L.omega, Reduce{});
    PFV_HIP_CHECK(hipGetLastError());
    return;
  }
#endif
  amg_spmv_fused<6>(c, L, x, d, b, SpmvFuse{});
}

// Damping of the Jacobi smoother per level: omega_l = sigma / rho_l with rho_l ~ rho(D^-1 A_l) from a power iteration.
// Damped Jacobi needs omega rho < 2 to damp the upper end of the spectrum; MPFA systems on simplices are not M-matrices
// (positive off-diagonal entries) and reach rho ~ 2.3, where a fixed omega fitted on one matrix is a cliff for the next.
// K steps of v <- (I - D^-1 A) v (the smoothing product itself with omega = 1 and a zero right-hand side: the shift
// by the identity spreads the upper end of the spectrum -- (rho_2 - 1) / (rho_1 - 1) instead of rho_2 / rho_1 --,
// dominant magnitude rho - 1 as soon as rho > 2, which is the case that matters), no normalisation, rho - 1 from the
// ratio of the last two 2-norms.  The estimate approaches rho from below: sigma (PFV_AMG_OMEGA_RHO_PCT,
// default 1.8) keeps the margin.  Deterministic: fixed start vector, fixed-shape reductions.  ~1 ms at 2 M rows.
static void amg_estimate_omegas(pfv_ctx_impl& c, Amg& amg) {
  stream_t s = c.stream;
  const int K = amg.sw.omega_power_steps;
  const double sigma = amg.sw.omega_sigma;
  const int64_t n0 = amg.lev[0]->n;
  double* va = amg.pw_a.ensure(n0);
  double* vb = amg.pw_b.ensure(n0);
  double* zero = amg.pw_zero.ensure(n0);
  constexpr int kChunks = 256;
  double* part = amg.pw_part.ensure(2 * kChunks + 2 * kAmgMaxLevels);
  double* out = part + 2 * kChunks;  // [2 per level]
  be_memset(zero, 0, sizeof(double) * (size_t)n0, s);
  size_t nest = 0;
  for (size_t l = 0; l < amg.nlev; ++l) {
    AmgLevel& L = *amg.lev[l];
    const bool smooths = l + 1 < amg.nlev || !amg.dense_ok;
    if (!smooths) continue;
    const int64_t n = L.n;
    parallel_for(s, n, PFV_LAMBDA(int64_t i) {
      // deterministic start vector with all frequencies in it
      uint64_t z = (uint64_t)i * 0x9E3779B97F4A7C15ull + 0x7F4A7C15ull;
      z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
      z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
      va[i] = 0.5 + (double)(z >> 11) * (1.0 / 9007199254740992.0);
    });
    const double keep = L.omega;
    L.omega = 1.0;
    double* x = va;
    double* y = vb;
    for (int k = 0; k < K; ++k) {
      amg_spmv(c, amg, L, x, y, zero);  // y = x - D^-1 A x
      double* t = x; x = y; y = t;
    }
    L.omega = keep;
    // ||x||^2 (last iterate) and ||y||^2 (the one before): fixed-shape two-stage sums
    const double* xa = x;
    const double* ya = y;
    wave_for<64>(s, kChunks, 2 * 64 * sizeof(double) + 16, PFV_LAMBDA(const WaveCtx& w) {
      double* p1 = reinterpret_cast<double*>(w.lds);
      double* p2 = p1 + 64;
      PFV_LANES(ln, 64) {
        double a = 0.0, b = 0.0;
        for (int64_t i = w.item * 64 + ln; i < n; i += (int64_t)kChunks * 64) {
          a += xa[i] * xa[i];
          b += ya[i] * ya[i];
        }
        p1[ln] = a;
        p2[ln] = b;
      }
      w.sync();
      if (w.lane0()) {
        double a = 0.0, b = 0.0;
        for (int j = 0; j < 64; ++j) { a += p1[j]; b += p2[j]; }
        part[w.item] = a;
        part[kChunks + w.item] = b;
      }
      w.sync();
    });
    double* o = out + 2 * nest;
    parallel_for(s, 1, PFV_LAMBDA(int64_t) {
      double a = 0.0, b = 0.0;
      for (int j = 0; j < kChunks; ++j) { a += part[j]; b += part[kChunks + j]; }
      o[0] = a;
      o[1] = b;
    });
    ++nest;
  }
  if (nest == 0) return;
  std::vector<double> h(2 * nest);
  be_d2h(h.data(), out, sizeof(double) * 2 * nest, s);
  size_t k = 0;
  for (size_t l = 0; l < amg.nlev; ++l) {
    AmgLevel& L = *amg.lev[l];
    const bool smooths = l + 1 < amg.nlev || !amg.dense_ok;
    if (!smooths) continue;
    const double a = h[2 * k], b = h[2 * k + 1];
    ++k;
    double rho = (b > 0.0 && a > 0.0 && a < 1.0e300) ? std::sqrt(a / b) + 1.0 : 0.0;
    if (!(rho > 0.5)) rho = 0.0;  // (degenerate estimate: keep the fixed damping)
    L.rho = rho;
    if (rho > 0.0) L.omega = std::min(1.0, sigma / rho);
  }
}

// Small levels are bound by the number of dependent launches, not by bytes (a product on 20 000 rows lasts the
// ~5 us a product on 76 rows does): there the residual product rides in the restriction kernel and the
// prolongation in the post-smoothing product -- two launches per level visit instead of four.
//   bc[R] = sum_{r in members(R)} (b[r] - (A x)[r]),  xn[R] = omega dn[R] bc[R]
template <class VT>
static void amg_restrict_residual(pfv_ctx_impl& c, const Amg& amg, const AmgLevel& L, const AmgLevel& Ln, const VT* val,
                                  const double* b, const double* x, bool next_smooths) {
  stream_t s = c.stream;
  const int bs = amg.bs;
  const double omega = Ln.omega;  // (the first smoothing step of the NEXT level rides along)
  const int32_t* ip = L.P->indptr;
  const int32_t* ix = L.P->indices;
  const int32_t* mptr = L.mptr;
  const int32_t* mem = L.mem;
  double* bc = Ln.b;
  double* xn = Ln.x;
  const double* dn = Ln.dinv;
  // 64 lanes per coarse row: 8 lanes per member row (a lane walking a whole member row alone pays its ~20 entries as
  // a chain of dependent-latency trips: measured slower than the two launches it replaces), partial sums through LDS
  // in lane order (deterministic)
  wave_for<64>(s, Ln.n, 64 * sizeof(double) + 16, PFV_LAMBDA(const WaveCtx& w) {
    double* sh = reinterpret_cast<double*>(w.lds);
    const int64_t R = w.item;
    const int64_t I = R / bs;
    const int a = (int)(R - I * bs);
    const int q0 = mptr[I], nm = mptr[I + 1] - q0;
    constexpr int SUB = 8;
    double part = 0.0;
    for (int t = w.lane; t < nm * SUB; t += w.width) {
      const int q = t / SUB, sl = t - q * SUB;
      const int64_t r = (int64_t)mem[q0 + q] * bs + a;
      double sum = 0.0;
      for (int p = ip[r] + sl; p < ip[r + 1]; p += SUB) sum += (double)val[p] * x[ix[p]];
      part += (sl == 0 ? b[r] : 0.0) - sum;
    }
    sh[w.lane] = part;
    w.lsync();
    if (w.lane0()) {
      double sum = 0.0;
      for (int j = 0; j < w.width; ++j) sum += sh[j];
      bc[R] = sum;
      if (next_smooths) xn[R] = omega * dn[R] * sum;
    }
    w.lsync();
  });
}
//   y = t + omega D^-1 (b - A t),  t[c] = x[c] + alpha xc[agg(c)]  (t is never stored)
template <class VT>
static void amg_prolong_smooth(pfv_ctx_impl& c, const Amg& amg, const AmgLevel& L, const VT* val, const double* b,
                               const double* x, const double* xc, double* y) {
  stream_t s = c.stream;
  const int bs = amg.bs;
  const double omega = L.omega, alpha = amg.alpha;
  const int32_t* ip = L.P->indptr;
  const int32_t* ix = L.P->indices;
  const int32_t* agg = L.agg;
  const double* dinv = L.dinv;
  wave_for<16>(s, L.n, 16 * sizeof(double) + 16, PFV_LAMBDA(const WaveCtx& w) {
    double* sh = reinterpret_cast<double*>(w.lds);
    const int64_t r = w.item;
    const int p0 = ip[r], len = ip[r + 1] - p0;
    double part = 0.0;
    PFV_LANES(k, len) {
      const int cc = ix[p0 + k];
      const int ci = cc / bs;
      part += (double)val[p0 + k] * (x[cc] + alpha * xc[(int64_t)agg[ci] * bs + (cc - ci * bs)]);
    }
    sh[w.lane] = part;
    w.lsync();
    if (w.lane0()) {
      double sum = 0.0;
      for (int j = 0; j < w.width; ++j) sum += sh[j];
      const int64_t i = r / bs;
      const double tr = x[r] + alpha * xc[(int64_t)agg[i] * bs + (r - i * bs)];
      y[r] = tr + omega * dinv[r] * (b[r] - sum);
    }
    w.lsync();
  });
}

// bc[R] = sum over the members of R of (b - t),  t = A_l x;  the next level's first smoothing step (from a zero guess)
// rides along: xn[R] = omega_n dn[R] bc[R].  b == nullptr: t holds d = b - A_l x already (one gather per member, the
// same numbers added in the same order)
static void amg_restrict(pfv_ctx_impl& c, const Amg& amg, const AmgLevel& L, const AmgLevel& Ln, const double* b,
                         const double* t, bool next_smooths) {
  stream_t s = c.stream;
  const int bs = amg.bs;
  const double omega_n = Ln.omega;
  {
    const int32_t* mptr = L.mptr;
    const int32_t* mem = L.mem;
    double* bc = Ln.b;
    double* xn = Ln.x;
    const double* dn = Ln.dinv;
    // 8 lanes per coarse row, one member each (a thread per coarse row walked its ~8 members through two
    // dependent gathers apiece: 46 us on the finest level of the 2 M-cell system, a quarter of the solve at 200 k
    // cells); the partial sums are added in member order
    if (!amg.restrict_lanes) {  // a thread per coarse row (block systems; PFV_AMG_RESTRICT_LANES overrides)
      parallel_for(s, Ln.n, PFV_LAMBDA(int64_t R) {
        const int64_t I = R / bs;
        const int a = (int)(R - I * bs);
        double sum = 0.0;
        for (int q = mptr[I]; q < mptr[I + 1]; ++q) {
          const int64_t r = (int64_t)mem[q] * bs + a;
          sum += b ? b[r] - t[r] : t[r];
        }
        bc[R] = sum;
        if (next_smooths) xn[R] = omega_n * dn[R] * sum;
      });
    } else
    wave_for<8>(s, Ln.n, 8 * sizeof(double) + 16, PFV_LAMBDA(const WaveCtx& w) {
      double* sh = reinterpret_cast<double*>(w.lds);
      const int64_t R = w.item;
      const int64_t I = R / bs;
      const int a = (int)(R - I * bs);
      const int q0 = mptr[I], nm = mptr[I + 1] - q0;
      double part = 0.0;
      PFV_LANES(q, nm) {
        const int64_t r = (int64_t)mem[q0 + q] * bs + a;
        part += b ? b[r] - t[r] : t[r];
      }
      sh[w.lane] = part;
      w.lsync();
      if (w.lane0()) {
        double sum = 0.0;
        for (int j = 0; j < w.width; ++j) sum += sh[j];
        bc[R] = sum;
        if (next_smooths) xn[R] = omega_n * dn[R] * sum;
      }
      w.lsync();
    });
  }
}

// approximate solution of A_l x = b; returns where it was left: x, or -- fused small levels -- the level's t
static double* amg_cycle(pfv_ctx_impl& c, Amg& amg, size_t l, const double* b, double* x, bool x_is_presmoothed,
                         int visit) {
  stream_t s = c.stream;
  AmgLevel& L = *amg.lev[l];
  const int64_t n = L.n;
  const double omega = L.omega, alpha = amg.alpha;
  const double* dinv = L.dinv;
  double* t = L.t;
  if (l + 1 == amg.nlev) {
    if (amg.dense_ok) {
      amg_dense_apply(c, amg.dense, n, b, x);
    } else {
      // stalled coarsening above the dense limit: a few damped Jacobi sweeps
      parallel_for(s, n, PFV_LAMBDA(int64_t i) { x[i] = omega * dinv[i] * b[i]; });
      for (int sweep = 0; sweep < 2; ++sweep) {  // x -> t -> x
        amg_spmv(c, amg, L, x, t, b);
        amg_spmv(c, amg, L, t, x, b);
      }
    }
    return x;
  }
  AmgLevel& Ln = *amg.lev[l + 1];
  const int bs = amg.bs;
  const double omega_n = Ln.omega;  // the next level's first smoothing step (from a zero guess) rides in the restriction
  // fused launches on small levels without an SpMV window; the result of a fused post-smoothing lands in t, so it is
  // kept off level 0 (the caller's x) and off the levels their parent visits twice (the second visit would reuse t)
  const AmgPath path = amg_level_path(amg, l);
  const bool small = path.small;
  const bool twice = path.twice;  // (this level: visited twice by its parent)
  const bool fuse_up = path.fuse_up;
  // larger coarse levels (PFV_AMG_FUSE_CYCLE): the prolongation inside the post-smoothing product (k_spmv_win MODE 4).
  // The result cannot overwrite x (other row blocks still read it): it lands in t -- or, on the first visit of a level
  // visited twice, in u, which the second visit (whose scratch t is) leaves alone.  Level 0 keeps the two launches: its
  // result belongs in the caller's x, and forming t per WINDOW column there would cost more bytes than t's round trip.
  const bool fuse_big = path.fuse_big;
  // level 0 on the AP path: the product leaves d = b - A_s x0 in t, all the restriction and amg_post_ap read of b and t
  const bool res0 = l == 0 && amg.ap_ok && !small && amg.sw.l0_residual;
  if (!x_is_presmoothed) parallel_for(s, n, PFV_LAMBDA(int64_t i) { x[i] = omega * dinv[i] * b[i]; });
  // restriction; the first smoothing step of the next level (from a zero guess) rides along
  const bool next_smooths = l + 2 < amg.nlev;
  if (small) {
    if (L.v32) amg_restrict_residual<float>(c, amg, L, Ln, L.v32, b, x, next_smooths);
    else amg_restrict_residual<double>(c, amg, L, Ln, L.val, b, x, next_smooths);
  } else if (res0) {
    amg_residual_l0(c, amg, L, x, b, t);
    amg_restrict(c, amg, L, Ln, nullptr, t, next_smooths);
  } else {
    amg_spmv(c, amg, L, x, t, nullptr);
    amg_restrict(c, amg, L, Ln, b, t, next_smooths);
  }
  double* xc = amg_cycle(c, amg, l + 1, Ln.b, Ln.x, next_smooths, 0);
  const double* xc2 = nullptr;  // correction of the second visit, folded into this level's prolongation
  if (path.second) {
    // second visit: correct the coarse solution with a cycle on its residual (levels visited twice keep their
    // result in Ln.x or Ln.u: see fuse_up / fuse_big)
    double* r2 = Ln.r2.ensure(Ln.n);
    double* x2 = Ln.x2.ensure(Ln.n);
    const double* bcn = Ln.b;
    const double* x2r;
    if (amg.fuse_cycle) {
      // r2 = b_n - A_n xc and the visit's first smoothing step x2 = omega_n D_n^-1 r2 in the launch of the product
      SpmvFuse F;
      F.y2 = x2;
      amg_spmv_fused<5>(c, Ln, xc, r2, bcn, F);
      x2r = amg_cycle(c, amg, l + 1, r2, x2, true, 1);
    } else {
      double* tn = Ln.t;
      amg_spmv(c, amg, Ln, xc, tn, nullptr);
      parallel_for(s, Ln.n, PFV_LAMBDA(int64_t i) { r2[i] = bcn[i] - tn[i]; });
      x2r = amg_cycle(c, amg, l + 1, r2, x2, false, 1);
    }
    if (amg.fuse_cycle && !fuse_up) xc2 = x2r;  // (xc + x2r is formed where the prolongation reads them)
    else parallel_for(s, Ln.n, PFV_LAMBDA(int64_t i) { xc[i] += x2r[i]; });
  }
  if (fuse_up) {
    if (L.v32) amg_prolong_smooth<float>(c, amg, L, L.v32, b, x, xc, t);
    else amg_prolong_smooth<double>(c, amg, L, L.val, b, x, xc, t);
    return t;
  }
  if (fuse_big) {
    double* out = (twice && visit == 0) ? L.u.ensure(n) : t;
    SpmvFuse F;
    F.xc = xc;
    F.xc2 = xc2;
    F.agg = L.agg;
    F.bs = bs;
    F.alpha = alpha;
    amg_spmv_fused<4>(c, L, x, out, b, F);
    return out;
  }
  if (l == 0 && amg.ap_ok && !small) {
    // level 0 with AP: t = A_s x0 of the restriction (res0: d = b - A_s x0) is still in L.t (the coarse visits work in
    // the vectors of their own levels; nothing above has written it), x still holds x0 -- prolongation and
    // post-smoothing in one launch
    amg_post_ap(c, amg, L, res0 ? nullptr : b, t, xc, xc2, x);
    return x;
  }
  {
    const int32_t* agg = L.agg;
    parallel_for(s, n, PFV_LAMBDA(int64_t r) {  // corrected iterate into t, smoothed back into x
      const int64_t i = r / bs;
      const int64_t a = (int64_t)agg[i] * bs + (r - i * bs);
      t[r] = x[r] + alpha * (xc2 ? xc[a] + xc2[a] : xc[a]);
    });
  }
  amg_spmv(c, amg, L, t, x, b);
  return x;
}

// ---- Block preconditioner for coupled multi-physics / mixed-dimensional Jacobians (SURVEY 8(f) N1: "needs
// block-Jacobi/ILU0 or AMG-lite for md problems"; the systems of models/solution_strategy.py:830-884 that the reference
// hands to a direct solver).  The unknowns come grouped in contiguous blocks -- one per (variable, subdomain /
// interface): pressure in the 3-D matrix, pressure in every fracture plane, the mortar fluxes of every interface,
// temperature ... -- and the preconditioner is the block lower-triangular part of A with every diagonal block solved
// by its own hierarchy:
//     z_k = M_k^-1 (r_k - sum_{j < k} A_kj z_j),      M_k^-1 = one cycle of the aggregation AMG of A_kk
// (blocks of at most kAmgDenseMax rows: one level, i.e. the exact dense inverse -- fracture planes, intersections,
// mortar grids; the large elliptic blocks: the same cycle the flow solve uses).  A fixed linear operator, so GMRES
// and BiCGStab apply.  gs = false drops the coupling term (block Jacobi).
struct BlockPc {
  struct Blk {
    int64_t p0 = 0, p1 = 0;
    CsrPattern P;
    Buf<double> val, diag;
    std::unique_ptr<Amg> amg;
    bool ascending = false;  // every row of the block stores its columns in ascending order (blockpc_extract)
  };
  std::vector<int64_t> ptr;   // block boundaries as given by the caller
  std::vector<std::unique_ptr<Blk>> blk;
  bool gs = true;
  const double* for_val = nullptr;  // values of the system the blocks were extracted from (nullptr: stale)
  Buf<double> tmp;
  double setup_ms = 0.0;
};

// diagonal block [p0, p1) of (P, val) as a matrix of its own
static void blockpc_extract(pfv_ctx_impl& c, const CsrPattern& P, const double* val, BlockPc::Blk& B) {
  stream_t s = c.stream;
  const int64_t p0 = B.p0, n = B.p1 - B.p0;
  const int32_t* ip = P.indptr;
  const int32_t* ix = P.indices;
  Buf<int32_t> len;
  Buf<int64_t> pos;
  int32_t* ln = len.ensure(n + 1);
  int64_t* ps = pos.ensure(n + 1);
  const int64_t p1 = B.p1;
  parallel_for(s, n, PFV_LAMBDA(int64_t r) {
    int m = 0;
    for (int e = ip[p0 + r]; e < ip[p0 + r + 1]; ++e) m += (ix[e] >= p0 && ix[e] < p1) ? 1 : 0;
    ln[r] = m;
  });
  exclusive_scan<int32_t, int64_t>(s, c.scratch, ln, ps, (size_t)n);
  const int64_t nnz = read_scalar<int64_t>(s, ps + n);
  if (nnz >= (int64_t(1) << 31)) throw Error(PFV_ERR_UNSUPPORTED, "block with more than 2^31 entries");
  B.P.nrows = B.P.ncols = n;
  B.P.nnz = nnz;
  int32_t* bip = B.P.indptr.ensure(n + 1);
  int32_t* bix = B.P.indices.ensure(std::max<int64_t>(nnz, 1));
  double* bv = B.val.ensure(std::max<int64_t>(nnz, 1));
  double* bd = B.diag.ensure(n);
  int32_t* st = c.status.ensure(16);
  be_memset(st + 11, 0, 2 * sizeof(int32_t), s);
  parallel_for(s, n + 1, PFV_LAMBDA(int64_t r) { bip[r] = (int32_t)ps[r]; });
  parallel_for(s, n, PFV_LAMBDA(int64_t r) {
    int64_t o = ps[r];
    double d = 0.0;
    int prev = -1;
    bool descends = false;
    for (int e = ip[p0 + r]; e < ip[p0 + r + 1]; ++e) {
      const int cc = ix[e];
      descends = descends || cc < prev;
      prev = cc;
      if (cc >= p0 && cc < p1) {
        bix[o] = (int32_t)(cc - p0);
        bv[o] = val[e];
        if (cc == p0 + r) d = val[e];
        ++o;
      }
    }
    bd[r] = d;
    if (!(d != 0.0)) atomic_max_i32(st + 11, 1);
    if (descends) atomic_max_i32(st + 12, 1);
  });
  int32_t hst[2];
  be_d2h(hst, st + 11, sizeof(hst), s);
  B.ascending = hst[1] == 0;
  if (hst[0])
    throw Error(PFV_ERR_ARGUMENT, "block preconditioner: a diagonal entry is zero (permute the rows first: "
                                  "porepy_amd.solvers.match_rows)");
  B.P.max_row = 0;
}

static void blockpc_setup(pfv_ctx_impl& c, BlockPc& M, const CsrPattern& P, const double* val) {
  Timer tm;
  tm.start(c.stream);
  const size_t nb = M.ptr.size() - 1;
  while (M.blk.size() < nb) M.blk.push_back(std::make_unique<BlockPc::Blk>());
  M.blk.resize(nb);
  for (size_t k = 0; k < nb; ++k) {
    BlockPc::Blk& B = *M.blk[k];
    B.p0 = M.ptr[k];
    B.p1 = M.ptr[k + 1];
    blockpc_extract(c, P, val, B);
    if (!B.amg) B.amg = std::make_unique<Amg>();
    B.amg->valid = false;
    B.amg->coarse_target = kAmgDenseMax;  // blocks up to kAmgDenseMax rows: exact
    // ... so their one level is the block itself, not its strength-filtered copy (whose inverse is not the block's;
    // the filter pays on the levels of a cycle, and these blocks have none)
    B.amg->no_filter = B.p1 - B.p0 <= kAmgDenseMax;
    amg_setup(c, *B.amg, B.P, B.val, 1, B.diag, nullptr);
  }
  M.for_val = val;
  M.setup_ms = tm.stop(c.stream);
}

static void blockpc_apply(pfv_ctx_impl& c, BlockPc& M, const CsrPattern& P, const double* val, int64_t n,
                          const double* in, double* out) {
  stream_t s = c.stream;
  const int32_t* ip = P.indptr;
  const int32_t* ix = P.indices;
  double* t = M.tmp.ensure(n);
  for (size_t k = 0; k < M.blk.size(); ++k) {
    BlockPc::Blk& B = *M.blk[k];
    const int64_t p0 = B.p0, nk = B.p1 - B.p0;
    const double* rhs = in + p0;
    if (M.gs && k > 0) {
      // t_k = r_k - sum_{j < k} A_kj z_j: every entry of the block's rows left of the block, in storage order (rows with
      // ascending columns stop at the first entry that is not; pfv_set_system does not ask for sorted rows)
      const bool ascending = B.ascending;
      parallel_for(s, nk, PFV_LAMBDA(int64_t r) {
        double sum = 0.0;
        for (int e = ip[p0 + r]; e < ip[p0 + r + 1]; ++e) {
          const int cc = ix[e];
          if (cc >= p0) {
            if (ascending) break;
            continue;
          }
          sum += val[e] * out[cc];
        }
        t[p0 + r] = in[p0 + r] - sum;
      });
      rhs = t + p0;
    }
    double* z = amg_cycle(c, *B.amg, 0, rhs, out + p0);
    if (z != out + p0) be_d2d(out + p0, z, sizeof(double) * (size_t)nk, s);
  }
}

// ---- preconditioner handle used by the Krylov loops
struct AmgNns;  // amg_nns.inc
static void amg_nns_cycle(pfv_ctx_impl& c, AmgNns& H, size_t l, const double* b, double* x);
struct Sweep;  // sweep.inc
static void sweep_apply(pfv_ctx_impl& c, const Sweep& sw, const CsrPattern& P, const double* val, const double* diag,
                        const double* in, double* out);
struct Precond {
  Amg* amg = nullptr;          // nullptr: Jacobi
  const Sweep* sweep = nullptr;  // flow-ordered sweep (PFV_PRECOND_SWEEP; takes precedence; couples through P / val / diag)
  AmgNns* nns = nullptr;       // aggregation AMG with a near-null space (PFV_PRECOND_AMG_NNS)
  const double* diag = nullptr;
  BlockPc* blocks = nullptr;   // block lower-triangular preconditioner (takes precedence)
  const CsrPattern* P = nullptr;  // ... and the system it couples through
  const double* val = nullptr;
};
static void precond_apply(pfv_ctx_impl& c, const Precond& M, int64_t n, const double* in, double* out) {
  if (M.sweep) {
    sweep_apply(c, *M.sweep, *M.P, M.val, M.diag, in, out);
  } else if (M.blocks) {
    blockpc_apply(c, *M.blocks, *M.P, M.val, n, in, out);
  } else if (M.nns) {
    amg_nns_cycle(c, *M.nns, 0, in, out);
  } else if (M.amg && M.amg->dist) {
    amg_apply_dist(c, *M.amg, in, out);
  } else if (M.amg) {
    amg_cycle(c, *M.amg, 0, in, out);
  } else {
    const double* d = M.diag;
    parallel_for(c.stream, n, PFV_LAMBDA(int64_t i) { out[i] = in[i] / d[i]; });
  }
}
// The first smoothing step of the plain AMG's cycle, x0 = omega D^-1 in with the finest level's omega and dinv, for a
// caller that forms it in the kernel that writes `in` and then calls amg_cycle with x_is_presmoothed (krylov_solve:
// the two updates of BiCGStab; PFV_AMG_KRYLOV_PRESMOOTH).  false: M is no such preconditioner -- precond_apply.
static bool precond_presmooth(const Precond& M, const double*& dinv, double& omega) {
  if (M.sweep || M.blocks || M.nns || !M.amg || M.amg->dist || !M.amg->valid) return false;
  const Amg& amg = *M.amg;
  if (!amg.sw.krylov_presmooth || !amg.ap_ok || amg.nlev < 2 || amg_level_path(amg, 0).small) return false;
  dinv = amg.lev[0]->dinv;
  omega = amg.lev[0]->omega;
  return true;
}

}  // namespace pfv
