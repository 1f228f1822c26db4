// amg_nns.inc — aggregation AMG whose tentative prolongator carries a near-null space (PFV_PRECOND_AMG_NNS).
//
// The plain hierarchy of amg.inc prolongates block systems with P = P_cell (x) I_bs: every aggregate carries the bs
// translations only.  For linear elasticity the rotations are near-null modes too, and a coarse level that cannot
// represent them costs iterations (MPSA, configs[3]: 44 BiCGStab iterations).  Here the caller hands k modes B (n x k;
// rigid-body modes of the grid when built on the device), and per level l (block size bs_l: bs on level 0, k below):
//   * aggregates: pairwise matching passes on the cell graph (amg_pairwise; the strength filter on level 0 only);
//   * tentative prolongator: per aggregate the thin QR of its (m bs_l) x k slice of B_l, P_l rows = Q_a,
//     B_{l+1} block a = R_a (one wavefront per aggregate, modified Gram-Schmidt applied twice, FP64);
//   * Galerkin product A_{l+1} = P_l^T A_l P_l with full k x k blocks: the block pattern is the Galerkin product of the
//     cell graph (amg_galerkin with piecewise-constant aggregation), the values one wavefront per coarse block row,
//     summed in LDS in a fixed order (no floating-point atomics: two setups give the same bits);
//   * damped block-Jacobi smoother (bs_l x bs_l diagonal blocks inverted in the setup), dense inverse on the coarsest.
// The cycle: pre-smoothing, residual, restriction P^T r, coarse correction (first coarse level visited twice on large
// systems, as in amg.inc), prolongation x += alpha P x_c, post-smoothing.  The state is separate from the plain
// hierarchy (pfv_ctx_impl::amg): setting or clearing the modes never touches it.

namespace pfv {

constexpr int kNnsMaxModes = 8;          // k of pfv_set_near_null_space (one wavefront holds a k x k block)
constexpr int kNnsPasses = 3;            // matching passes on level 0 (aggregates of ~8 cells: >= 4 for 6 modes in 3-D)
constexpr int kNnsPassesCoarse = 2;      // ... below it
constexpr int kNnsCoarseTarget = 512;    // stop coarsening at this many rows (dense inverse below kAmgDenseMax)
constexpr double kNnsDropTol = 1e-10;    // a QR column whose norm falls below this fraction of its own is dropped

struct NnsLevel {
  int64_t n = 0, cells = 0;  // rows, cells (n = cells * bs)
  int bs = 1;
  const CsrPattern* P = nullptr;  // this level's matrix (level 0: the system)
  const double* val = nullptr;
  CsrPattern P_own;
  Buf<double> val_own;
  Buf<float> val32;
  const float* v32 = nullptr;
  Buf<double> dblk;                // [cells][bs][bs] inverses of the diagonal blocks
  Buf<double> B;                   // [n][k] near-null space of this level (row-major)
  Buf<int32_t> agg, mptr, mem;     // cell -> aggregate, members of every aggregate (ascending)
  int64_t nagg = 0;                // aggregates (coarse cells); 0 on the coarsest level
  Buf<double> Pt;                  // [n][k] tentative prolongator
  Buf<double> Bc;                  // [nagg * k][k] the next level's near-null space (R of the QR)
  Buf<int32_t> zc;                 // [nagg * k] 1: that column of Q was dropped (rank deficiency)
  Buf<double> x, b, t, r2, x2;     // cycle vectors
};

// The switches of one setup: read in ONE place, nns_read_switches, at the start of every setup; amg_nns_cfg hashes them.
struct NnsSwitches {
  int passes = kNnsPasses, passes_coarse = kNnsPassesCoarse;  // PFV_AMG_NNS_PASSES, _PASSES_COARSE: 1..6
  int omega_pct = 70, alpha_pct = 130;                        // PFV_AMG_NNS_OMEGA_PCT, _ALPHA_PCT
  bool fp32 = true;                                           // PFV_AMG_NNS_FP32
  // PFV_AMG_NNS_GAMMA as given: the default follows the size of the system (amg_nns_setup resolves and clamps to 1..2)
  bool gamma_set = false;
  int gamma_raw = 0;
  int gamma_levels = 1;                    // PFV_AMG_NNS_GAMMA_LEVELS, >= 1
  int sweeps = 1;                          // PFV_AMG_NNS_SWEEPS, 1..4
  int coarse_target = kNnsCoarseTarget;    // PFV_AMG_NNS_COARSE_TARGET, 1..kAmgDenseMax
  int filter_permil = 0;                   // PFV_AMG_NNS_FILTER_PERMIL (block sizes above 4: no filter)
};

static NnsSwitches nns_read_switches(int bs) {
  NnsSwitches w;
  w.passes = std::max(1, std::min(6, env_int("PFV_AMG_NNS_PASSES", kNnsPasses)));
  w.passes_coarse = std::max(1, std::min(6, env_int("PFV_AMG_NNS_PASSES_COARSE", kNnsPassesCoarse)));
  w.omega_pct = env_int("PFV_AMG_NNS_OMEGA_PCT", 70);
  w.alpha_pct = env_int("PFV_AMG_NNS_ALPHA_PCT", 130);
  w.fp32 = env_int("PFV_AMG_NNS_FP32", 1) != 0;
  const char* gamma = std::getenv("PFV_AMG_NNS_GAMMA");
  w.gamma_set = gamma != nullptr;
  if (gamma) w.gamma_raw = std::atoi(gamma);
  w.gamma_levels = std::max(1, env_int("PFV_AMG_NNS_GAMMA_LEVELS", 1));
  w.sweeps = std::max(1, std::min(4, env_int("PFV_AMG_NNS_SWEEPS", 1)));
  w.coarse_target = std::max(1, std::min(kAmgDenseMax, env_int("PFV_AMG_NNS_COARSE_TARGET", kNnsCoarseTarget)));
  const int permil = env_int("PFV_AMG_NNS_FILTER_PERMIL", bs == 1 ? kAmgFilterPermil : kAmgFilterPermilBlock);
  w.filter_permil = bs <= 4 ? permil : 0;
  return w;
}

// the switches a hierarchy is built with, in one word (a changed effective value rebuilds it; PFV_AMG_NNS_GAMMA, whose
// default follows the size, as given)
static unsigned long long amg_nns_cfg(int bs) {
  const NnsSwitches w = nns_read_switches(bs);
  unsigned long long h = 1469598103934665603ull;
  for (int v : {w.passes, w.passes_coarse, w.omega_pct, w.alpha_pct, (int)w.fp32, w.gamma_set ? w.gamma_raw : -1,
                (int)w.gamma_set, w.gamma_levels, w.sweeps, w.coarse_target, w.filter_permil})
    h = (h ^ (unsigned long long)(v + 7)) * 1099511628211ull;
  return h;
}

struct AmgNns {
  std::vector<std::unique_ptr<NnsLevel>> lev;
  size_t nlev = 0;
  AmgWork wk;
  AmgSwitches plain;  // the plain hierarchy's switches the shared helpers read (matching, Galerkin pattern, filter, dense inverse)
  int k = 0;
  int passes = kNnsPasses, passes_coarse = kNnsPassesCoarse;
  double omega = 0.7, alpha = 1.3, filter_theta = 0.0;
  int gamma = 1, gamma_levels = 1;  // levels l < gamma_levels visit their coarse level gamma times
  int sweeps = 1;                    // smoothing steps before and after the coarse correction
  bool fp32 = true;
  CsrPattern filtP, cellP, cellC;  // filtered finest matrix, cell graph of a level, its aggregated graph
  Buf<double> filtV, ones, cellCV, cellCD;
  Buf<double> dense;
  bool dense_ok = false, valid = false;
  double setup_ms = 0.0, op_complexity = 0.0;
};

// cell graph of a matrix of full bs x bs blocks: cell i's neighbours are the block columns of its first row
static void nns_cell_graph(pfv_ctx_impl& c, AmgNns& H, const CsrPattern& A, int bs) {
  stream_t s = c.stream;
  const int64_t cells = A.nrows / bs, nb = A.nnz / ((int64_t)bs * bs);
  const int32_t* ip = A.indptr;
  const int32_t* ix = A.indices;
  int32_t* cp = H.cellP.indptr.ensure(cells + 1);
  int32_t* cx = H.cellP.indices.ensure(std::max<int64_t>(nb, 1));
  double* one = H.ones.ensure(std::max<int64_t>(nb, 1));
  parallel_for(s, cells + 1, PFV_LAMBDA(int64_t i) { cp[i] = ip[i * bs] / (bs * bs); });
  parallel_for(s, cells, PFV_LAMBDA(int64_t i) {
    const int p0 = ip[i * bs], q0 = p0 / (bs * bs), m = (ip[i * bs + 1] - p0) / bs;
    for (int kb = 0; kb < m; ++kb) {
      cx[q0 + kb] = ix[p0 + kb * bs] / bs;
      one[q0 + kb] = 1.0;
    }
  });
  H.cellP.nrows = H.cellP.ncols = cells;
  H.cellP.nnz = nb;
  H.cellP.max_row = A.max_row;
}

// Tentative prolongator of one level: for every aggregate a (one wavefront) the thin QR of the rows of its members in
// B (row-major [n][k]), Q_a -> Pt, R_a -> Bc rows a k .. a k + k - 1.  Modified Gram-Schmidt, every projection applied
// twice.  Rank deficiency (a singleton aggregate of 3 rows carrying 6 modes, modes that coincide on an aggregate): a
// column whose norm after the projections is below kNnsDropTol times its norm before becomes a zero column of Q, its
// row of R is zero and zc marks the coarse unknown -- the Galerkin kernel puts a unit entry on its diagonal, so the
// coarse matrix stays non-singular (the dense coarsest inverse and the block-Jacobi blocks need that).
// cc (level 0 of device-made rigid-body modes, [3][cells] in the system's numbering, else nullptr): the rotations are
// orthogonalised about the aggregate's centroid -- coordinates far from the origin (~1e6 against metre-sized
// aggregates) would otherwise lose their digits to the cancellation against the translations --, and R is turned back
// into the coefficients of the modes about the origin (a rotation about the centroid differs from one about the
// origin by a translation), so that P B_{l+1} = B_l holds for the B the caller sees.
static void nns_tentative(pfv_ctx_impl& c, NnsLevel& L, int k, const double* cc = nullptr, int nd = 0) {
  stream_t s = c.stream;
  const int bs = L.bs;
  const int64_t nagg = L.nagg;
  const int32_t* mptr = L.mptr;
  const int32_t* mem = L.mem;
  const double* B = L.B;
  double* Pt = L.Pt.ensure(std::max<int64_t>(L.n * k, 1));
  double* Bc = L.Bc.ensure(std::max<int64_t>(nagg * k * k, 1));
  int32_t* zc = L.zc.ensure(std::max<int64_t>(nagg * k, 1));
  const int64_t ncell = L.cells;
  const size_t lds = sizeof(double) * (64 + kNnsMaxModes * kNnsMaxModes + 2) + 16;
  wave_for(s, nagg, lds, PFV_LAMBDA(const WaveCtx& w) {
    const int64_t a = w.item;
    double* part = reinterpret_cast<double*>(w.lds);  // [64] per-lane partial sums
    double* R = part + 64;                            // [k][k]
    double* bc = R + kNnsMaxModes * kNnsMaxModes;     // [1] broadcast
    const int q0 = mptr[a], nr = (mptr[a + 1] - q0) * bs;
    auto row = [&](int t) -> int64_t { return (int64_t)mem[q0 + t / bs] * bs + (t % bs); };
    // <col u, col v> over the aggregate's rows, lanes in order (deterministic)
    auto dot = [&](int u, int v) -> double {
      double p = 0.0;
      PFV_LANES(t, nr) {
        const int64_t r = row(t);
        p += Pt[r * k + u] * Pt[r * k + v];
      }
      part[w.lane] = p;
      w.sync();
      if (w.lane0()) {
        double sum = 0.0;
        for (int l = 0; l < w.width; ++l) sum += part[l];
        bc[0] = sum;
      }
      w.sync();
      const double d = bc[0];
      w.sync();
      return d;
    };
    PFV_LANES(t, nr) {
      const int64_t r = row(t);
      for (int j = 0; j < k; ++j) Pt[r * k + j] = B[r * k + j];
    }
    PFV_LANES(t, k * k) R[t] = 0.0;
    w.sync();
    double cen[3] = {0.0, 0.0, 0.0};
    if (cc) {
      const int m = mptr[a + 1] - q0;
      for (int d = 0; d < nd; ++d) {  // centroid of the members' centres, lanes in order
        double p = 0.0;
        PFV_LANES(q, m) p += cc[d * ncell + mem[q0 + q]];
        part[w.lane] = p;
        w.sync();
        if (w.lane0()) {
          double sum = 0.0;
          for (int l = 0; l < w.width; ++l) sum += part[l];
          bc[0] = sum / m;
        }
        w.sync();
        cen[d] = bc[0];
        w.sync();
      }
      PFV_LANES(t, nr) {
        const int64_t r = row(t);
        const int64_t i = r / nd;
        const int comp = (int)(r - i * nd);
        const double x = cc[i] - cen[0], y = cc[ncell + i] - cen[1], z = nd == 3 ? cc[2 * ncell + i] - cen[2] : 0.0;
        if (nd == 2) {
          Pt[r * k + 2] = comp == 0 ? -y : x;
        } else {
          const double rx[3] = {0.0, -z, y}, ry[3] = {z, 0.0, -x}, rz[3] = {-y, x, 0.0};
          Pt[r * k + 3] = rx[comp];
          Pt[r * k + 4] = ry[comp];
          Pt[r * k + 5] = rz[comp];
        }
      }
      w.sync();
    }
    for (int j = 0; j < k; ++j) {
      const double n0 = sqrt(dot(j, j));
      for (int sweep = 0; sweep < 2; ++sweep) {
        for (int i = 0; i < j; ++i) {
          if (R[i * k + i] == 0.0) continue;  // (dropped column)
          const double d = dot(i, j);
          PFV_LANES(t, nr) {
            const int64_t r = row(t);
            Pt[r * k + j] -= d * Pt[r * k + i];
          }
          if (w.lane0()) R[i * k + j] += d;
          w.sync();
        }
      }
      const double n1 = sqrt(dot(j, j));
      const bool drop = !(n1 > kNnsDropTol * n0);
      const double sc = drop ? 0.0 : 1.0 / n1;
      PFV_LANES(t, nr) {
        const int64_t r = row(t);
        Pt[r * k + j] *= sc;
      }
      if (w.lane0()) {
        R[j * k + j] = drop ? 0.0 : n1;
        if (drop)
          for (int jj = j + 1; jj < k; ++jj) R[j * k + jj] = 0.0;
        zc[a * k + j] = drop ? 1 : 0;
      }
      w.sync();
    }
    if (cc && w.lane0()) {
      // back to rotations about the origin: rot = rot_centroid + sum_t coef_t translation_t
      const double xc = cen[0], yc = cen[1], zc0 = cen[2];
      double coef[3][3] = {{0.0, 0.0, 0.0}, {0.0, 0.0, 0.0}, {0.0, 0.0, 0.0}};  // [rotation][translation]
      int nrot = 1;
      if (nd == 2) {
        coef[0][0] = -yc;
        coef[0][1] = xc;
      } else {
        nrot = 3;
        coef[0][1] = -zc0; coef[0][2] = yc;
        coef[1][0] = zc0;  coef[1][2] = -xc;
        coef[2][0] = -yc;  coef[2][1] = xc;
      }
      for (int q = 0; q < nrot; ++q)
        for (int i = 0; i < k; ++i) {
          double add = 0.0;
          for (int t = 0; t < nd; ++t) add += coef[q][t] * R[i * k + t];
          R[i * k + nd + q] += add;
        }
    }
    w.sync();
    PFV_LANES(t, k * k) Bc[a * k * k + t] = R[t];
    w.sync();
  });
}

// A_{l+1} = P_l^T A_l P_l.  Pattern: the Galerkin product of the cell graph (H.cellC, sorted block columns per coarse
// cell).  Values: one wavefront per coarse cell I; lane t < k^2 owns entry (p, q) = (t / k, t % k) of every block of
// the row and walks the members of I and their block columns in order, adding (P_i^T A_ij P_j)_pq to the LDS slot of
// the block column agg(j) -- the same additions in the same order on every run.
static void nns_galerkin(pfv_ctx_impl& c, AmgNns& H, NnsLevel& L, NnsLevel& Ln) {
  stream_t s = c.stream;
  const int bs = L.bs, k = H.k, kk = k * k;
  const int64_t nagg = L.nagg;
  nns_cell_graph(c, H, *L.P, bs);
  amg_galerkin(c, H.plain, H.wk, H.cellP, H.ones.p, 1, L.agg, L.mptr, L.mem, nagg, H.cellC, H.cellCV, H.cellCD, nullptr);
  const int32_t* cp = H.cellC.indptr;
  const int32_t* cx = H.cellC.indices;
  int32_t* st = c.status.ensure(16);
  be_memset(st + 8, 0, sizeof(int32_t), s);
  parallel_for(s, nagg, PFV_LAMBDA(int64_t I) { track_max_i32(st + 8, cp[I + 1] - cp[I]); });
  const int maxcol = std::max(1, read_scalar<int32_t>(s, st + 8));
  const size_t lds = sizeof(double) * (size_t)maxcol * kk + sizeof(int32_t) * (size_t)maxcol + 16;
  if (lds > 150 * 1024) throw Error(PFV_ERR_UNSUPPORTED, "AMG near-null space: a coarse block row too wide for LDS");
  const int64_t nbc = H.cellC.nnz;
  if (nbc * kk >= (int64_t(1) << 31)) throw Error(PFV_ERR_UNSUPPORTED, "AMG near-null space: coarse matrix with more than 2^31 entries");
  const int64_t ncr = nagg * k;
  Ln.n = ncr;
  Ln.cells = nagg;
  Ln.bs = k;
  CsrPattern& C = Ln.P_own;
  C.nrows = C.ncols = ncr;
  C.nnz = nbc * kk;
  C.max_row = maxcol * k;
  int32_t* rp = C.indptr.ensure(ncr + 1);
  int32_t* rx = C.indices.ensure(std::max<int64_t>(C.nnz, 1));
  double* rv = Ln.val_own.ensure(std::max<int64_t>(C.nnz, 1));
  parallel_for(s, ncr + 1, PFV_LAMBDA(int64_t R) {
    const int64_t I = R / k;
    const int p = (int)(R - I * k);
    rp[R] = I < nagg ? (int32_t)((int64_t)cp[I] * kk + (int64_t)p * (cp[I + 1] - cp[I]) * k) : (int32_t)((int64_t)cp[I] * kk);
  });
  const int32_t* ip = L.P->indptr;
  const int32_t* ix = L.P->indices;
  const double* av = L.val;
  const double* Pt = L.Pt;
  const int32_t* agg = L.agg;
  const int32_t* mptr = L.mptr;
  const int32_t* mem = L.mem;
  const int32_t* zc = L.zc;
  wave_for(s, nagg, lds, PFV_LAMBDA(const WaveCtx& w) {
    const int64_t I = w.item;
    double* acc = reinterpret_cast<double*>(w.lds);
    int32_t* col = reinterpret_cast<int32_t*>(acc + (size_t)maxcol * kk);
    const int c0 = cp[I], nc = cp[I + 1] - c0;
    PFV_LANES(t, nc) col[t] = cx[c0 + t];
    PFV_LANES(t, nc * kk) acc[t] = 0.0;
    w.sync();
    for (int q = mptr[I]; q < mptr[I + 1]; ++q) {
      const int64_t i = mem[q];
      const int p0 = ip[i * bs], m = (ip[i * bs + 1] - p0) / bs;
      for (int kb = 0; kb < m; ++kb) {
        const int64_t j = ix[p0 + kb * bs] / bs;
        const int J = agg[j];
        int lo = 0, hi = nc - 1;  // position of J among the sorted block columns
        while (lo < hi) {
          const int mid = (lo + hi) >> 1;
          if (col[mid] < J) lo = mid + 1; else hi = mid;
        }
        PFV_LANES(t, kk) {
          const int p = t / k, qq = t - (t / k) * k;
          double sum = 0.0;
          for (int a = 0; a < bs; ++a) {
            const int ra = ip[i * bs + a] + kb * bs;
            double inner = 0.0;
            for (int b = 0; b < bs; ++b) inner += av[ra + b] * Pt[(j * bs + b) * k + qq];
            sum += Pt[(i * bs + a) * k + p] * inner;
          }
          acc[lo * kk + t] += sum;
        }
      }
    }
    w.sync();
    PFV_LANES(e, nc * kk) {
      const int pos = e / kk, t = e - pos * kk;
      const int p = t / k, qq = t - p * k;
      double v = acc[e];
      if (col[pos] == (int32_t)I && p == qq && zc[I * k + p]) v += 1.0;  // dropped mode: unit diagonal
      const int64_t o = (int64_t)c0 * kk + (int64_t)p * nc * k + (int64_t)pos * k + qq;
      rx[o] = col[pos] * k + qq;
      rv[o] = v;
    }
    w.sync();
  });
  Ln.P = &Ln.P_own;
  Ln.val = Ln.val_own.p;
}

// inverses of the bs x bs diagonal blocks (Gauss-Jordan with partial pivoting, FP64); a singular block gets the
// inverse of its diagonal instead (zeros where the diagonal is zero)
static void nns_block_inverse(pfv_ctx_impl& c, NnsLevel& L) {
  const int bs = L.bs;
  const int32_t* ip = L.P->indptr;
  const int32_t* ix = L.P->indices;
  const double* v = L.val;
  double* dinv = L.dblk.ensure(std::max<int64_t>(L.cells * bs * bs, 1));
  parallel_for(c.stream, L.cells, PFV_LAMBDA(int64_t i) {
    double a[kNnsMaxModes][2 * kNnsMaxModes];
    const int p0 = ip[i * bs], m = (ip[i * bs + 1] - p0) / bs;
    int kd = -1;
    for (int kb = 0; kb < m; ++kb)
      if (ix[p0 + kb * bs] / bs == (int32_t)i) kd = kb;
    for (int r = 0; r < bs; ++r)
      for (int q = 0; q < 2 * bs; ++q)
        a[r][q] = q < bs ? (kd >= 0 ? v[ip[i * bs + r] + kd * bs + q] : 0.0) : (q - bs == r ? 1.0 : 0.0);
    bool ok = true;
    for (int col = 0; col < bs && ok; ++col) {
      int pr = col;
      for (int r = col + 1; r < bs; ++r)
        if (fabs(a[r][col]) > fabs(a[pr][col])) pr = r;
      if (!(fabs(a[pr][col]) > 0.0)) { ok = false; break; }
      if (pr != col)
        for (int q = 0; q < 2 * bs; ++q) { const double tmp = a[col][q]; a[col][q] = a[pr][q]; a[pr][q] = tmp; }
      const double inv = 1.0 / a[col][col];
      for (int q = 0; q < 2 * bs; ++q) a[col][q] *= inv;
      for (int r = 0; r < bs; ++r) {
        if (r == col) continue;
        const double f = a[r][col];
        if (f != 0.0)
          for (int q = 0; q < 2 * bs; ++q) a[r][q] -= f * a[col][q];
      }
    }
    double* out = dinv + i * bs * bs;
    for (int r = 0; r < bs; ++r)
      for (int q = 0; q < bs; ++q) {
        if (ok) out[r * bs + q] = a[r][bs + q];
        else {
          const double d = kd >= 0 ? v[ip[i * bs + r] + kd * bs + r] : 0.0;
          out[r * bs + q] = (r == q && d != 0.0) ? 1.0 / d : 0.0;
        }
      }
  });
}

// matching passes on the cell graph of (G, gv) with block size bs: L.agg, L.nagg, member lists.  Returns false when
// the coarsening stalled (this level is then the coarsest).
static bool nns_aggregate(pfv_ctx_impl& c, AmgNns& H, NnsLevel& L, const CsrPattern& G, const double* gv, int passes) {
  stream_t s = c.stream;
  AmgWork& wk = H.wk;
  const int bs = L.bs;
  const int64_t cells = L.cells;
  int32_t* aggL = L.agg.ensure(std::max<int64_t>(cells, 1));
  const CsrPattern* curP = &G;
  const double* curV = gv;
  int64_t cur = cells;
  int slot = 0;
  bool any = false;
  for (int pass = 0; pass < passes; ++pass) {
    const int64_t nagg = amg_pairwise(c, H.plain, wk, *curP, curV, bs, wk.a1);
    if (nagg >= cur) break;
    const int32_t* a1 = wk.a1;
    if (!any) parallel_for(s, cells, PFV_LAMBDA(int64_t i) { aggL[i] = a1[i]; });
    else parallel_for(s, cells, PFV_LAMBDA(int64_t i) { aggL[i] = a1[aggL[i]]; });
    any = true;
    if (pass + 1 < passes && nagg * bs > kNnsCoarseTarget) {
      // the aggregated graph the next pass matches on (piecewise-constant Galerkin product, bs kept)
      amg_members(c, wk, a1, cur, nagg, wk.mp, wk.me);
      amg_galerkin(c, H.plain, wk, *curP, curV, bs, a1, wk.mp, wk.me, nagg, wk.P[slot], wk.V[slot], wk.D[slot], nullptr);
      curP = &wk.P[slot];
      curV = wk.V[slot].p;
      slot = 1 - slot;
      cur = nagg;
    } else {
      cur = nagg;
      break;
    }
  }
  if (!any || cur > 0.85 * cells) return false;
  L.nagg = cur;
  amg_members(c, wk, aggL, cells, cur, L.mptr, L.mem);
  return true;
}

// B0: the level-0 near-null space, row-major [n][k], in the numbering of the system the hierarchy is built for
// cc0: cell centres ([3][cells], the system's numbering) when B0 holds the device-made rigid-body modes, else nullptr
static void amg_nns_setup(pfv_ctx_impl& c, AmgNns& H, const CsrPattern& A, const double* val, int bs, int k,
                          const double* B0, const double* cc0 = nullptr) {
  stream_t s = c.stream;
  Timer tm;
  tm.start(s);
  H.valid = H.dense_ok = false;
  H.k = k;
  if (k < 1 || k > kNnsMaxModes) throw Error(PFV_ERR_UNSUPPORTED, "AMG near-null space: 1 to 8 modes");
  if (bs < 1 || bs > kNnsMaxModes || A.nrows % bs) throw Error(PFV_ERR_ARGUMENT, "AMG near-null space: bad block size");
  const NnsSwitches w = nns_read_switches(bs);
  H.plain = amg_read_switches(bs);
  H.passes = w.passes;
  H.passes_coarse = w.passes_coarse;
  H.omega = 0.01 * w.omega_pct;
  H.alpha = 0.01 * w.alpha_pct;
  H.fp32 = w.fp32;
  H.gamma = std::max(1, std::min(2, w.gamma_set ? w.gamma_raw : (A.nrows >= kAmgWTopRows ? 2 : 1)));
  H.gamma_levels = w.gamma_levels;
  H.sweeps = w.sweeps;
  H.filter_theta = 0.001 * w.filter_permil;
  if (bs > 1) {  // full bs x bs blocks (the cell graph and the Galerkin kernel address them so)
    const int32_t* ip = A.indptr;
    int32_t* st = c.status.ensure(16);
    be_memset(st + 10, 0, sizeof(int32_t), s);
    const int32_t* ix = A.indices;
    parallel_for(s, A.nrows / bs, PFV_LAMBDA(int64_t i) {
      const int len = ip[i * bs + 1] - ip[i * bs];
      bool bad = (len % bs) != 0;
      for (int a = 1; a < bs; ++a) bad = bad || (ip[i * bs + a + 1] - ip[i * bs + a]) != len;
      // ... and every block's bs columns aligned and the same in the bs rows of the cell
      for (int e = 0; e < len && !bad; ++e) {
        const int32_t c0 = ix[ip[i * bs] + e - e % bs];
        for (int a = 0; a < bs && !bad; ++a) bad = c0 % bs != 0 || ix[ip[i * bs + a] + e] != c0 + e % bs;
      }
      if (bad) atomic_max_i32(st + 10, 1);
    });
    if (read_scalar<int32_t>(s, st + 10))
      throw Error(PFV_ERR_UNSUPPORTED, "AMG: the matrix is not made of full, aligned blocks of the given block size");
  }
  auto level = [&](size_t l) -> NnsLevel& {
    while (H.lev.size() <= l) H.lev.push_back(std::make_unique<NnsLevel>());
    return *H.lev[l];
  };
  {
    NnsLevel& L0 = level(0);
    L0.n = A.nrows;
    L0.bs = bs;
    L0.cells = A.nrows / bs;
    L0.P = &A;
    L0.val = val;
    be_d2d(L0.B.ensure(std::max<int64_t>(L0.n * k, 1)), B0, sizeof(double) * (size_t)(L0.n * k), s);
  }
  double nnz_sum = 0.0;
  size_t l = 0;
  while (true) {
    NnsLevel& L = level(l);
    nnz_sum += (double)L.P->nnz;
    L.nagg = 0;
    nns_block_inverse(c, L);
    L.t.ensure(std::max<int64_t>(L.n, 1));
    if (l > 0) {
      L.x.ensure(L.n);
      L.b.ensure(L.n);
    }
    L.v32 = nullptr;
    if (H.fp32) {
      float* v32 = L.val32.ensure(std::max<int64_t>(L.P->nnz, 1));
      const double* v64 = L.val;
      parallel_for(s, L.P->nnz, PFV_LAMBDA(int64_t e) { v32[e] = (float)v64[e]; });
      L.v32 = v32;
    }
    if (L.n <= w.coarse_target || (int)l + 1 >= kAmgMaxLevels) break;
    const CsrPattern* G = L.P;
    const double* gv = L.val;
    if (l == 0 && H.filter_theta > 0.0) {  // strength filter (amg.inc: amg_filter) for the matching only
      amg_filter(c, H.plain, *L.P, L.val, H.filter_theta, H.filtP, H.filtV, H.wk, bs);
      G = &H.filtP;
      gv = H.filtV.p;
    }
    if (!nns_aggregate(c, H, L, *G, gv, l == 0 ? H.passes : H.passes_coarse)) break;
    nns_tentative(c, L, k, l == 0 ? cc0 : nullptr, bs);
    NnsLevel& Ln = level(l + 1);
    nns_galerkin(c, H, L, Ln);
    be_d2d(Ln.B.ensure(std::max<int64_t>(Ln.n * k, 1)), L.Bc.p, sizeof(double) * (size_t)(Ln.n * k), s);
    ++l;
  }
  H.nlev = l + 1;
  NnsLevel& Lc = *H.lev[H.nlev - 1];
  if (Lc.n <= kAmgDenseMax) H.dense_ok = amg_dense_invert(c, H.plain, H.wk, *Lc.P, Lc.val, H.dense);
  H.op_complexity = nnz_sum / (double)std::max<int64_t>(A.nnz, 1);
  H.valid = true;
  if (env_int("PFV_DEBUG_AMG", 0)) {
    std::fprintf(stderr, "amg_nns_setup: k %d, levels:", k);
    for (size_t q = 0; q < H.nlev; ++q)
      std::fprintf(stderr, " %lld/%lld", (long long)H.lev[q]->n, (long long)H.lev[q]->P->nnz);
    std::fprintf(stderr, " dense %d\n", (int)H.dense_ok);
  }
  H.setup_ms = tm.stop(s);
}

// t = A_l x  (single-precision values when the hierarchy keeps them; vectors and sums in double)
static void nns_spmv(pfv_ctx_impl& c, const NnsLevel& L, const double* x, double* t) {
  if (L.v32) amg_spmv_t<float, 0>(c, *L.P, L.v32, x, t, nullptr, nullptr, 0.0);
  else amg_spmv_t<double, 0>(c, *L.P, L.val, x, t, nullptr, nullptr, 0.0);
}

// block-Jacobi step y = x + omega D^-1 (b - t); x == nullptr: x = 0 and t = 0 (y = omega D^-1 b).  y may be x.
static void nns_smooth(pfv_ctx_impl& c, const NnsLevel& L, double omega, const double* x, const double* b,
                       const double* t, double* y) {
  const int bs = L.bs;
  const double* D = L.dblk;
  parallel_for(c.stream, L.n, PFV_LAMBDA(int64_t r) {
    const int64_t i = r / bs;
    const int a = (int)(r - i * bs);
    const double* Dr = D + (i * bs + a) * bs;
    double sum = 0.0;
    for (int q = 0; q < bs; ++q) {
      const int64_t rq = i * bs + q;
      sum += Dr[q] * (x ? b[rq] - t[rq] : b[rq]);
    }
    y[r] = (x ? x[r] : 0.0) + omega * sum;
  });
}

// r_c = P^T (b - t): one wavefront per aggregate, lanes over its member rows, per-lane sums added in lane order
static void nns_restrict(pfv_ctx_impl& c, const NnsLevel& L, int k, const double* b, const double* t, double* rc) {
  const int bs = L.bs;
  const double* Pt = L.Pt;
  const int32_t* mptr = L.mptr;
  const int32_t* mem = L.mem;
  wave_for(c.stream, L.nagg, sizeof(double) * 64 * kNnsMaxModes + 16, PFV_LAMBDA(const WaveCtx& w) {
    const int64_t a = w.item;
    double* part = reinterpret_cast<double*>(w.lds);  // [k][64]
    const int q0 = mptr[a], nr = (mptr[a + 1] - q0) * bs;
    double acc[kNnsMaxModes];
    for (int p = 0; p < kNnsMaxModes; ++p) acc[p] = 0.0;
    PFV_LANES(e, nr) {
      const int64_t r = (int64_t)mem[q0 + e / bs] * bs + (e % bs);
      const double res = b[r] - t[r];
      for (int p = 0; p < k; ++p) acc[p] += Pt[r * k + p] * res;
    }
    for (int p = 0; p < k; ++p) part[p * 64 + w.lane] = acc[p];
    w.sync();
    PFV_LANES(p, k) {
      double sum = 0.0;
      for (int l = 0; l < w.width; ++l) sum += part[p * 64 + l];
      rc[a * k + p] = sum;
    }
    w.sync();
  });
}

// x += alpha P x_c: one thread per fine row (its cell's k coefficients, its aggregate's k coarse values)
static void nns_prolong(pfv_ctx_impl& c, const NnsLevel& L, int k, double alpha, const double* xc, double* x) {
  const int bs = L.bs;
  const double* Pt = L.Pt;
  const int32_t* agg = L.agg;
  parallel_for(c.stream, L.n, PFV_LAMBDA(int64_t r) {
    const int64_t I = agg[r / bs];
    double sum = 0.0;
    for (int p = 0; p < k; ++p) sum += Pt[r * k + p] * xc[I * k + p];
    x[r] += alpha * sum;
  });
}

// x = M_l b: one cycle from level l (x need not be initialised)
static void amg_nns_cycle(pfv_ctx_impl& c, AmgNns& H, size_t l, const double* b, double* x) {
  NnsLevel& L = *H.lev[l];
  double* t = L.t;
  if (l + 1 == H.nlev) {
    if (H.dense_ok) {
      amg_dense_apply(c, H.dense, L.n, b, x);
    } else {  // coarsening stalled above the dense limit: a few damped block-Jacobi sweeps
      nns_smooth(c, L, H.omega, nullptr, b, nullptr, x);
      for (int sweep = 0; sweep < 3; ++sweep) {
        nns_spmv(c, L, x, t);
        nns_smooth(c, L, H.omega, x, b, t, x);
      }
    }
    return;
  }
  NnsLevel& Ln = *H.lev[l + 1];
  const int k = H.k;
  nns_smooth(c, L, H.omega, nullptr, b, nullptr, x);
  for (int sweep = 1; sweep < H.sweeps; ++sweep) {
    nns_spmv(c, L, x, t);
    nns_smooth(c, L, H.omega, x, b, t, x);
  }
  nns_spmv(c, L, x, t);
  nns_restrict(c, L, k, b, t, Ln.b);
  amg_nns_cycle(c, H, l + 1, Ln.b, Ln.x);
  if ((int)l < H.gamma_levels && H.gamma == 2 && l + 2 < H.nlev) {
    // second visit of the first coarse level, on its residual
    double* r2 = Ln.r2.ensure(Ln.n);
    double* x2 = Ln.x2.ensure(Ln.n);
    nns_spmv(c, Ln, Ln.x, Ln.t);
    const double* bb = Ln.b;
    const double* tt = Ln.t;
    parallel_for(c.stream, Ln.n, PFV_LAMBDA(int64_t i) { r2[i] = bb[i] - tt[i]; });
    amg_nns_cycle(c, H, l + 1, r2, x2);
    double* xx = Ln.x;
    parallel_for(c.stream, Ln.n, PFV_LAMBDA(int64_t i) { xx[i] += x2[i]; });
  }
  nns_prolong(c, L, k, H.alpha, Ln.x, x);
  for (int sweep = 0; sweep < H.sweeps; ++sweep) {
    nns_spmv(c, L, x, t);
    nns_smooth(c, L, H.omega, x, b, t, x);
  }
}

// rigid-body modes of the grid's cells, column-major [k][nc * nd] in the grid's numbering (cell-major,
// component-minor rows): nd translations, then the rotations (2-D: (-y, x); 3-D: about x, y, z)
static void nns_rigid_body_modes(pfv_ctx_impl& c, int nd, int64_t nc, const double* ccen, double* B) {
  const int64_t n = nc * nd;
  parallel_for(c.stream, nc, PFV_LAMBDA(int64_t i) {
    const double x = ccen[i], y = ccen[nc + i], z = ccen[2 * nc + i];
    if (nd == 2) {
      const double m[3][2] = {{1.0, 0.0}, {0.0, 1.0}, {-y, x}};
      for (int j = 0; j < 3; ++j)
        for (int a = 0; a < 2; ++a) B[j * n + i * 2 + a] = m[j][a];
    } else {
      const double m[6][3] = {{1.0, 0.0, 0.0}, {0.0, 1.0, 0.0}, {0.0, 0.0, 1.0},
                              {0.0, -z, y},    {z, 0.0, -x},    {-y, x, 0.0}};
      for (int j = 0; j < 6; ++j)
        for (int a = 0; a < 3; ++a) B[j * n + i * 3 + a] = m[j][a];
    }
  });
}

}  // namespace pfv
