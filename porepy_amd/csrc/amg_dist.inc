// amg_dist.inc — the coupled hierarchy of a sharded solve (pfv_amg_setup_sharded); included by amg.inc.
//
// pfv_amg_setup(n_own) builds a hierarchy of the rank's own diagonal block: block Jacobi across ranks, no
// communication in the preconditioner, and the iteration count grows with the number of ranks (the error across a
// rank boundary is seen by no coarse level).  Here the levels keep the couplings:
//   * level l of a rank: the rows of the unknowns it owns over owned + halo columns, with a halo plan of its own;
//   * aggregates never cross a rank boundary (matching ignores halo columns); the Galerkin product of the owned rows
//     carries the halo columns along, and one exchange of the owners' aggregate numbers per level renames them --
//     the plan of the next level follows from that exchange alone (both ends sort the same set of numbers);
//   * smoothing / residual products see current halo values: one point-to-point exchange before each (2 per level
//     visit; the first smoothing step starts from zero and needs none);
//   * from the first level whose rows, summed over the ranks, number at most PFV_AMG_GATHER_ROWS the rows of all ranks
//     are gathered (allgather of row lengths, global columns, values) and every rank continues with the same
//     replicated hierarchy (amg_setup on the gathered matrix; identical on all ranks, the kernels are deterministic):
//     per cycle one allgather of that level's right-hand side.  Small levels are bound by launch latency, not by
//     work -- replicating them costs nothing, exchanging on them would cost 2 latencies per level.
// Control flow is the same on every rank: the number of distributed levels and the cycle shape are decided from
// gathered sizes only; a rank whose matching stalls keeps its cells as they are (identity aggregation).
// The transport (pfv_shard_hooks::sendrecv / allgather) moves packed buffers; packing, plans and the gathered matrix
// are built here with the portable kernels, so the host emulation runs the same code under gloo in the tests.

static void amg_hook_failed(const char* what) {
  throw Error(PFV_ERR_ARGUMENT, std::string("coupled hierarchy: the ") + what + " hook reported a failure");
}

// halo entries of x (cells [n_own, n_own + n_halo) of the level, bs values each) from their owners
static void amg_halo_exchange(pfv_ctx_impl& c, AmgDist& D, const AmgPlan& pl, double* x, int bs) {
  if (pl.n_peers == 0 || (pl.n_send == 0 && pl.n_recv == 0)) return;
  stream_t s = c.stream;
  double* sb = D.sbuf.ensure((size_t)std::max<int64_t>(pl.n_send * bs, 1));
  double* rb = D.rbuf.ensure((size_t)std::max<int64_t>(pl.n_recv * bs, 1));
  const int32_t* si = pl.send_idx;
  const int32_t* rp = pl.recv_pos;
  parallel_for(s, pl.n_send * bs, PFV_LAMBDA(int64_t q) {
    const int64_t k = q / bs;
    sb[q] = x[(int64_t)si[k] * bs + (q - k * bs)];
  });
  std::vector<int64_t> sp(pl.send_ptr), rv(pl.recv_ptr);
  for (auto& v : sp) v *= bs;
  for (auto& v : rv) v *= bs;
  if (D.hooks.sendrecv(D.hooks.user, pl.n_peers, pl.peers.data(), sb, sp.data(), rb, rv.data(), (void*)(intptr_t)s))
    amg_hook_failed("sendrecv");
  parallel_for(s, pl.n_recv * bs, PFV_LAMBDA(int64_t q) {
    const int64_t k = q / bs;
    x[(int64_t)rp[k] * bs + (q - k * bs)] = rb[q];
  });
  ++D.exchanges;
}

static void amg_allgather(pfv_ctx_impl& c, AmgDist& D, const void* send, void* recv, int64_t bytes_per_rank) {
  if (D.hooks.allgather(D.hooks.user, send, recv, bytes_per_rank, (void*)(intptr_t)c.stream)) amg_hook_failed("allgather");
  ++D.allgathers;
}

// two int64 of every rank -> host
static std::vector<int64_t> amg_gather_counts(pfv_ctx_impl& c, AmgDist& D, int64_t a, int64_t b) {
  stream_t s = c.stream;
  int64_t mine[2] = {a, b};
  int64_t* ds = D.cnt_s.ensure(2);
  int64_t* dr = D.cnt_r.ensure((size_t)2 * D.world);
  be_h2d(ds, mine, sizeof(mine), s);
  amg_allgather(c, D, ds, dr, sizeof(mine));
  std::vector<int64_t> out((size_t)2 * D.world);
  be_d2h(out.data(), dr, sizeof(int64_t) * out.size(), s);
  be_sync(s);
  return out;
}

static void amg_plan_upload(pfv_ctx_impl& c, AmgPlan& pl) {
  stream_t s = c.stream;
  pl.n_send = pl.send_ptr.empty() ? 0 : pl.send_ptr.back();
  pl.n_recv = pl.recv_ptr.empty() ? 0 : pl.recv_ptr.back();
  be_h2d(pl.send_idx.ensure((size_t)std::max<int64_t>(pl.n_send, 1)), pl.h_send_idx.data(), sizeof(int32_t) * (size_t)pl.n_send, s);
  be_h2d(pl.recv_pos.ensure((size_t)std::max<int64_t>(pl.n_recv, 1)), pl.h_recv_pos.data(), sizeof(int32_t) * (size_t)pl.n_recv, s);
}

// Plan of level l + 1 from the plan of level l and the aggregates of the owned cells; chalo[h] = halo cell of the new
// level that halo cell h of level l belongs to (returned on the device in D.chalo).
static std::unique_ptr<AmgPlan> amg_coarse_plan(pfv_ctx_impl& c, AmgDist& D, const AmgPlan& pl, const int32_t* agg,
                                                int64_t nc_cells) {
  stream_t s = c.stream;
  const int64_t n = pl.n_own, nh = pl.n_halo;
  // the owners' aggregate numbers of the halo cells (exact in a double)
  double* g = D.gid.ensure((size_t)std::max<int64_t>(n + nh, 1));
  parallel_for(s, n, PFV_LAMBDA(int64_t i) { g[i] = (double)agg[i]; });
  parallel_for(s, nh, PFV_LAMBDA(int64_t h) { g[n + h] = -1.0; });
  amg_halo_exchange(c, D, pl, g, 1);
  std::vector<double> hg((size_t)nh);
  be_d2h(hg.data(), g + n, sizeof(double) * (size_t)nh, s);
  // ... and the aggregates of the cells this rank sends
  int32_t* tmp = D.itmp.ensure((size_t)std::max<int64_t>(pl.n_send, 1));
  const int32_t* si = pl.send_idx;
  parallel_for(s, pl.n_send, PFV_LAMBDA(int64_t k) { tmp[k] = agg[si[k]]; });
  std::vector<int32_t> sagg((size_t)pl.n_send);
  be_d2h(sagg.data(), tmp, sizeof(int32_t) * (size_t)pl.n_send, s);
  be_sync(s);
  auto np = std::make_unique<AmgPlan>();
  np->n_peers = pl.n_peers;
  np->peers = pl.peers;
  np->n_own = nc_cells;
  np->send_ptr.assign(1, 0);
  np->recv_ptr.assign(1, 0);
  std::vector<int32_t> chalo((size_t)nh, -1);
  for (int p = 0; p < pl.n_peers; ++p) {
    // receive side: the distinct aggregates of peer p among my halo cells, ascending -- the order p sends them in
    std::vector<int32_t> u;
    for (int64_t k = pl.recv_ptr[p]; k < pl.recv_ptr[p + 1]; ++k) {
      const double v = hg[(size_t)(pl.h_recv_pos[k] - n)];
      if (!(v >= 0.0)) throw Error(PFV_ERR_ARGUMENT, "coupled hierarchy: a halo cell received no aggregate number (plans of the ranks disagree)");
      u.push_back((int32_t)v);
    }
    std::sort(u.begin(), u.end());
    u.erase(std::unique(u.begin(), u.end()), u.end());
    const int64_t base = np->recv_ptr.back();
    for (int64_t k = pl.recv_ptr[p]; k < pl.recv_ptr[p + 1]; ++k) {
      const int64_t h = pl.h_recv_pos[k] - n;
      const int32_t id = (int32_t)hg[(size_t)h];
      chalo[(size_t)h] = (int32_t)(base + (std::lower_bound(u.begin(), u.end(), id) - u.begin()));
    }
    for (size_t k = 0; k < u.size(); ++k) {
      np->h_recv_pos.push_back((int32_t)(nc_cells + base + (int64_t)k));
      np->halo_peer.push_back((int32_t)p);
      np->halo_owner_id.push_back(u[k]);
    }
    np->recv_ptr.push_back(base + (int64_t)u.size());
    // send side: the distinct aggregates of the cells I send to p, ascending
    std::vector<int32_t> v(sagg.begin() + pl.send_ptr[p], sagg.begin() + pl.send_ptr[p + 1]);
    std::sort(v.begin(), v.end());
    v.erase(std::unique(v.begin(), v.end()), v.end());
    np->h_send_idx.insert(np->h_send_idx.end(), v.begin(), v.end());
    np->send_ptr.push_back(np->send_ptr.back() + (int64_t)v.size());
  }
  for (int64_t h = 0; h < nh; ++h)
    if (chalo[(size_t)h] < 0) throw Error(PFV_ERR_ARGUMENT, "coupled hierarchy: a halo cell is in no receive list of the plan");
  np->n_halo = np->recv_ptr.back();
  amg_plan_upload(c, *np);
  be_h2d(D.chalo.ensure((size_t)std::max<int64_t>(nh, 1)), chalo.data(), sizeof(int32_t) * (size_t)nh, s);
  return np;
}

// ---- the steps of amg_setup that exist only under the coupled hierarchy (called behind its `if (D)`)

// fetches the halo entries of a level-0 vector from their owners (empty without a coupled hierarchy)
static std::function<void(double*)> amg_fill_halo0(pfv_ctx_impl& c, AmgDist* D, int bs) {
  if (!D) return nullptr;
  return [&c, D, bs](double* v) { amg_halo_exchange(c, *D, *D->plan[0], v, bs); };
}

// The sizes of all ranks and, in the second word, whether EVERY rank may keep its aggregate maps, in one gather: all
// ranks get the same answer and take the same branch of the setup (its exchanges stay matched).
static bool amg_dist_vote(pfv_ctx_impl& c, AmgDist& D, int64_t nrows, bool mine) {
  const std::vector<int64_t> cnt0 = amg_gather_counts(c, D, nrows, mine ? 1 : 0);
  D.global_rows0 = 0;
  bool all = true;
  for (int r = 0; r < D.world; ++r) {
    D.global_rows0 += cnt0[2 * r];
    all = all && cnt0[2 * r + 1] == 1;
  }
  D.global_rows_level = D.global_rows0;
  D.kgather = 0;
  D.exchanges = D.allgathers = 0;
  return all;
}

// halo columns ride along unchanged through the passes of a level (renamed once, after the last pass): the map of a pass
// extended by the identity on the halo cells
static const int32_t* amg_dist_extend_map(pfv_ctx_impl& c, AmgDist& D, size_t l, const int32_t* a1p, int64_t cur_cells,
                                          int64_t nagg) {
  const int64_t nh = D.plan[l]->n_halo;
  int32_t* ae = D.aext.ensure((size_t)(cur_cells + nh));
  parallel_for(c.stream, cur_cells + nh, PFV_LAMBDA(int64_t i) { ae[i] = i < cur_cells ? a1p[i] : (int32_t)(nagg + (i - cur_cells)); });
  return ae;
}

// this rank has nothing left to merge, others may: its cells go on as they are (every rank builds every level); the
// level's matrix lands in slot 0 of the workspace
static void amg_dist_identity_level(pfv_ctx_impl& c, Amg& amg, AmgDist& D, size_t l, const CsrPattern& P, const double* val,
                                    int32_t* aggL, int64_t cells) {
  stream_t s = c.stream;
  AmgWork& wk = amg.wk;
  int32_t* ident = wk.a1.ensure((size_t)cells);
  const int64_t nh = D.plan[l]->n_halo;
  int32_t* ae = D.aext.ensure((size_t)(cells + nh));
  parallel_for(s, cells, PFV_LAMBDA(int64_t i) { ident[i] = (int32_t)i; aggL[i] = (int32_t)i; });
  parallel_for(s, cells + nh, PFV_LAMBDA(int64_t i) { ae[i] = (int32_t)i; });
  amg_members(c, wk, ident, cells, cells, wk.mp, wk.me);
  amg_galerkin(c, amg.sw, wk, P, val, amg.bs, ae, wk.mp, wk.me, cells, wk.P[0], wk.V[0], wk.D[0]);
  wk.P[0].ncols = (cells + nh) * amg.bs;
}

// the plan of level l + 1, and the owners' aggregates rename the halo columns of its matrix
static void amg_dist_rename_halo(pfv_ctx_impl& c, AmgDist& D, size_t l, const int32_t* aggL, int64_t ncn, int bs, AmgLevel& Ln) {
  while (D.plan.size() <= l + 1) D.plan.push_back(nullptr);
  D.plan[l + 1] = amg_coarse_plan(c, D, *D.plan[l], aggL, ncn);
  const int32_t* ch = D.chalo;
  int32_t* ixn = Ln.P_own.indices;
  parallel_for(c.stream, Ln.P_own.nnz, PFV_LAMBDA(int64_t e) {
    const int col = ixn[e];
    const int cc = col / bs;
    if (cc >= ncn) ixn[e] = (int32_t)((ncn + ch[cc - ncn]) * bs + (col - cc * bs));
  });
  Ln.P_own.ncols = (ncn + D.plan[l + 1]->n_halo) * bs;
  Ln.m = Ln.P_own.ncols;
}

// gather from level l + 1 on?  (decided from the rows of all ranks: the same on every rank)
static void amg_dist_decide_gather(pfv_ctx_impl& c, AmgDist& D, size_t l, int64_t rows_next, int64_t gather_rows) {
  const std::vector<int64_t> cn = amg_gather_counts(c, D, rows_next, 0);
  int64_t tot = 0;
  for (int r = 0; r < D.world; ++r) tot += cn[2 * r];
  const int64_t tot_here = D.global_rows_level;
  D.global_rows_level = tot;
  if (tot <= gather_rows || tot > 0.85 * tot_here || (int)l + 3 >= kAmgMaxLevels) D.kgather = l + 1;
}

// Rows of all ranks at the gathered level -> one matrix in global numbering (rank-major), sorted and merged; then the
// replicated hierarchy on it.
static void amg_build_global(pfv_ctx_impl& c, Amg& amg, AmgDist& D, AmgLevel& LK, const AmgPlan& plK) {
  stream_t s = c.stream;
  const int bs = amg.bs;
  const int W = D.world;
  const int64_t nK = LK.n, nnzK = LK.P->nnz;
  const std::vector<int64_t> cnt = amg_gather_counts(c, D, nK, nnzK);
  D.gn.assign((size_t)W, 0);
  D.goff.assign((size_t)W + 1, 0);
  std::vector<int64_t> gnnz((size_t)W), nnzoff((size_t)W + 1, 0);
  int64_t nmax = 1, nnzmax = 1;
  for (int r = 0; r < W; ++r) {
    D.gn[r] = cnt[2 * r];
    gnnz[r] = cnt[2 * r + 1];
    D.goff[r + 1] = D.goff[r] + D.gn[r];
    nnzoff[r + 1] = nnzoff[r] + gnnz[r];
    nmax = std::max(nmax, D.gn[r]);
    nnzmax = std::max(nnzmax, gnnz[r]);
  }
  const int64_t N = D.goff[W], NNZ = nnzoff[W];
  if (NNZ >= (int64_t(1) << 31) || N >= (int64_t(1) << 31))
    throw Error(PFV_ERR_UNSUPPORTED, "coupled hierarchy: the gathered level does not fit 32-bit indices (lower PFV_AMG_GATHER_ROWS)");
  D.gN = N;
  D.gnmax = nmax;
  be_h2d(D.gn_d.ensure((size_t)W), D.gn.data(), sizeof(int64_t) * (size_t)W, s);
  be_h2d(D.goff_d.ensure((size_t)W + 1), D.goff.data(), sizeof(int64_t) * (size_t)(W + 1), s);
  // global cell of every halo cell of this level
  std::vector<int32_t> hg((size_t)std::max<int64_t>(plK.n_halo, 1), 0);
  for (int64_t h = 0; h < plK.n_halo; ++h)
    hg[(size_t)h] = (int32_t)(D.goff[plK.peers[plK.halo_peer[(size_t)h]]] / bs + plK.halo_owner_id[(size_t)h]);
  int32_t* hgd = D.hal_gcell.ensure(hg.size());
  be_h2d(hgd, hg.data(), sizeof(int32_t) * hg.size(), s);
  // my rows: lengths, global columns, values (padded to the largest rank)
  int32_t* ls = D.glen_s.ensure((size_t)nmax);
  int32_t* cs = D.gcol_s.ensure((size_t)nnzmax);
  double* vs = D.gval_s.ensure((size_t)nnzmax);
  const int32_t* ip = LK.P->indptr;
  const int32_t* ix = LK.P->indices;
  const double* val = LK.val;
  const int64_t ncell = nK / bs, mycell0 = D.goff[D.rank] / bs;
  be_memset(ls, 0, sizeof(int32_t) * (size_t)nmax, s);
  parallel_for(s, nK, PFV_LAMBDA(int64_t r) { ls[r] = ip[r + 1] - ip[r]; });
  parallel_for(s, nnzK, PFV_LAMBDA(int64_t e) {
    const int col = ix[e];
    const int cc = col / bs;
    const int64_t gc = cc < ncell ? mycell0 + cc : (int64_t)hgd[cc - ncell];
    cs[e] = (int32_t)(gc * bs + (col - cc * bs));
    vs[e] = val[e];
  });
  int32_t* lr = D.glen_r.ensure((size_t)nmax * W);
  int32_t* cr = D.gcol_r.ensure((size_t)nnzmax * W);
  double* vr = D.gval_r.ensure((size_t)nnzmax * W);
  amg_allgather(c, D, ls, lr, (int64_t)sizeof(int32_t) * nmax);
  amg_allgather(c, D, cs, cr, (int64_t)sizeof(int32_t) * nnzmax);
  amg_allgather(c, D, vs, vr, (int64_t)sizeof(double) * nnzmax);
  // concatenate
  CsrPattern& T = D.gT;
  T.nrows = T.ncols = N;
  T.nnz = NNZ;
  T.max_row = LK.P->max_row;
  int32_t* tp = T.indptr.ensure((size_t)N + 1);
  int32_t* tx = T.indices.ensure((size_t)std::max<int64_t>(NNZ, 1));
  double* tv = D.gTV.ensure((size_t)std::max<int64_t>(NNZ, 1));
  int32_t* glen = D.itmp.ensure((size_t)N + 1);
  int64_t* gpos = amg.wk.pos.ensure((size_t)N + 1);
  for (int r = 0; r < W; ++r) {
    be_d2d(glen + D.goff[r], lr + (size_t)r * nmax, sizeof(int32_t) * (size_t)D.gn[r], s);
    be_d2d(tx + nnzoff[r], cr + (size_t)r * nnzmax, sizeof(int32_t) * (size_t)gnnz[r], s);
    be_d2d(tv + nnzoff[r], vr + (size_t)r * nnzmax, sizeof(double) * (size_t)gnnz[r], s);
  }
  exclusive_scan<int32_t, int64_t>(s, c.scratch, glen, gpos, (size_t)N);
  parallel_for(s, N + 1, PFV_LAMBDA(int64_t r) { tp[r] = (int32_t)gpos[r]; });
  // sort the rows and merge the entries that met in one halo aggregate: the Galerkin kernel with the identity map
  const int64_t Ncell = N / bs;
  int32_t* ident = D.gagg.ensure((size_t)std::max<int64_t>(Ncell, 1));
  parallel_for(s, Ncell, PFV_LAMBDA(int64_t i) { ident[i] = (int32_t)i; });
  amg_members(c, amg.wk, ident, Ncell, Ncell, D.gmp, D.gme);
  amg_galerkin(c, amg.sw, amg.wk, T, tv, bs, ident, D.gmp, D.gme, Ncell, D.gP, D.gV, D.gD);
  if (!D.glob) D.glob = std::make_unique<Amg>();
  D.glob->no_filter = true;
  D.glob->finest_cells_parent = std::max<int64_t>(1, D.global_rows0 / bs);
  amg_setup(c, *D.glob, D.gP, D.gV.p, bs);
  D.gb.ensure((size_t)N);
  D.gx.ensure((size_t)N);
  D.gsend.ensure((size_t)nmax);
  D.grecv.ensure((size_t)nmax * W);
}

// ---- the cycle
static double* amg_cycle_dist(pfv_ctx_impl& c, Amg& amg, size_t l, const double* b, double* x, bool x_is_presmoothed) {
  stream_t s = c.stream;
  AmgDist& D = *amg.dist;
  AmgLevel& L = *amg.lev[l];
  const int64_t n = L.n;
  const int bs = amg.bs;
  if (l == D.kgather) {
    // every rank solves the gathered level with the same replicated hierarchy
    const int64_t nmax = D.gnmax, N = D.gN;
    const int W = D.world;
    double* gs = D.gsend;
    double* gr = D.grecv;
    double* gb = D.gb;
    be_d2d(gs, b, sizeof(double) * (size_t)n, s);
    amg_allgather(c, D, gs, gr, (int64_t)sizeof(double) * nmax);
    const int64_t* gn = D.gn_d;
    const int64_t* goff = D.goff_d;
    parallel_for(s, nmax * W, PFV_LAMBDA(int64_t q) {
      const int64_t r = q / nmax, i = q - r * nmax;
      if (i < gn[r]) gb[goff[r] + i] = gr[q];
    });
    (void)N;
    const double* xg = amg_cycle(c, *D.glob, 0, gb, D.gx);
    const int64_t off = D.goff[D.rank];
    parallel_for(s, n, PFV_LAMBDA(int64_t i) { x[i] = xg[off + i]; });
    return x;
  }
  const AmgPlan& pl = *D.plan[l];
  AmgLevel& Ln = *amg.lev[l + 1];
  const double omega = L.omega, alpha = amg.alpha;
  const double* dinv = L.dinv;
  double* t = L.t;
  if (!x_is_presmoothed) parallel_for(s, n, PFV_LAMBDA(int64_t i) { x[i] = omega * dinv[i] * b[i]; });
  amg_halo_exchange(c, D, pl, x, bs);
  amg_spmv(c, amg, L, x, t, nullptr);
  const bool next_smooths = l + 1 < D.kgather;  // (the gathered level starts its own cycle)
  amg_restrict(c, amg, L, Ln, b, t, next_smooths);
  double* xc = amg_cycle_dist(c, amg, l + 1, Ln.b, Ln.x, next_smooths);
  if (amg.gamma == 2 && (int)l < amg.gamma_levels && l + 1 < D.kgather) {
    // second visit of the first coarse level, on its residual
    double* r2 = Ln.r2.ensure((size_t)Ln.n);
    double* x2 = Ln.x2.ensure((size_t)Ln.m);
    const double* bcn = Ln.b;
    double* tn = Ln.t;
    amg_halo_exchange(c, D, *D.plan[l + 1], xc, bs);
    amg_spmv(c, amg, Ln, xc, tn, nullptr);
    parallel_for(s, Ln.n, PFV_LAMBDA(int64_t i) { r2[i] = bcn[i] - tn[i]; });
    const double* x2r = amg_cycle_dist(c, amg, l + 1, r2, x2, false);
    parallel_for(s, Ln.n, PFV_LAMBDA(int64_t i) { xc[i] += x2r[i]; });
  }
  {
    const int32_t* agg = L.agg;
    parallel_for(s, n, PFV_LAMBDA(int64_t r) {
      const int64_t i = r / bs;
      t[r] = x[r] + alpha * xc[(int64_t)agg[i] * bs + (r - i * bs)];
    });
  }
  amg_halo_exchange(c, D, pl, t, bs);
  amg_spmv(c, amg, L, t, x, b);
  return x;
}

// one application of the coupled hierarchy: out (n_own) ~ A^-1 in (n_own); a collective of the transport
static void amg_apply_dist(pfv_ctx_impl& c, Amg& amg, const double* in, double* out) {
  AmgLevel& L0 = *amg.lev[0];
  double* x0 = L0.x.ensure((size_t)L0.m);
  const double* res = amg_cycle_dist(c, amg, 0, in, x0, false);
  be_d2d(out, res, sizeof(double) * (size_t)L0.n, c.stream);
}
