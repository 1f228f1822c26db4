// mpfa_adjoint.inc — the exact permeability gradient of the MPFA flow solve (pfv_flow_adjoint_exact): the derivative of
// the MPFA matrices themselves, where flow_adjoint.inc's grad_perm is the two-point product rule.
//
//   dJ = z^T d(T p + B bc + V g)/dK at fixed (p, bc, g),   z = g_q - cell_faces mu      (z: flow_adjoint_faces)
//
// so only the K-derivative of the flux at fixed pressure is needed, and K enters the interaction region of a node only
// through nK_h = n_h^T K_c.  In the condensed form of mpfa_numeric.inc (unknowns: the continuity-point pressures lambda)
//
//   g_j = D_j^-1 (lambda_(faces of j) - p_j 1),   u_j = g_j - gamma_j              (gamma: the cell's vector source)
//   R_l = sum_{h in l} sgn_h nK_h . u_j(h) - beta_l bc_l = 0   (rows that are not Dirichlet),   lambda_l = bc_l (Dirichlet)
//   q_s = -nK_{h*} . u_{j*}                                                          (the sub-face flux)
//
// one region does, with the row-scaled A of node_setup and ONE pivoted inverse X = (S A)^-1 (node_gj_lds):
//   1. r from the actual p, bc, gamma;  lambda = X (S r);  u_j per sub-cell
//   2. w_l = -sum_s z_f(s) omega_{h*(s)}[k] on the column l = lf(j*, k);  A^T nu = w:  nu = S (X^T w)
//   3. per sub-half-face h = (j, l) of cell c:
//        grad[r][b][c] += ( -z_f(s) [h = h*(s)] - nu_l sgn_h [row l not Dirichlet] ) n_h[r] u_j[b]
//
// One interaction region per wavefront, the system in LDS.  No floating-point atomics: a region writes the nd^2 numbers
// of each of its sub-cells (sub-cell = nd consecutive sub-half-faces, h / nd) into a buffer indexed by sub-cell, and a
// second kernel sums the sub-cells of every cell in the fixed order of the cell -> sub-cell map (one stable sort of h_cell,
// kept with the topology: rebuilt only when the topology digest changes).  The PFV_EMULATE build runs the same bodies,
// one lane per region.
//
// pfv_advdiff_adjoint_exact needs the same derivative for the N states of a time loop, sum_n d/dK (z^n)^T (T c^n + B bc):
// set-up and inverse do not depend on n, so adj_batch_body does them once per region and runs stages 1 - 3 per state.
namespace pfv {

struct AdjNodeArgs {
  NodeArgs a;
  const double *p, *bc, *vs, *z;  // cell pressures, boundary values per face, vector source [cell][vd] or nullptr, z per face
  int vd;
  double* sub;  // [nh / nd][nd * nd] the regions' contributions per sub-cell
};

struct AdjLds {
  double *di, *nrm, *lam, *nu, *rv, *u, *zs;
};

PFV_HD inline size_t adj_extra_doubles(int n, int nh, int nd) {
  return ((size_t)2 * nh * nd + 4 * (size_t)n + (size_t)nh + 1) & ~size_t(1);  // (even: A stays 16-byte aligned)
}

static size_t adj_node_lds_bytes(int nmax, int degmax, int nd) {
  return node_lds_bytes(nmax, degmax, nd) + 8 * adj_extra_doubles(nmax, degmax * nd, nd);
}

// the region's own arrays first, then the block of node_carve
PFV_FN void adj_carve(char* lds, int n, int ld, int nh, int nd, NodeLds& L, AdjLds& X) {
  Carver cv(lds);
  X.di = cv.take<double>((size_t)nh * nd);   // [j][i][k]: D_j^-1
  X.nrm = cv.take<double>((size_t)nh * nd);  // [hh][i]: n_h = n_f / #nodes(f)
  X.lam = cv.take<double>(n);
  X.nu = cv.take<double>(n);
  X.rv = cv.take<double>(n);  // S r, then w
  X.u = cv.take<double>(nh);  // [j][b]
  X.zs = cv.take<double>(n);
  node_carve(lds + 8 * adj_extra_doubles(n, nh, nd), n, ld, nh, nd, L);
}

// The node of work item `first + w.item`, its set-up and (S A)^-1 in L.A: what a region does once, whatever the number
// of states.  false: a node without sub-faces.
template <int ND>
PFV_FN bool adj_region(const NodeArgs& a, const WaveCtx& w, int64_t first, NodeLds& L, AdjLds& X, int& h0, int& nh,
                       int& n, int& ld) {
  int v = a.order[first + w.item];
  h0 = a.hp[v];
  nh = a.hp[v + 1] - h0;
  int f0 = a.fp[v];
  n = a.fp[v + 1] - f0;
#ifndef PFV_EMULATE
  // one node per wavefront: wave-uniform (SGPRs, scalar branches)
  v = __builtin_amdgcn_readfirstlane(v);
  h0 = __builtin_amdgcn_readfirstlane(h0);
  nh = __builtin_amdgcn_readfirstlane(nh);
  f0 = __builtin_amdgcn_readfirstlane(f0);
  n = __builtin_amdgcn_readfirstlane(n);
#endif
  if (n == 0) return false;
  ld = n | 1;
  adj_carve(w.lds, n, ld, nh, ND, L, X);
  node_setup<ND, true>(a, w, L, v, h0, nh, f0, n, ld, 0, X.di, X.nrm);
  node_gj_lds(w, L, n, ld, v, a.st);
  return true;
}

// Stages 1 and 2 for one state (p, bc, vs, z): lambda, u_j and nu of the region in X, from the inverse in L.A
template <int ND>
PFV_FN void adj_state_solve(const NodeArgs& a, const WaveCtx& w, const NodeLds& L, const AdjLds& X, int h0, int nh,
                            int n, int ld, const double* p, const double* bc, const double* vs, int vd,
                            const double* z) {
  constexpr int nd = ND;
  const int deg = nh / nd;
  const double* A = L.A;  // (S A)^-1
  // ---- 1. S r: the boundary value, then one side of every sub-face per pass (no two lanes share a row)
  PFV_LANES(l, n) {
    const int t = L.type[l];
    const int f = L.fid[l];
    X.rv[l] = t == 0 ? 0.0 : L.beta[l] * bc[f];
    X.zs[l] = z[f];
  }
  w.lsync();
  for (int pass = 1; pass >= 0; --pass) {
    PFV_LANES(hh, nh) {
      if ((int)L.fsL[hh] == pass) {
        const int l = L.lfL[hh];
        if (L.type[l] != 1) {
          const int cell = a.h_cell[h0 + hh];
          double c = 0.0;
          for (int k2 = 0; k2 < nd; ++k2) c += L.om[hh * nd + k2];
          double t = (double)L.sgL[hh] * c * p[cell];
          if (vs)
            for (int b = 0; b < nd; ++b) t += L.bg[hh * nd + b] * vs[(int64_t)cell * vd + b];
          X.rv[l] += t;
        }
      }
    }
    w.lsync();
  }
  PFV_LANES(l, n) X.rv[l] *= L.scale[l];
  w.lsync();
  PFV_LANES(r, n) {
    double t = 0.0;
    for (int l = 0; l < n; ++l) t += A[r * ld + l] * X.rv[l];
    X.lam[r] = t;
  }
  w.lsync();
  // ---- u_j = D_j^-1 (lambda - p_j 1) - gamma_j
  PFV_LANES(j, deg) {
    const int cell = a.h_cell[h0 + nd * j];
    const double pj = p[cell];
    double dl[nd];
    for (int k = 0; k < nd; ++k) dl[k] = X.lam[L.lfL[nd * j + k]] - pj;
    for (int i = 0; i < nd; ++i) {
      double t = 0.0;
      for (int k = 0; k < nd; ++k) t += X.di[(nd * j + i) * nd + k] * dl[k];
      if (vs) t -= vs[(int64_t)cell * vd + i];
      X.u[nd * j + i] = t;
    }
  }
  // ---- 2. w gathered per column (every sub-face s contributes through the nd sub-faces of the sub-cell of h*(s))
  PFV_LANES(l, n) {
    double t = 0.0;
    for (int s = 0; s < n; ++s) {
      const int hh = L.firstjk[s];
      const int jb = (hh / nd) * nd;
      for (int k = 0; k < nd; ++k)
        if ((int)L.lfL[jb + k] == l) t -= X.zs[s] * L.om[hh * nd + k];
    }
    X.rv[l] = t;
  }
  w.lsync();
  PFV_LANES(l, n) {
    double t = 0.0;
    for (int r = 0; r < n; ++r) t += A[r * ld + l] * X.rv[r];
    X.nu[l] = L.scale[l] * t;
  }
  w.lsync();
}

// Stage 3 for sub-cell j of the state in X: its nd x nd numbers, summed over the nd sub-half-faces from zero
template <int ND>
PFV_FN void adj_subcell_term(const NodeLds& L, const AdjLds& X, int j, double (&acc)[ND][ND]) {
  constexpr int nd = ND;
  for (int r = 0; r < nd; ++r)
    for (int b = 0; b < nd; ++b) acc[r][b] = 0.0;
  for (int k = 0; k < nd; ++k) {
    const int hh = nd * j + k;
    const int l = L.lfL[hh];
    double coef = L.fsL[hh] ? -X.zs[l] : 0.0;
    if (L.type[l] != 1) coef -= X.nu[l] * (double)L.sgL[hh];
    for (int r = 0; r < nd; ++r)
      for (int b = 0; b < nd; ++b) acc[r][b] += coef * X.nrm[hh * nd + r] * X.u[nd * j + b];
  }
}

template <int ND>
PFV_FN void adj_node_body(const AdjNodeArgs& g, const WaveCtx& w, int64_t first) {
  constexpr int nd = ND;
  NodeLds L;
  AdjLds X;
  int h0, nh, n, ld;
  if (!adj_region<ND>(g.a, w, first, L, X, h0, nh, n, ld)) return;
  adj_state_solve<ND>(g.a, w, L, X, h0, nh, n, ld, g.p, g.bc, g.vs, g.vd, g.z);
  // ---- 3. the nd x nd numbers of every sub-cell
  PFV_LANES(j, nh / nd) {
    double acc[nd][nd];
    adj_subcell_term<ND>(L, X, j, acc);
    double* dst = g.sub + ((int64_t)(h0 / nd) + j) * (nd * nd);
    for (int r = 0; r < nd; ++r)
      for (int b = 0; b < nd; ++b) dst[r * nd + b] = acc[r][b];
  }
}

// ---- the same region for a batch of states (pfv_advdiff_adjoint_exact): set-up and inverse ONCE, then stages 1 - 3 per
// state m = 0 .. nb - 1 with p = p0 + m pstride, z = z0 + m zstride, no vector source; lam / nu / rv / u / zs are reused,
// so the LDS need is that of adj_node_body.  sub holds the running sum over the states of all batches so far (zeros before
// the first batch): a lane loads the nd x nd numbers of its sub-cell j = lane, adds the states' terms in the order of m
// -- each term summed from zero as in adj_node_body -- and stores them once; a region with more sub-cells than lanes
// (and every sub-cell but the first of the one-lane emulation build) adds those in memory, same terms, same order.
// Hence the same bits for every split of the states into batches.
struct AdjBatchArgs {
  NodeArgs a;
  const double *p0, *z0, *bc;
  int64_t pstride, zstride;
  int nb;
  double* sub;
};

template <int ND>
PFV_FN void adj_batch_body(const AdjBatchArgs& g, const WaveCtx& w, int64_t first) {
  constexpr int nd = ND;
  NodeLds L;
  AdjLds X;
  int h0, nh, n, ld;
  if (!adj_region<ND>(g.a, w, first, L, X, h0, nh, n, ld)) return;
  const int deg = nh / nd;
  double* sub = g.sub + (int64_t)(h0 / nd) * (nd * nd);
  const bool own = w.lane < deg;
  double run[nd][nd], term[nd][nd];
  for (int r = 0; r < nd; ++r)
    for (int b = 0; b < nd; ++b) run[r][b] = own ? sub[w.lane * (nd * nd) + r * nd + b] : 0.0;
  for (int m = 0; m < g.nb; ++m) {
    adj_state_solve<ND>(g.a, w, L, X, h0, nh, n, ld, g.p0 + m * g.pstride, g.bc, nullptr, 0, g.z0 + m * g.zstride);
    if (own) {
      adj_subcell_term<ND>(L, X, w.lane, term);
      for (int r = 0; r < nd; ++r)
        for (int b = 0; b < nd; ++b) run[r][b] += term[r][b];
    }
    for (int j = w.lane + w.width; j < deg; j += w.width) {
      adj_subcell_term<ND>(L, X, j, term);
      double* dst = sub + j * (nd * nd);
      for (int r = 0; r < nd; ++r)
        for (int b = 0; b < nd; ++b) dst[r * nd + b] += term[r][b];
    }
    w.lsync();  // (the next state overwrites zs, rv and u)
  }
  if (own)
    for (int r = 0; r < nd; ++r)
      for (int b = 0; b < nd; ++b) sub[w.lane * (nd * nd) + r * nd + b] = run[r][b];
}

// cell -> sub-cell map: the sub-cells (h / nd) sorted by their cell, stable, so that the sub-cells of a cell come in
// ascending order (= ascending node); adj_cptr[c] .. adj_cptr[c + 1] is the cell's segment of adj_csub
static void adj_cell_map(pfv_ctx_impl& c) {
  stream_t s = c.stream;
  const int nd = c.nd;
  const int64_t nsc = c.nh / nd, nc = c.nc;
  if (nsc >= (int64_t(1) << 31)) throw Error(PFV_ERR_UNSUPPORTED, "the exact gradient needs fewer than 2^31 sub-cells");
  const int32_t* hc = c.h_cell;
  Buf<uint32_t> kin_, kout_;
  Buf<int32_t> vin_;
  uint32_t* kin = kin_.ensure((size_t)std::max<int64_t>(nsc, 1));
  uint32_t* kout = kout_.ensure((size_t)std::max<int64_t>(nsc, 1));
  int32_t* vin = vin_.ensure((size_t)std::max<int64_t>(nsc, 1));
  int32_t* csub = c.adj_csub.ensure((size_t)std::max<int64_t>(nsc, 1));
  int32_t* cptr = c.adj_cptr.ensure((size_t)nc + 1);
  parallel_for(s, nsc, PFV_LAMBDA(int64_t q) {
    kin[q] = (uint32_t)hc[q * nd];
    vin[q] = (int32_t)q;
  });
  int bits = 1;
  while ((int64_t(1) << bits) < nc) ++bits;
  sort_pairs(s, c.scratch, kin, kout, vin, csub, (size_t)nsc, bits);
  parallel_for(s, nc + 1, PFV_LAMBDA(int64_t j) {
    cptr[j] = (int32_t)lower_bound_idx<uint32_t>(kout, (int)nsc, (uint32_t)j);
  });
  be_sync(s);  // (the sort's staging buffers are freed on return)
}

// A class whose largest region does not fit the LDS of a workgroup: PFV_ERR_UNSUPPORTED naming a node of it.  Depends on
// the topology alone, so the caller asks before its solve (a refused call costs nothing).
static void adj_check_lds(pfv_ctx_impl& c) {
  if (!c.have_topology) throw Error(PFV_ERR_ARGUMENT, "no sub-cell topology on the handle: pfv_mpfa_discretize first");
  const int nd = c.nd;
  for (int cls = 0; cls < kNumClasses; ++cls) {
    const int64_t b0 = c.class_begin[cls], b1 = c.class_begin[cls + 1];
    if (b1 <= b0) continue;
    const int nmax = std::min(kClassBounds[cls], std::max(c.max_block, 1));
    const int degmax = std::max(1, std::min(c.max_deg, 2 * nmax / nd));
    if (adj_node_lds_bytes(nmax, degmax, nd) > 160 * 1024) {
      const int32_t node = read_scalar<int32_t>(c.stream, c.node_order.p + b0);
      throw Error(PFV_ERR_UNSUPPORTED, "the interaction region of node " + std::to_string(node) + " (up to " +
                                           std::to_string(nmax) + " sub-faces) does not fit the LDS: no exact gradient");
    }
  }
}

// what node_setup<ND, true> reads of the handle; st: the status words [4] of the pass (zeroed by the caller)
static void adj_node_args(pfv_ctx_impl& c, int32_t* st, NodeArgs& a) {
  const int nd = c.nd;
  a.nd = nd; a.nc = c.nc; a.nf = c.nf; a.nn = c.nn; a.eta = c.eta;
  a.order = c.node_order; a.hp = c.node_hptr; a.fp = c.node_fptr; a.node_sf = c.node_sf; a.node_face = c.node_face;
  a.sf_face = c.sf_face; a.fn_ptr = c.fn_ptr; a.nsides = c.face_nsides; a.h_cell = c.h_cell;
  a.bp = c.node_bptr; a.bls = c.node_bls;
  a.h_lf = c.h_lf; a.h_first = c.h_first; a.bcflag = c.bcflag; a.h_sgn = c.h_sgn;
  a.robin = c.robin; a.farea = c.farea; a.fnorm = c.fnorm; a.fcen = c.fcen; a.ccen = c.ccen;
  a.nodes = c.nodes; a.perm = c.perm; a.eta_sub = c.have_eta_sub ? c.eta_sub.p : nullptr;
  a.fshift = nullptr; a.fnative = nullptr;  // (periodic grids are refused by the caller, conditions per sub-face too)
  a.tptr = nullptr; a.tbptr = nullptr; a.tab = nullptr; a.tabb = nullptr; a.rec = nullptr;  // never touched (ADJ)
  a.st = st;
  a.ablate = 0;
  a.active = nullptr;
  a.sub_bc = 0;
  a.refine = -1;
  a.redo = nullptr;
}

// the status words of the region passes as errors
static void adj_throw_status(const int32_t* sth) {
  if (sth[1]) throw Error(PFV_ERR_ARGUMENT, "Boundary values should be either Dirichlet, Neumann or Robin");
  if (sth[0])
    throw Error(PFV_ERR_SINGULAR, "Error in inversion of local linear systems (node " + std::to_string(sth[0] - 1) + ")");
}

// gexact [9][nc] = the sub-cells of every cell summed in the order of the cell -> sub-cell map
static void adj_cell_sum(pfv_ctx_impl& c, const double* sub, double* gexact) {
  const int nd = c.nd;
  const int64_t nc = c.nc;
  const int32_t* cptr = c.adj_cptr;
  const int32_t* csub = c.adj_csub;
  parallel_for(c.stream, nc, PFV_LAMBDA(int64_t cell) {
    double acc[9];
    for (int r = 0; r < 9; ++r) acc[r] = 0.0;
    for (int k = cptr[cell]; k < cptr[cell + 1]; ++k) {
      const double* src = sub + (int64_t)csub[k] * (nd * nd);
      for (int r = 0; r < nd; ++r)
        for (int b = 0; b < nd; ++b) acc[3 * r + b] += src[r * nd + b];
    }
    for (int r = 0; r < 9; ++r) gexact[(int64_t)r * nc + cell] = acc[r];
  });
}

// The two kernels (after adj_check_lds).  gexact: [9][nc] in the layout of perm; entries outside the nd x nd block are zero.
static void flow_adjoint_grad_perm_exact(pfv_ctx_impl& c, const double* d_p, const double* d_bc, const double* d_vs,
                                         int vd, const double* z, double* gexact) {
  stream_t s = c.stream;
  const int nd = c.nd;
  adj_check_lds(c);
  be_memset(c.status.ensure(16), 0, sizeof(int32_t) * 4, s);
  AdjNodeArgs g;
  adj_node_args(c, c.status, g.a);
  g.p = d_p; g.bc = d_bc; g.vs = d_vs; g.z = z; g.vd = vd;
  const int64_t nsc = c.nh / nd;
  g.sub = c.adj_sub.ensure((size_t)std::max<int64_t>(nsc * nd * nd, 1));
  for (int cls = 0; cls < kNumClasses; ++cls) {
    const int64_t b0 = c.class_begin[cls], b1 = c.class_begin[cls + 1];
    if (b1 <= b0) continue;
    const int nmax = std::min(kClassBounds[cls], std::max(c.max_block, 1));
    const int degmax = std::max(1, std::min(c.max_deg, 2 * nmax / nd));
    const size_t lds = adj_node_lds_bytes(nmax, degmax, nd);
    const int64_t cnt = b1 - b0;
    if (nd == 2) wave_for<64>(s, cnt, lds, PFV_LAMBDA(const WaveCtx& w) { adj_node_body<2>(g, w, b0); });
    else wave_for<64>(s, cnt, lds, PFV_LAMBDA(const WaveCtx& w) { adj_node_body<3>(g, w, b0); });
  }
  int32_t sth[4];
  be_d2h(sth, c.status.p, sizeof(sth), s);
  adj_throw_status(sth);
  adj_cell_sum(c, g.sub, gexact);
}

// One pass over the regions for the nb states of a batch (adj_batch_body), class by class; adj_sub holds the running sum.
// Returns the number of launches.  The status words st are the caller's: read once, after the last batch.
static int advdiff_adjoint_exact_batch(pfv_ctx_impl& c, int32_t* st, const double* p0, int64_t pstride, const double* z0,
                                       const double* bc, int nb) {
  stream_t s = c.stream;
  const int nd = c.nd;
  AdjBatchArgs g;
  adj_node_args(c, st, g.a);
  g.p0 = p0; g.pstride = pstride; g.z0 = z0; g.zstride = c.nf; g.bc = bc; g.nb = nb;
  g.sub = c.adj_sub.p;
  int launches = 0;
  for (int cls = 0; cls < kNumClasses; ++cls) {
    const int64_t b0 = c.class_begin[cls], b1 = c.class_begin[cls + 1];
    if (b1 <= b0) continue;
    const int nmax = std::min(kClassBounds[cls], std::max(c.max_block, 1));
    const int degmax = std::max(1, std::min(c.max_deg, 2 * nmax / nd));
    const size_t lds = adj_node_lds_bytes(nmax, degmax, nd);
    const int64_t cnt = b1 - b0;
    if (nd == 2) wave_for<64>(s, cnt, lds, PFV_LAMBDA(const WaveCtx& w) { adj_batch_body<2>(g, w, b0); });
    else wave_for<64>(s, cnt, lds, PFV_LAMBDA(const WaveCtx& w) { adj_batch_body<3>(g, w, b0); });
    ++launches;
  }
  return launches;
}

}  // namespace pfv
