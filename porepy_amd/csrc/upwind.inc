// upwind.inc — first-order upwind advection (numerics/fv/upwind.py:67-335 of the reference) and the
// transport step built on it, kept on the handle next to the flow discretization that feeds it.
//
//   face flux    q = flux p + bound_flux bc (+ vector_source g): one thread per face row, the three rows
//                summed one after the other in stored order
//   discretize   per face: pos = (q >= 0) as numpy evaluates it on sign(q) (+0, -0 positive; NaN negative);
//                upstream cell = the cell with cell_faces sign +1 (pos) or -1 (neg), -1 outside the domain.
//                Rows of Neumann faces and of Dirichlet faces with the upstream side outside are empty
//                (classify -> exclusive scan -> fill); values are 0 / +-1, patterns as the reference stores them
//   assemble     A = div diag(q) U and b_ref = div (rhs_neu + rhs_dir diag(q)) bc fused, one thread per cell
//                row over its faces in cell_faces order; A on the pattern {cell, face neighbours}
//   advance      r = acc o c - b_ref + source, one kernel per step; the solve is the handle's Krylov solver
//
// No floating-point atomics; every sum has a fixed order.
namespace pfv {

enum { UPW_KEPT = 1, UPW_NEU = 2, UPW_DIRIN = 4 };

// face -> (cell with sign +1, cell with sign -1), -1 = none; sgn_div = sum of the signs of the face's cells
// (a property of the grid: kept until the next pfv_set_grid)
static void upwind_face_cells(pfv_ctx_impl& c) {
  if (c.have_upw_cells) return;
  stream_t s = c.stream;
  const int64_t nc = c.nc, nf = c.nf;
  const int32_t* cf_ptr = c.cf_ptr;
  const int32_t* cf_idx = c.cf_idx;
  const int8_t* cf_sgn = c.cf_sgn;
  int32_t* side = c.upw_side.ensure(2 * nf);
  int32_t* cnt = c.upw_cnt.ensure(2 * nf);
  be_memset(side, 0xff, sizeof(int32_t) * 2 * (size_t)nf, s);
  be_memset(cnt, 0, sizeof(int32_t) * 2 * (size_t)nf, s);
  parallel_for(s, nc, PFV_LAMBDA(int64_t cell) {
    for (int e = cf_ptr[cell]; e < cf_ptr[cell + 1]; ++e) {
      const int64_t slot = (cf_sgn[e] > 0 ? 0 : nf) + cf_idx[e];
      side[slot] = (int32_t)cell;  // (a second cell on the same side is reported below)
      atomic_add_i32(cnt + slot, 1);
    }
  });
  int32_t* st = c.status.ensure(16);
  be_memset(st, 0, sizeof(int32_t) * 8, s);
  parallel_for(s, nf, PFV_LAMBDA(int64_t f) {
    if (cnt[f] > 1 || cnt[nf + f] > 1 || cnt[f] + cnt[nf + f] < 1) atomic_max_i32(st + 1, 1);
  });
  if (read_scalar<int32_t>(s, st + 1))
    throw Error(PFV_ERR_CELL_SHAPE, "a face must have one or two neighbouring cells, of opposite cell_faces sign");
  c.have_upw_cells = true;
}

// A's pattern: every cell and the cells across its faces, ascending (what tpfa.inc builds for div @ flux)
static void upwind_system_pattern(pfv_ctx_impl& c) {
  stream_t s = c.stream;
  const int64_t nc = c.nc, nf = c.nf;
  const int32_t* cf_ptr = c.cf_ptr;
  const int32_t* cf_idx = c.cf_idx;
  const int32_t* side = c.upw_side;
  int32_t* st = c.status.ensure(16);
  be_memset(st, 0, sizeof(int32_t) * 8, s);
  Buf<int32_t> len;
  Buf<int64_t> ptr64;
  int32_t* ln = len.ensure(nc + 1);
  ptr64.ensure(nc + 1);
  CsrPattern& PT = c.pat_T;
  c.have_tpos_T = false;  // (the transposed positions belong to the pattern that is replaced here)
  // Rows come out ascending by selection -- the smallest column above the last one written, over the cell and the
  // <= 2 cells of each of its faces -- so that no per-thread list (scratch memory) is needed: a cell has few faces.
  for (int pass = 0; pass < 2; ++pass) {
    const int32_t* ap = pass ? PT.indptr.p : nullptr;
    int32_t* ax = pass ? PT.indices.p : nullptr;
    parallel_for(s, nc, PFV_LAMBDA(int64_t cell) {
      const int e0 = cf_ptr[cell], e1 = cf_ptr[cell + 1];
      int m = 0;
      int32_t last = -1;
      for (;;) {
        int32_t best = 0x7fffffff;
        if ((int32_t)cell > last) best = (int32_t)cell;
        for (int e = e0; e < e1; ++e) {
          const int f = cf_idx[e];
          const int32_t v0 = side[f], v1 = side[nf + f];
          if (v0 > last && v0 < best) best = v0;
          if (v1 > last && v1 < best) best = v1;
        }
        if (best == 0x7fffffff) break;
        if (ax) ax[ap[cell] + m] = best;
        last = best;
        ++m;
      }
      if (!ax) {
        ln[cell] = m;
        track_max_i32(st + 7, m);
      }
    });
    if (pass == 0) {
      exclusive_scan<int32_t, int64_t>(s, c.scratch, len.p, ptr64.p, (size_t)nc);
      const int64_t nnz = read_scalar<int64_t>(s, ptr64.p + nc);
      if (nnz >= (int64_t(1) << 31)) throw Error(PFV_ERR_UNSUPPORTED, "transport system beyond 2^31 entries");
      PT.nrows = PT.ncols = nc;
      PT.nnz = nnz;
      int32_t* ip = PT.indptr.ensure(nc + 1);
      PT.indices.ensure(std::max<int64_t>(nnz, 1));
      const int64_t* p64 = ptr64;
      parallel_for(s, nc + 1, PFV_LAMBDA(int64_t i) { ip[i] = (int32_t)p64[i]; });
    }
  }
  int32_t sth[8];
  be_d2h(sth, st, sizeof(sth), s);
  PT.max_row = sth[7];
}

// ---- (a) q = flux p + bound_flux bc (+ vector_source g) into c.q_res
static void upwind_face_flux(pfv_ctx_impl& c, const double* d_p, const double* d_bc, const double* d_vs) {
  stream_t s = c.stream;
  const int64_t nf = c.nf;
  const int32_t* fp = c.pat_flux.indptr;
  const int32_t* fx = c.pat_flux.indices;
  const int32_t* bp = c.pat_bound.indptr;
  const int32_t* bx = c.pat_bound.indices;
  const double* vf = c.val[PFV_MAT_FLUX];
  const double* vb = c.val[PFV_MAT_BOUND_FLUX];
  const double* vv = d_vs ? c.val[PFV_MAT_VECTOR_SOURCE].p : nullptr;
  const bool implicit_vs = d_vs && c.vs_implicit && !c.tpfa_mode;
  if (d_vs && !implicit_vs) ensure_vs_indices(c);
  const int32_t* vp = (d_vs && !implicit_vs) ? c.pat_vs.indptr.p : nullptr;
  const int32_t* vx = (d_vs && !implicit_vs) ? c.pat_vs.indices.p : nullptr;
  const int nd = c.nd;
  double* q = c.q_res.ensure(nf);
  parallel_for(s, nf, PFV_LAMBDA(int64_t f) {
    double acc = 0.0;
    const int p0 = fp[f], p1 = fp[f + 1];
    for (int p = p0; p < p1; ++p) acc += vf[p] * d_p[fx[p]];
    for (int p = bp[f]; p < bp[f + 1]; ++p) acc += vb[p] * d_bc[bx[p]];
    if (vv) {
      if (vp) {
        for (int p = vp[f]; p < vp[f + 1]; ++p) acc += vv[p] * d_vs[vx[p]];
      } else {  // values addressed through the flux pattern: entry p, component k -> nd p + k
        for (int p = p0; p < p1; ++p)
          for (int k = 0; k < nd; ++k) acc += vv[(int64_t)p * nd + k] * d_vs[(int64_t)fx[p] * nd + k];
      }
    }
    q[f] = acc;
  });
}

// ---- (b) the three matrices of Upwind.discretize for the flux d_q (Nf values, kept as c.upw_q)
static void upwind_discretize(pfv_ctx_impl& c, const double* d_q, int ncomp) {
  stream_t s = c.stream;
  const int64_t nc = c.nc, nf = c.nf;
  const int64_t k = ncomp;
  if (nf * k >= (int64_t(1) << 31) || nc * k >= (int64_t(1) << 31))
    throw Error(PFV_ERR_UNSUPPORTED, "num_components x faces beyond int32 row indices");
  upwind_face_cells(c);
  double* q = c.upw_q.ensure(nf);
  if (q != d_q) be_d2d(q, d_q, sizeof(double) * (size_t)nf, s);
  const int32_t* side = c.upw_side;
  const int32_t* cnt = c.upw_cnt;
  const uint8_t* flag = c.have_upw_bc ? c.upw_bc.p : nullptr;
  uint8_t* cls = c.upw_cls.ensure(nf);
  int32_t* up = c.upw_up.ensure(nf);
  Buf<int32_t> n_[3];
  Buf<int64_t> pos_[3];
  int32_t* n0 = n_[0].ensure(nf + 1);
  int32_t* n1 = n_[1].ensure(nf + 1);
  int32_t* n2 = n_[2].ensure(nf + 1);
  for (auto& b : pos_) b.ensure(nf + 1);
  int32_t* st = c.status.ensure(16);
  be_memset(st, 0x7f, sizeof(int32_t), s);  // st[0]: first face without an upstream cell
  parallel_for(s, nf, PFV_LAMBDA(int64_t f) {
    const bool boundary = cnt[f] + cnt[nf + f] == 1;
    const unsigned fl = flag ? flag[f] : (boundary ? (unsigned)PFV_BC_DIR : 0u);
    const bool pos = q[f] >= 0.0;  // false for NaN: the negative branch, as numpy's comparison
    const int32_t u = pos ? side[f] : side[nf + f];
    const bool neu = (fl & PFV_BC_NEU) != 0;
    const bool dirin = (fl & PFV_BC_DIR) != 0 && u < 0;
    const bool kept = !neu && !dirin;
    if (kept && u < 0) atomic_min_i32(st, (int32_t)f);
    cls[f] = (uint8_t)((kept ? UPW_KEPT : 0) | (neu ? UPW_NEU : 0) | (dirin ? UPW_DIRIN : 0));
    up[f] = u;
    n0[f] = kept ? 1 : 0;
    n1[f] = dirin ? 1 : 0;
    n2[f] = neu ? 1 : 0;
  });
  const int32_t bad = read_scalar<int32_t>(s, st);
  if (bad != 0x7f7f7f7f)
    throw Error(PFV_ERR_ARGUMENT, "negative axis 1 index: -1 (face " + std::to_string(bad) +
                                      " lies on the boundary, is neither Dirichlet nor Neumann and has inflow: "
                                      "no upstream cell)");
  CsrPattern* P[3] = {&c.pat_upw, &c.pat_upw_dir, &c.pat_upw_neu};
  const int which[3] = {PFV_MAT_UPWIND, PFV_MAT_UPWIND_RHS_DIR, PFV_MAT_UPWIND_RHS_NEU};
  const int32_t* nn[3] = {n0, n1, n2};
  for (int m = 0; m < 3; ++m) {
    exclusive_scan<int32_t, int64_t>(s, c.scratch, nn[m], pos_[m].p, (size_t)nf);
    const int64_t tot = read_scalar<int64_t>(s, pos_[m].p + nf);
    CsrPattern& Q = *P[m];
    // kron(., eye(k)) as the reference stores it: a full k x k block per entry, zeros off its diagonal included
    Q.nrows = nf * k;
    Q.ncols = (m == 0 ? nc : nf) * k;
    Q.nnz = tot * k * k;
    Q.max_row = (int)k;
    if (Q.nnz >= (int64_t(1) << 31)) throw Error(PFV_ERR_UNSUPPORTED, "upwind matrix beyond 2^31 entries");
    int32_t* ip = Q.indptr.ensure(nf * k + 1);
    int32_t* ix = Q.indices.ensure(std::max<int64_t>(Q.nnz, 1));
    double* v = c.val[which[m]].ensure(std::max<int64_t>(Q.nnz, 1));
    const int64_t* pos = pos_[m];
    const int32_t* has = nn[m];
    parallel_for(s, nf + 1, PFV_LAMBDA(int64_t f) {
      const int64_t base = pos[f] * k * k;
      if (f == nf) {
        ip[nf * k] = (int32_t)base;
        return;
      }
      const int h = has[f];
      // row k f + a holds the block row a of the entry of face f: columns k col + b, value val * delta_ab
      const int64_t col = m == 0 ? (int64_t)up[f] : f;
      const double val = m == 2 ? (double)(cnt[f] - cnt[nf + f]) : 1.0;  // rhs_neu: the sign of the face's one cell
      for (int64_t a = 0; a < k; ++a) {
        ip[f * k + a] = (int32_t)(base + a * k * h);
        if (!h) continue;
        for (int64_t b = 0; b < k; ++b) {
          ix[base + a * k + b] = (int32_t)(col * k + b);
          v[base + a * k + b] = val * (a == b ? 1.0 : 0.0);  // (the product keeps the sign of the zeros: -1 * 0 = -0)
        }
      }
    });
    c.filled[which[m]] = true;
  }
  be_sync(s);  // (the scan buffers are freed on return)
}

// ---- (c) A = div diag(q) U (+ diag(acc)), b_ref = div (rhs_neu + rhs_dir diag(q)) bc, r = acc o c_old - b_ref + source
static void upwind_assemble(pfv_ctx_impl& c, const double* d_q, const double* d_bc, const double* d_acc,
                            const double* d_cold, const double* d_src) {
  stream_t s = c.stream;
  const int64_t nc = c.nc, nf = c.nf;
  if (c.pat_T.nrows != nc || !c.have_pat_T) {
    upwind_system_pattern(c);
    c.have_pat_T = true;
  }
  const int32_t* cf_ptr = c.cf_ptr;
  const int32_t* cf_idx = c.cf_idx;
  const int8_t* cf_sgn = c.cf_sgn;
  const int32_t* ap = c.pat_T.indptr;
  const int32_t* ax = c.pat_T.indices;
  const uint8_t* cls = c.upw_cls;
  const int32_t* up = c.upw_up;
  const int32_t* cnt = c.upw_cnt;
  double* Aval = c.val[PFV_MAT_TRANSPORT_SYSTEM].ensure(std::max<int64_t>(c.pat_T.nnz, 1));
  double* diag = c.diag_t.ensure(nc);
  double* rhs = c.rhs_t.ensure(nc);
  double* bref = c.bref_t.ensure(nc);
  int32_t* st = c.status.ensure(16);
  be_memset(st, 0x7f, sizeof(int32_t), s);  // st[0]: first row with a zero diagonal
  parallel_for(s, nc, PFV_LAMBDA(int64_t cell) {
    const int a0 = ap[cell], alen = ap[cell + 1] - a0;
    for (int i = 0; i < alen; ++i) Aval[a0 + i] = 0.0;
    double b = 0.0;
    for (int e = cf_ptr[cell]; e < cf_ptr[cell + 1]; ++e) {
      const int f = cf_idx[e];
      const double sg = (double)cf_sgn[e];
      const unsigned cl = cls[f];
      if (cl & UPW_KEPT) {
        const int32_t col = up[f];
        const int pos = lower_bound_idx<int32_t>(ax + a0, alen, col);
        Aval[a0 + pos] += sg * d_q[f];
      }
      if (cl & (UPW_NEU | UPW_DIRIN)) {
        double m = 0.0;  // the entry of rhs_neu + rhs_dir diag(q) in row f
        if (cl & UPW_NEU) m = (double)(cnt[f] - cnt[nf + f]);
        if (cl & UPW_DIRIN) m += 1.0 * d_q[f];
        b += sg * (m * d_bc[f]);
      }
    }
    const int dpos = lower_bound_idx<int32_t>(ax + a0, alen, (int32_t)cell);
    if (d_acc) Aval[a0 + dpos] += d_acc[cell];
    const double d = Aval[a0 + dpos];
    diag[cell] = d;
    if (!(d != 0.0) || !(d == d)) atomic_min_i32(st, (int32_t)cell);
    bref[cell] = b;
    double r = (d_acc && d_cold) ? d_acc[cell] * d_cold[cell] : 0.0;
    r -= b;
    if (d_src) r += d_src[cell];
    rhs[cell] = r;
  });
  const int32_t zd = read_scalar<int32_t>(s, st);
  c.transport_zero_diag = zd == 0x7f7f7f7f ? -1 : (int64_t)zd;
  c.filled[PFV_MAT_TRANSPORT_SYSTEM] = true;
}

// ---- (d) right-hand side of one implicit Euler step
static void upwind_step_rhs(pfv_ctx_impl& c, const double* d_c) {
  const double* acc = c.have_acc_t ? c.acc_t.p : nullptr;
  const double* src = c.have_src_t ? c.src_t.p : nullptr;
  const double* bref = c.bref_t;
  double* rhs = c.rhs_t;
  parallel_for(c.stream, c.nc, PFV_LAMBDA(int64_t cell) {
    double r = acc ? acc[cell] * d_c[cell] : 0.0;
    r -= bref[cell];
    if (src) r += src[cell];
    rhs[cell] = r;
  });
}

// ---- (e) k components on one flux (pfv_transport_advance_multi).  Every multi-component vector on the device is
// cell-major and interleaved, v[i * k + a]: the k values a row needs from an upstream cell are one contiguous run.
// The caller's arrays are component-major [k][n]; they are transposed here, on the device, on the way in and out.
static void multi_interleave(pfv_ctx_impl& c, int64_t n, int k, const double* by_comp, double* by_cell) {
  parallel_for(c.stream, n * k, PFV_LAMBDA(int64_t t) { by_cell[t] = by_comp[(t % k) * n + t / k]; });
}

static void multi_deinterleave(pfv_ctx_impl& c, int64_t n, int k, const double* by_cell, double* by_comp) {
  parallel_for(c.stream, n * k, PFV_LAMBDA(int64_t t) { by_comp[t] = by_cell[(t % n) * k + t / n]; });
}

// column a of an interleaved vector <-> a plain vector of n values
static void multi_get_column(pfv_ctx_impl& c, int64_t n, int k, int a, const double* by_cell, double* col) {
  parallel_for(c.stream, n, PFV_LAMBDA(int64_t i) { col[i] = by_cell[i * k + a]; });
}

static void multi_set_column(pfv_ctx_impl& c, int64_t n, int k, int a, const double* col, double* by_cell) {
  parallel_for(c.stream, n, PFV_LAMBDA(int64_t i) { by_cell[i * k + a] = col[i]; });
}

// b_ref of every component from its boundary values bc[a][f], by the rule and in the order of upwind_assemble
static void upwind_bref_multi(pfv_ctx_impl& c, int k, const double* d_q, const double* bc, double* bref) {
  const int64_t nc = c.nc, nf = c.nf;
  const int32_t* cf_ptr = c.cf_ptr;
  const int32_t* cf_idx = c.cf_idx;
  const int8_t* cf_sgn = c.cf_sgn;
  const uint8_t* cls = c.upw_cls;
  const int32_t* cnt = c.upw_cnt;
  parallel_for(c.stream, nc * k, PFV_LAMBDA(int64_t t) {
    const int64_t cell = t / k, a = t % k;
    double b = 0.0;
    for (int e = cf_ptr[cell]; e < cf_ptr[cell + 1]; ++e) {
      const int f = cf_idx[e];
      const unsigned cl = cls[f];
      if (cl & (UPW_NEU | UPW_DIRIN)) {
        double m = 0.0;
        if (cl & UPW_NEU) m = (double)(cnt[f] - cnt[nf + f]);
        if (cl & UPW_DIRIN) m += 1.0 * d_q[f];
        b += (double)cf_sgn[e] * (m * bc[a * nf + f]);
      }
    }
    bref[t] = b;
  });
}

// first (row, component), as row * k + component, whose diagonal A[i,i] + acc[i,a] is zero or NaN; -1: none
static int64_t upwind_zero_diag_multi(pfv_ctx_impl& c, int k, const double* diag, const double* acc) {
  stream_t s = c.stream;
  int32_t* st = c.status.ensure(16);
  be_memset(st, 0x7f, sizeof(int32_t), s);
  parallel_for(s, c.nc * k, PFV_LAMBDA(int64_t t) {
    const double d = diag[t / k] + acc[t];
    if (!(d != 0.0) || !(d == d)) atomic_min_i32(st, (int32_t)t);
  });
  const int32_t zd = read_scalar<int32_t>(s, st);
  return zd == 0x7f7f7f7f ? -1 : (int64_t)zd;
}

// right-hand side of one implicit Euler step of all components: the expression of upwind_step_rhs
static void upwind_step_rhs_multi(pfv_ctx_impl& c, int k, const double* acc, const double* src, const double* bref,
                                  const double* x, double* rhs) {
  parallel_for(c.stream, c.nc * k, PFV_LAMBDA(int64_t t) {
    double r = acc[t] * x[t];
    r -= bref[t];
    if (src) r += src[t];
    rhs[t] = r;
  });
}

}  // namespace pfv
