// advdiff.inc — advection-diffusion on one handle: the diffusion discretization of the transport keyword (MPFA or
// TPFA, A_D = div flux_D on pat_A) fused with the upwind term of its faces (upwind.inc) into one system
//
//   S = diag(acc) + div flux_D + w div diag(q) U        on pat_A
//   r = acc o c_old - b_ref + b_D + source,             b_D = -div bound_flux_D bc,
//                                                       b_ref = div (rhs_neu + rhs_dir diag(w q)) bc
//
//   b_D, check   once per discretization: bound_flux_D bc (kept per face for the total flux) and its divergence;
//                every face neighbour of a cell is looked up in the cell's row of pat_A (the upwind pattern must be
//                contained in it: asserted, not assumed)
//   refresh      ONE wave-cooperative kernel over the rows of pat_A, a lane group per cell row (16 / 32 / 64 lanes by
//                the longest row; longer rows are strided, shorter ones leave lanes idle): entry k of the row is
//                   A_D[k]  +  the upwind entries of the cell's faces whose upstream cell is column k, in cell_faces
//                   order  +  acc on the diagonal
//                in that order.  The upstream side is decided here from sign(q) (+0, -0 positive; NaN negative), as
//                upwind_discretize does, with the flags of the keyword's one "bc": a changed flux needs no
//                discretize call and no symbolic work.  Lane 0 of the group sums b_ref over the faces and writes r.
//                Algorithmic bytes: 16 nnz(pat_A) (A_D read, S written) + 4 nnz (columns) + O(Nc + Nf).
//   total flux   w q c_up (+ the Dirichlet-inflow / Neumann boundary parts) + flux_D c + bound_flux_D bc, per face
//
// No floating-point atomics; every sum has a fixed order; the PFV_EMULATE build runs the same bodies (one lane).
namespace pfv {

enum { ADV_ST_ZERO_DIAG = 0, ADV_ST_NO_UPSTREAM = 1, ADV_ST_ROBIN = 2, ADV_ST_WORDS = 3 };

// every face neighbour of every cell must be a column of the cell's row of pat_A
static void advdiff_check_pattern(pfv_ctx_impl& c) {
  stream_t s = c.stream;
  upwind_face_cells(c);
  const int64_t nc = c.nc, nf = c.nf;
  const int32_t* cf_ptr = c.cf_ptr;
  const int32_t* cf_idx = c.cf_idx;
  const int32_t* side = c.upw_side;
  const int32_t* ap = c.pat_A.indptr;
  const int32_t* ax = c.pat_A.indices;
  int32_t* st = c.status.ensure(16);
  be_memset(st, 0x7f, sizeof(int32_t), s);  // st[0]: first cell whose row misses a neighbour (or itself)
  parallel_for(s, nc, PFV_LAMBDA(int64_t cell) {
    const int a0 = ap[cell], a1 = ap[cell + 1];
    bool ok = false;
    for (int p = a0; p < a1; ++p) ok = ok || ax[p] == (int32_t)cell;
    for (int e = cf_ptr[cell]; e < cf_ptr[cell + 1] && ok; ++e) {
      const int f = cf_idx[e];
      for (int sd = 0; sd < 2 && ok; ++sd) {
        const int32_t v = side[(int64_t)sd * nf + f];
        if (v < 0) continue;
        bool found = false;
        for (int p = a0; p < a1; ++p) found = found || ax[p] == v;
        ok = found;
      }
    }
    if (!ok) atomic_min_i32(st, (int32_t)cell);
  });
  const int32_t bad = read_scalar<int32_t>(s, st);
  if (bad != 0x7f7f7f7f)
    throw Error(PFV_ERR_UNSUPPORTED, "the pattern of div @ flux does not contain the face neighbours of cell " +
                                         std::to_string(bad) + ": the upwind term has no place in it");
}

// fb = bound_flux_D bc (per face), b_D = -div fb
static void advdiff_diffusion_rhs(pfv_ctx_impl& c, const double* d_bc) {
  stream_t s = c.stream;
  const int64_t nc = c.nc, nf = c.nf;
  double* fb = c.adv_fb.ensure(nf);
  spmv(c, c.pat_bound, c.val[PFV_MAT_BOUND_FLUX], d_bc, fb);
  double* b = c.adv_bD.ensure(nc);
  const int32_t* cf_ptr = c.cf_ptr;
  const int32_t* cf_idx = c.cf_idx;
  const int8_t* cf_sgn = c.cf_sgn;
  parallel_for(s, nc, PFV_LAMBDA(int64_t cell) {
    double acc = 0.0;
    for (int e = cf_ptr[cell]; e < cf_ptr[cell + 1]; ++e) acc -= (double)cf_sgn[e] * fb[cf_idx[e]];
    b[cell] = acc;
  });
}

// the refresh: S, its diagonal, b_ref and r from the kept diffusion values and (q, w, acc, c_old, source)
static void advdiff_refresh(pfv_ctx_impl& c, const double* d_q, double w_scale, const double* d_bc, const double* d_acc,
                            const double* d_cold, const double* d_src) {
  stream_t s = c.stream;
  const int64_t nc = c.nc, nf = c.nf;
  const int32_t* cf_ptr = c.cf_ptr;
  const int32_t* cf_idx = c.cf_idx;
  const int8_t* cf_sgn = c.cf_sgn;
  const int32_t* ap = c.pat_A.indptr;
  const int32_t* ax = c.pat_A.indices;
  const int32_t* side = c.upw_side;
  const int32_t* cnt = c.upw_cnt;
  const uint8_t* flag = c.bcflag;
  const double* AD = c.val[PFV_MAT_SYSTEM];
  const double* bD = c.adv_bD;
  double* S = c.val[PFV_MAT_ADVDIFF_SYSTEM].ensure(std::max<int64_t>(c.pat_A.nnz, 1));
  double* diag = c.adv_diag.ensure(nc);
  double* rhs = c.adv_rhs.ensure(nc);
  double* bref = c.adv_bref.ensure(nc);
  int32_t* st = c.status.ensure(16);
  be_memset(st, 0x7f, sizeof(int32_t) * ADV_ST_WORDS, s);
  const int G = c.pat_A.max_row > 32 ? 64 : (c.pat_A.max_row > 16 ? 32 : 16);
  wave_for_g(G, s, nc, 0, PFV_LAMBDA(const WaveCtx& w) {
    const int64_t cell = w.item;
    const int a0 = ap[cell], alen = ap[cell + 1] - a0;
    const int e0 = cf_ptr[cell], e1 = cf_ptr[cell + 1];
    PFV_LANES(k, alen) {
      const int32_t col = ax[a0 + k];
      double v = AD[a0 + k];
      for (int e = e0; e < e1; ++e) {
        const int f = cf_idx[e];
        const double qf = d_q[f];
        const int32_t u = (qf >= 0.0) ? side[f] : side[nf + f];  // false for NaN: the negative branch
        const unsigned fl = flag[f];
        const bool kept = !(fl & PFV_BC_NEU) && !((fl & PFV_BC_DIR) && u < 0);
        if (kept && u == col) v += (double)cf_sgn[e] * (w_scale * qf);
      }
      if (col == (int32_t)cell) {
        if (d_acc) v += d_acc[cell];
        diag[cell] = v;
        if (!(v != 0.0) || !(v == v)) atomic_min_i32(st + ADV_ST_ZERO_DIAG, (int32_t)cell);
      }
      S[a0 + k] = v;
    }
    if (w.lane0()) {
      double b = 0.0;
      for (int e = e0; e < e1; ++e) {
        const int f = cf_idx[e];
        const double qf = d_q[f];
        const int32_t u = (qf >= 0.0) ? side[f] : side[nf + f];
        const unsigned fl = flag[f];
        const bool neu = (fl & PFV_BC_NEU) != 0;
        const bool dirin = (fl & PFV_BC_DIR) != 0 && u < 0;
        if (fl & PFV_BC_ROB) atomic_min_i32(st + ADV_ST_ROBIN, (int32_t)f);
        if (!neu && !dirin && u < 0) atomic_min_i32(st + ADV_ST_NO_UPSTREAM, (int32_t)f);
        if (neu || dirin) {
          double m = 0.0;  // the entry of rhs_neu + rhs_dir diag(w q) in row f
          if (neu) m = (double)(cnt[f] - cnt[nf + f]);
          if (dirin) m += w_scale * qf;
          b += (double)cf_sgn[e] * (m * d_bc[f]);
        }
      }
      bref[cell] = b;
      double r = (d_acc && d_cold) ? d_acc[cell] * d_cold[cell] : 0.0;
      r -= b;
      r += bD[cell];
      if (d_src) r += d_src[cell];
      rhs[cell] = r;
    }
  });
  int32_t sth[ADV_ST_WORDS];
  be_d2h(sth, st, sizeof(sth), s);
  if (sth[ADV_ST_ROBIN] != 0x7f7f7f7f)
    throw Error(PFV_ERR_UNSUPPORTED, "face " + std::to_string(sth[ADV_ST_ROBIN]) +
                                         " carries a Robin condition: the advection-diffusion step does not cover it");
  if (sth[ADV_ST_NO_UPSTREAM] != 0x7f7f7f7f)
    throw Error(PFV_ERR_ARGUMENT, "negative axis 1 index: -1 (face " + std::to_string(sth[ADV_ST_NO_UPSTREAM]) +
                                      " lies on the boundary, is neither Dirichlet nor Neumann and has inflow: "
                                      "no upstream cell)");
  c.advdiff_zero_diag = sth[ADV_ST_ZERO_DIAG] == 0x7f7f7f7f ? -1 : (int64_t)sth[ADV_ST_ZERO_DIAG];
  c.filled[PFV_MAT_ADVDIFF_SYSTEM] = true;
}

// right-hand side of one implicit Euler step
static void advdiff_step_rhs(pfv_ctx_impl& c, const double* d_c) {
  const double* acc = c.have_adv_acc ? c.adv_acc.p : nullptr;
  const double* src = c.have_adv_src ? c.adv_src.p : nullptr;
  const double* bref = c.adv_bref;
  const double* bD = c.adv_bD;
  double* rhs = c.adv_rhs;
  parallel_for(c.stream, c.nc, PFV_LAMBDA(int64_t cell) {
    double r = acc ? acc[cell] * d_c[cell] : 0.0;
    r -= bref[cell];
    r += bD[cell];
    if (src) r += src[cell];
    rhs[cell] = r;
  });
}

// total face flux of the transported quantity for the state d_c
static void advdiff_face_flux(pfv_ctx_impl& c, const double* d_c, double* out) {
  stream_t s = c.stream;
  const int64_t nf = c.nf;
  const int32_t* fp = c.pat_flux.indptr;
  const int32_t* fx = c.pat_flux.indices;
  const double* vf = c.val[PFV_MAT_FLUX];
  const double* fb = c.adv_fb;
  const double* q = c.adv_q;
  const double* bc = c.adv_bc;
  const double w_scale = c.adv_w;
  const int32_t* side = c.upw_side;
  const int32_t* cnt = c.upw_cnt;
  const uint8_t* flag = c.bcflag;
  parallel_for(s, nf, PFV_LAMBDA(int64_t f) {
    const double qf = q[f];
    const int32_t u = (qf >= 0.0) ? side[f] : side[nf + f];
    const unsigned fl = flag[f];
    const bool neu = (fl & PFV_BC_NEU) != 0;
    const bool dirin = (fl & PFV_BC_DIR) != 0 && u < 0;
    double t = 0.0;
    if (!neu && !dirin) t = (w_scale * qf) * d_c[u];
    if (neu || dirin) {
      double m = 0.0;
      if (neu) m = (double)(cnt[f] - cnt[nf + f]);
      if (dirin) m += w_scale * qf;
      t += m * bc[f];
    }
    for (int p = fp[f]; p < fp[f + 1]; ++p) t += vf[p] * d_c[fx[p]];
    t += fb[f];
    out[f] = t;
  });
}

}  // namespace pfv
