// advdiff_adjoint.inc — the adjoint of the advection-diffusion step (pfv_advdiff_adjoint): loads on the states of
// pfv_advdiff_advance become gradients with respect to c0, source, accumulation, bc_values, the flux q, the flux scale w
// and the conductivity tensor of every cell.
//
//   forward, n = 1 .. N:   S c^n = acc o c^{n-1} - b_ref + b_D + src,   S = diag(acc) + div T_D + w div diag(q) U
//   backward, n = N .. 1:  S^T lambda^n = g^n (scattered to the cells) + acc o lambda^{n+1},   lambda^{N+1} = 0
//
//   y^n_f = lambda^n[p] - lambda^n[m]  (p / m: the cells of cell_faces sign +1 / -1 at f),  Lambda = sum_n lambda^n
//   grad_c0 = acc o lambda^1,  grad_source = Lambda,  grad_accumulation = sum_n lambda^n o (c^{n-1} - c^n)
//   grad_bc_values = -(B_D^T + (rhs_neu + rhs_dir diag(w q))^T) (cell_faces Lambda)
//   grad_flux_f = -w sum_n y^n_f cup^n_f,   grad_flux_scale = -sum_f q_f sum_n y^n_f cup^n_f = (1/w) sum_f q_f grad_flux_f
//   grad_conductivity = flow_adjoint_grad_perm(zw),   zw_f = -sum_n y^n_f w^n_f
//
// cup is the value the upwind rule takes at f (upstream c^n; bc on a Dirichlet inflow face; 0 on a Neumann face), w^n_f
// the face weight of flow_adjoint_faces for p = c^n.  grad_conductivity is exact for a TPFA diffusion; for MPFA it is the
// two-point product rule of the reference's AdTpfaFlux, NOT the derivative of the MPFA matrices.  That derivative is
//   grad_conductivity_exact = sum_n d/dK [ (z^n)^T (T_D c^n + B_D bc) ] at fixed c^n, bc,   z^n_f = -y^n_f
// (pfv_advdiff_adjoint_exact): the load z^n is formed here, the region passes are mpfa_adjoint.inc's adj_batch_body.
//
// Per step: one right-hand-side kernel, the solve (the caller), ONE pass over the faces and ONE over the cells.  No
// floating-point atomics; every sum has a fixed order; the PFV_EMULATE build runs the same bodies.
namespace pfv {

// the first Robin face and the first face flagged internal (0x7f7f7f7f: none), one pass, one read
static void advdiff_adjoint_check_faces(pfv_ctx_impl& c, int32_t& robin, int32_t& internal) {
  stream_t s = c.stream;
  const uint8_t* bcflag = c.bcflag;
  int32_t* st = c.status.ensure(16);
  be_memset(st, 0x7f, sizeof(int32_t) * 2, s);
  parallel_for(s, c.nf, PFV_LAMBDA(int64_t f) {
    const unsigned fl = bcflag[f];
    if (fl & PFV_BC_ROB) atomic_min_i32(st + 0, (int32_t)f);
    if (fl & PFV_BC_INTERNAL) atomic_min_i32(st + 1, (int32_t)f);
  });
  int32_t out[2];
  be_d2h(out, st, sizeof(out), s);
  robin = out[0];
  internal = out[1];
}

// rhs = scatter(g^n) + acc o lambda^{n+1}.  slot: position of every cell among the observation cells (-1: none;
// nullptr: every cell in order); acc nullptr: no accumulation term
static void advdiff_adjoint_rhs(pfv_ctx_impl& c, const int32_t* slot, const double* loads, const double* acc,
                                const double* lam, double* rhs) {
  parallel_for(c.stream, c.nc, PFV_LAMBDA(int64_t cell) {
    double r = 0.0;
    if (slot) {
      const int32_t m = slot[cell];
      if (m >= 0) r = loads[m];
    } else {
      r = loads[cell];
    }
    if (acc) r += acc[cell] * lam[cell];
    rhs[cell] = r;
  });
}

// The face pass of one step: s_f += y_f cup_f and zw_f -= y_f w_f.  lambda, c^n, q, the flags and bc are read once per
// face; the sides are added in the order of ad_flux_system (lower cell_faces entry first), so that w_f has the bits of
// flow_adjoint_faces.  A face without cells keeps its zeros.  sq / zw may be nullptr (not wanted).
static void advdiff_adjoint_faces(pfv_ctx_impl& c, const int32_t* first, const int32_t* last, const int32_t* ecell,
                                  const double* q, const double* bc, const double* lam, const double* cn, double* sq,
                                  double* zw) {
  const int8_t* cf_sgn = c.cf_sgn;
  const uint8_t* bcflag = c.bcflag;
  parallel_for(c.stream, c.nf, PFV_LAMBDA(int64_t f) {
    const int e1 = first[f], e2 = last[f];
    if (e1 == 0x7f7f7f7f || e2 < 0) return;
    const int es[2] = {e1, e2};
    const int nside = e1 == e2 ? 1 : 2;
    double y = 0.0, diff = 0.0, cp = 0.0, cm = 0.0;
    bool havep = false, havem = false;
    for (int k = 0; k < nside; ++k) {
      const int e = es[k];
      const int cell = ecell[e];
      const double sg = (double)cf_sgn[e];
      const double l = lam[cell], v = cn[cell];
      y += sg * l;
      diff += sg * v;
      if (cf_sgn[e] > 0) {
        cp = v;
        havep = true;
      } else {
        cm = v;
        havem = true;
      }
    }
    const unsigned fl = bcflag[f];
    if (sq) {
      const double qf = q[f];
      const bool pos = qf >= 0.0;  // false for NaN: the negative branch, as advdiff_refresh decides
      const bool haveu = pos ? havep : havem;
      const bool neu = (fl & PFV_BC_NEU) != 0;
      const bool dirin = (fl & PFV_BC_DIR) != 0 && !haveu;
      double cup = 0.0;
      if (!neu) cup = dirin ? bc[f] : (haveu ? (pos ? cp : cm) : 0.0);
      sq[f] += y * cup;
    }
    if (zw) {
      const bool bnd = nside == 1;
      const bool dir = bnd && (fl & PFV_BC_DIR) && !(fl & PFV_BC_INTERNAL);
      const double filter = (bnd && !dir) ? 0.0 : 1.0;  // Neumann faces: no two-point term
      const double sgn = bnd ? (double)cf_sgn[e1] : 0.0;
      const double w = filter * diff - (dir ? sgn * bc[f] : 0.0);
      zw[f] -= y * w;
    }
  });
}

// The cell pass of one step: Lambda += lambda, grad_accumulation += lambda o (c^{n-1} - c^n), lambda copied out.  Each
// output may be nullptr.
static void advdiff_adjoint_cells(pfv_ctx_impl& c, const double* lam, const double* cprev, const double* cn,
                                  double* Lam, double* gacc, double* mult) {
  parallel_for(c.stream, c.nc, PFV_LAMBDA(int64_t cell) {
    const double l = lam[cell];
    if (Lam) Lam[cell] += l;
    if (gacc) gacc[cell] += l * (cprev[cell] - cn[cell]);
    if (mult) mult[cell] = l;
  });
}

// Y_f = (cell_faces Lambda)_f, the sides in the order of the half-face lists
static void advdiff_adjoint_face_sum(pfv_ctx_impl& c, const int32_t* first, const int32_t* last, const int32_t* ecell,
                                     const double* Lam, double* Y) {
  const int8_t* cf_sgn = c.cf_sgn;
  parallel_for(c.stream, c.nf, PFV_LAMBDA(int64_t f) {
    const int e1 = first[f], e2 = last[f];
    double y = 0.0;
    if (e1 != 0x7f7f7f7f && e2 >= 0) {
      y = (double)cf_sgn[e1] * Lam[ecell[e1]];
      if (e2 != e1) y += (double)cf_sgn[e2] * Lam[ecell[e2]];
    }
    Y[f] = y;
  });
}

// z^n_f = -y^n_f = -(cell_faces lambda^n)_f, the load of the exact conductivity gradient (mpfa_adjoint.inc:
// adj_batch_body) for step n; the sides in the order of the half-face lists, a face without cells gets zero
static void advdiff_adjoint_exact_load(pfv_ctx_impl& c, const int32_t* first, const int32_t* last, const int32_t* ecell,
                                       const double* lam, double* z) {
  const int8_t* cf_sgn = c.cf_sgn;
  parallel_for(c.stream, c.nf, PFV_LAMBDA(int64_t f) {
    const int e1 = first[f], e2 = last[f];
    double y = 0.0;
    if (e1 != 0x7f7f7f7f && e2 >= 0) {
      y = (double)cf_sgn[e1] * lam[ecell[e1]];
      if (e2 != e1) y += (double)cf_sgn[e2] * lam[ecell[e2]];
    }
    z[f] = -y;
  });
}

// gb_f = -(gb_f + m_f Y_f) with gb = B_D^T Y on entry and m_f the entry of rhs_neu + rhs_dir diag(w q) in row f, as
// advdiff_refresh forms it
static void advdiff_adjoint_grad_bc(pfv_ctx_impl& c, const double* q, double w_scale, const double* Y, double* gb) {
  const int64_t nf = c.nf;
  const int32_t* side = c.upw_side;
  const int32_t* cnt = c.upw_cnt;
  const uint8_t* flag = c.bcflag;
  parallel_for(c.stream, nf, PFV_LAMBDA(int64_t f) {
    const double qf = q[f];
    const int32_t u = (qf >= 0.0) ? side[f] : side[nf + f];
    const unsigned fl = flag[f];
    const bool neu = (fl & PFV_BC_NEU) != 0;
    const bool dirin = (fl & PFV_BC_DIR) != 0 && u < 0;
    double m = 0.0;
    if (neu) m = (double)(cnt[f] - cnt[nf + f]);
    if (dirin) m += w_scale * qf;
    double g = gb[f];
    if (neu || dirin) g += m * Y[f];
    gb[f] = -g;
  });
}

// grad_flux = -w sq (in place) and grad_flux_scale = -sum_f q_f sq_f: a reduction of fixed shape -- kAdaParts partial
// sums over the faces f = t, t + kAdaParts, ..., then one thread adds them in order -- whatever the launch is
enum { kAdaParts = 4096 };
static void advdiff_adjoint_flux_out(pfv_ctx_impl& c, const double* q, double w_scale, double* sq, double* parts,
                                     double* total) {
  stream_t s = c.stream;
  const int64_t nf = c.nf;
  parallel_for(s, (int64_t)kAdaParts, PFV_LAMBDA(int64_t t) {
    double sum = 0.0;
    for (int64_t f = t; f < nf; f += kAdaParts) sum += q[f] * sq[f];
    parts[t] = sum;
  });
  parallel_for(s, 1, PFV_LAMBDA(int64_t) {
    double sum = 0.0;
    for (int t = 0; t < kAdaParts; ++t) sum += parts[t];
    total[0] = -sum;
  });
  parallel_for(s, nf, PFV_LAMBDA(int64_t f) { sq[f] = -(w_scale * sq[f]); });
}

// grad_c0 = acc o lambda^1 (zeros without an accumulation)
static void advdiff_adjoint_grad_c0(pfv_ctx_impl& c, const double* acc, const double* lam, double* out) {
  parallel_for(c.stream, c.nc, PFV_LAMBDA(int64_t cell) { out[cell] = acc ? acc[cell] * lam[cell] : 0.0; });
}

}  // namespace pfv
