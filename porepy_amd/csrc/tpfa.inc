// tpfa.inc — two-point flux approximation (numerics/fv/tpfa.py:84-279 of the reference): what
// Mpfa hands 1-D grids to (mpfa.py:690-712), and a discretization class of its own.  One thread
// per face; the face -> (cell, sign) lists come from one stable radix sort of the cell_faces
// entries by face (entries are cell-major, so each face's cells come out ascending).
//
//   half transmissibility of entry e = (cell c, face f, sign):  t_e = (sgn n_f)^T K_c d / |d|^2,
//   d = x_f - x_c;   t_f = 1 / sum_e 1 / t_e;   Neumann (and internal) faces: flux row zeroed.
//
// Stored patterns follow what the reference stores (explicit zeros included): flux and
// bound_pressure_cell on the cell_faces pattern, bound_flux on the diagonal of the boundary
// faces, bound_pressure_face on the diagonal of the
// faces flagged Dirichlet or Neumann, the vector-source matrices on the
// cell_faces pattern expanded by the ambient dimension.

namespace pfv {

static void tpfa_discretize(pfv_ctx_impl& c, int vd) {
  stream_t s = c.stream;
  const int64_t nc = c.nc, nf = c.nf, ncf = c.ncf;
  const int32_t* cf_ptr = c.cf_ptr;
  const int32_t* cf_idx = c.cf_idx;
  const int8_t* cf_sgn = c.cf_sgn;
  const double* fnorm = c.fnorm;
  const double* fcen = c.fcen;
  const double* fshift = c.periodic ? c.face_shift.p : nullptr;
  const int32_t* fnative = c.periodic ? c.face_native.p : nullptr;
  const double* ccen = c.ccen;
  const double* perm = c.perm;
  const uint8_t* bcflag = c.bcflag;
  int32_t* st = c.status.ensure(16);
  be_memset(st, 0, sizeof(int32_t) * 8, s);
  const bool periodic = c.periodic;
  c.have_cmap = c.have_tpos_A = false;  // (flow_adjoint.inc: properties of the patterns replaced here)

  // ---- transpose cell_faces: entries grouped by face
  Buf<uint32_t> kin, kout;
  Buf<int32_t> vin, sent, ecell;
  kin.ensure(ncf); kout.ensure(ncf); vin.ensure(ncf); sent.ensure(ncf); ecell.ensure(ncf);
  {
    uint32_t* k = kin;
    int32_t* v = vin;
    int32_t* ec = ecell;
    parallel_for(s, nc, PFV_LAMBDA(int64_t cell) {
      for (int e = cf_ptr[cell]; e < cf_ptr[cell + 1]; ++e) {
        k[e] = (uint32_t)cf_idx[e];
        v[e] = e;
        ec[e] = (int32_t)cell;
      }
    });
  }
  int bits = 1;
  while ((int64_t(1) << bits) < nf) ++bits;
  sort_pairs(s, c.scratch, kin.p, kout.p, vin.p, sent.p, (size_t)ncf, bits);

  CsrPattern& PF = c.pat_flux;
  PF.nrows = nf; PF.ncols = nc; PF.nnz = ncf; PF.max_row = 2;
  int32_t* fp = PF.indptr.ensure(nf + 1);
  int32_t* fx = PF.indices.ensure(std::max<int64_t>(ncf, 1));
  {
    const uint32_t* sk = kout;
    const int32_t* se = sent;
    const int32_t* ec = ecell;
    parallel_for(s, nf + 1, PFV_LAMBDA(int64_t f) {
      fp[f] = (int32_t)lower_bound_idx<uint32_t>(sk, (int)ncf, (uint32_t)f);
    });
    parallel_for(s, ncf, PFV_LAMBDA(int64_t p) { fx[p] = ec[se[p]]; });
  }
  // ---- diagonal patterns: boundary faces (bound_flux), every face (bound_pressure_face)
  Buf<int32_t> isb;
  Buf<int64_t> bpos;
  int32_t* ib = isb.ensure(nf + 1);
  bpos.ensure(nf + 1);
  parallel_for(s, nf, PFV_LAMBDA(int64_t f) {
    const int n = fp[f + 1] - fp[f];
    ib[f] = (n == 1) ? 1 : 0;
    if (n > 2 || (n < 1 && !periodic)) atomic_max_i32(st + 1, 1);  // (merged periodic grids leave the right faces empty)
  });
  exclusive_scan<int32_t, int64_t>(s, c.scratch, isb.p, bpos.p, (size_t)nf);
  const int64_t nb = read_scalar<int64_t>(s, bpos.p + nf);
  CsrPattern& PB = c.pat_bound;
  PB.nrows = PB.ncols = nf; PB.nnz = nb; PB.max_row = 1;
  int32_t* bp_ = PB.indptr.ensure(nf + 1);
  int32_t* bx = PB.indices.ensure(std::max<int64_t>(nb, 1));
  {
    const int64_t* pos = bpos;
    parallel_for(s, nf + 1, PFV_LAMBDA(int64_t f) {
      bp_[f] = (int32_t)pos[f];
      if (f < nf && ib[f]) bx[pos[f]] = (int32_t)f;
    });
  }
  // bound_pressure_face: the reference builds a diagonal matrix and converts it to CSR, which
  // keeps the non-zero entries only (tpfa.py:243-247): faces flagged Dirichlet or Neumann
  Buf<int32_t> isd;
  Buf<int64_t> dpos;
  int32_t* id_ = isd.ensure(nf + 1);
  dpos.ensure(nf + 1);
  parallel_for(s, nf, PFV_LAMBDA(int64_t f) { id_[f] = (bcflag[f] & (PFV_BC_DIR | PFV_BC_NEU)) ? 1 : 0; });
  exclusive_scan<int32_t, int64_t>(s, c.scratch, isd.p, dpos.p, (size_t)nf);
  const int64_t ndg = read_scalar<int64_t>(s, dpos.p + nf);
  CsrPattern& PD = c.pat_bpf;
  PD.nrows = PD.ncols = nf; PD.nnz = ndg; PD.max_row = 1;
  int32_t* dp = PD.indptr.ensure(nf + 1);
  int32_t* dx = PD.indices.ensure(std::max<int64_t>(ndg, 1));
  {
    const int64_t* pos = dpos;
    parallel_for(s, nf + 1, PFV_LAMBDA(int64_t f) {
      dp[f] = (int32_t)pos[f];
      if (f < nf && id_[f]) dx[pos[f]] = (int32_t)f;
    });
  }
  c.vs_indices_pending = false;  // (written right here)
  c.vs_implicit = false;
  CsrPattern& PV = c.pat_vs;
  PV.nrows = nf; PV.ncols = nc * vd; PV.nnz = ncf * vd; PV.max_row = 2 * vd;
  int32_t* vp = PV.indptr.ensure(nf + 1);
  int32_t* vx = PV.indices.ensure(std::max<int64_t>(ncf * vd, 1));
  parallel_for(s, nf + 1, PFV_LAMBDA(int64_t f) { vp[f] = fp[f] * vd; });
  parallel_for(s, ncf * vd, PFV_LAMBDA(int64_t q) {
    const int64_t p = q / vd;
    vx[q] = fx[p] * vd + (int32_t)(q - p * vd);
  });

  // ---- values
  double* vq = c.val[PFV_MAT_FLUX].ensure(std::max<int64_t>(ncf, 1));
  double* vt = c.val[PFV_MAT_BOUND_PRESSURE_CELL].ensure(std::max<int64_t>(ncf, 1));
  double* vqb = c.val[PFV_MAT_BOUND_FLUX].ensure(std::max<int64_t>(nb, 1));
  double* vtb = c.val[PFV_MAT_BOUND_PRESSURE_FACE].ensure(std::max<int64_t>(ndg, 1));
  double* vqv = c.val[PFV_MAT_VECTOR_SOURCE].ensure(std::max<int64_t>(ncf * vd, 1));
  double* vtv = c.val[PFV_MAT_BOUND_PRESSURE_VECTOR_SOURCE].ensure(std::max<int64_t>(ncf * vd, 1));
  {
    const int32_t* se = sent;
    const int64_t* pos = bpos;
    const int64_t* posd = dpos;
    parallel_for(s, nf, PFV_LAMBDA(int64_t f) {
      const int p0 = fp[f], n = fp[f + 1] - p0;
      if (n < 1 || n > 2) return;
      double th[2], d[2][3], sg[2];
      double inv_sum = 0.0;
      for (int j = 0; j < n; ++j) {
        const int e = se[p0 + j];
        const int cell = fx[p0 + j];
        sg[j] = (double)cf_sgn[e];
        double nk = 0.0, dd = 0.0;
        const bool far = fshift && fnative[f] >= 0 && fnative[f] != cell;  // other side of a periodic face
        for (int i = 0; i < 3; ++i) d[j][i] = fcen[i * nf + f] - (far ? fshift[i * nf + f] : 0.0) - ccen[i * nc + cell];
        for (int i = 0; i < 3; ++i) {
          double kn = 0.0;  // (K n)_i
          for (int b = 0; b < 3; ++b) kn += perm[(3 * i + b) * nc + cell] * fnorm[b * nf + f] * sg[j];
          nk += kn * d[j][i];
          dd += d[j][i] * d[j][i];
        }
        th[j] = nk / dd;
        inv_sum += 1.0 / th[j];
      }
      const double t_full = 1.0 / inv_sum;
      const uint8_t fl = bcflag[f];
      const bool dir_raw = fl & PFV_BC_DIR, neu_raw = fl & PFV_BC_NEU, internal = fl & PFV_BC_INTERNAL;
      const bool is_dir = dir_raw && !internal, is_neu = neu_raw || internal;
      const double t = is_neu ? 0.0 : t_full;
      for (int j = 0; j < n; ++j) {
        vq[p0 + j] = t * sg[j];
        vt[p0 + j] = neu_raw ? 1.0 : 0.0;
        for (int k = 0; k < vd; ++k) {
          vqv[(int64_t)(p0 + j) * vd + k] = t * d[j][k] * sg[j];
          vtv[(int64_t)(p0 + j) * vd + k] = neu_raw ? d[j][k] : 0.0;
        }
      }
      if (n == 1) {
        const double tb = is_dir ? -t_full : (is_neu ? 1.0 : 0.0);
        vqb[pos[f]] = tb * sg[0];
      }
      if (dir_raw || neu_raw) vtb[posd[f]] = dir_raw ? 1.0 : -1.0 / t_full;
    });
  }

  // ---- A = div @ flux pattern: cells sharing a face with the cell (and the cell itself)
  {
    Buf<int32_t> len;
    Buf<int64_t> ptr64;
    int32_t* ln = len.ensure(nc + 1);
    ptr64.ensure(nc + 1);
    constexpr int kMaxNb = 64;
    for (int pass = 0; pass < 2; ++pass) {
      const int32_t* ap = pass ? c.pat_A.indptr.p : nullptr;
      int32_t* ax = pass ? c.pat_A.indices.p : nullptr;
      parallel_for(s, nc, PFV_LAMBDA(int64_t cell) {
        int32_t loc[kMaxNb];
        int m = 0;
        for (int e = cf_ptr[cell]; e < cf_ptr[cell + 1]; ++e) {
          const int f = cf_idx[e];
          for (int p = fp[f]; p < fp[f + 1]; ++p) {
            const int32_t v = fx[p];
            int i = 0;
            while (i < m && loc[i] < v) ++i;
            if (i < m && loc[i] == v) continue;
            if (m >= kMaxNb) { atomic_max_i32(st + 2, 1); continue; }
            for (int q = m; q > i; --q) loc[q] = loc[q - 1];
            loc[i] = v;
            ++m;
          }
        }
        if (!ax) {
          ln[cell] = m;
          track_max_i32(st + 7, m);
        } else {
          for (int i = 0; i < m; ++i) ax[ap[cell] + i] = loc[i];
        }
      });
      if (pass == 0) {
        exclusive_scan<int32_t, int64_t>(s, c.scratch, len.p, ptr64.p, (size_t)nc);
        finish_pattern(c, c.pat_A, ptr64, nc, nc);
      }
    }
  }
  int32_t sth[8];
  be_d2h(sth, st, sizeof(sth), s);
  if (sth[1]) throw Error(PFV_ERR_CELL_SHAPE, "a face must have one or two neighbouring cells");
  if (sth[2]) throw Error(PFV_ERR_UNSUPPORTED, "more than 64 face neighbours of one cell");
  c.pat_A.max_row = sth[7];
  for (int m = 0; m < 6; ++m) c.filled[m] = true;
  c.filled[PFV_MAT_SYSTEM] = false;
}

// ---- differentiable transmissibilities (pfv_tpfa_transmissibility_ad; constitutive_laws.py:1504-1578)
// d_perm: (3,3,Nc) on the device; d_t: Nf; d_jac: 9 per cell_faces entry
static void tpfa_transmissibility_ad(pfv_ctx_impl& c, const double* d_perm, double* d_t, double* d_jac) {
  stream_t s = c.stream;
  const int64_t nc = c.nc, nf = c.nf, ncf = c.ncf;
  const int32_t* cf_ptr = c.cf_ptr;
  const int32_t* cf_idx = c.cf_idx;
  const int8_t* cf_sgn = c.cf_sgn;
  const double* fnorm = c.fnorm;
  const double* fcen = c.fcen;
  const double* ccen = c.ccen;
  // half-face quantities, entry order: 1 / t_e with its sign, and the cell of the entry
  Buf<double> inv_;
  Buf<int32_t> ecell_, vin_, sent_;
  Buf<uint32_t> kin_, kout_;
  double* inv = inv_.ensure(std::max<int64_t>(ncf, 1));
  int32_t* ecell = ecell_.ensure(std::max<int64_t>(ncf, 1));
  uint32_t* k = kin_.ensure(std::max<int64_t>(ncf, 1));
  int32_t* v = vin_.ensure(std::max<int64_t>(ncf, 1));
  parallel_for(s, nc, PFV_LAMBDA(int64_t cell) {
    double K[3][3];
    for (int r = 0; r < 3; ++r)
      for (int q = 0; q < 3; ++q) K[r][q] = d_perm[(3 * r + q) * nc + cell];
    for (int e = cf_ptr[cell]; e < cf_ptr[cell + 1]; ++e) {
      const int f = cf_idx[e];
      double d[3], n[3], dist = 0.0, num = 0.0;
      for (int r = 0; r < 3; ++r) {
        d[r] = fcen[r * nf + f] - ccen[r * nc + cell];
        n[r] = fnorm[r * nf + f];
        dist += d[r] * d[r];
      }
      for (int r = 0; r < 3; ++r)
        for (int q = 0; q < 3; ++q) num += d[r] * K[r][q] * n[q];
      inv[e] = (double)cf_sgn[e] * dist / num;  // sgn_e / t_e
      ecell[e] = (int32_t)cell;
      k[e] = (uint32_t)f;
      v[e] = e;
    }
  });
  // entries grouped by face (stable: ascending entry index within a face -> fixed summation order)
  int bits = 1;
  while ((int64_t(1) << bits) < nf) ++bits;
  uint32_t* ko = kout_.ensure(std::max<int64_t>(ncf, 1));
  int32_t* se = sent_.ensure(std::max<int64_t>(ncf, 1));
  sort_pairs(s, c.scratch, k, ko, v, se, (size_t)ncf, bits);
  parallel_for(s, nf, PFV_LAMBDA(int64_t f) {
    const int lo = lower_bound_idx<uint32_t>(ko, (int)ncf, (uint32_t)f);
    double sum = 0.0;
    for (int q = lo; q < ncf && ko[q] == (uint32_t)f; ++q) sum += inv[se[q]];
    d_t[f] = 1.0 / sum;
  });
  parallel_for(s, ncf, PFV_LAMBDA(int64_t e) {
    const int f = cf_idx[e];
    const int cell = ecell[e];
    double d[3], dist = 0.0;
    for (int r = 0; r < 3; ++r) {
      d[r] = fcen[r * nf + f] - ccen[r * nc + cell];
      dist += d[r] * d[r];
    }
    // sgn_e / t_e = inv[e]  ->  t_f^2 sgn_e / (t_e^2 |d|^2) = t_f^2 inv[e]^2 sgn_e / |d|^2
    const double tf = d_t[f];
    const double w = tf * tf * inv[e] * inv[e] * (double)cf_sgn[e] / dist;
    for (int r = 0; r < 3; ++r)
      for (int q = 0; q < 3; ++q) d_jac[9 * e + 3 * r + q] = w * d[r] * fnorm[q * nf + f];
  });
}

}  // namespace pfv
