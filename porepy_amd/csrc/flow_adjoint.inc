// flow_adjoint.inc — the adjoint of the linear flow solve (pfv_flow_adjoint): a load on the face flux (and on the
// pressure) becomes gradients with respect to the permeability tensor of every cell, the boundary values and the source.
//
//   q = T p + B bc (+ V g),   A p = source - div (B bc + V g),   A = div T,   div = cell_faces^T
//
//   A^T mu = g_p + T^T g_q                          one transposed solve (the caller: pfv_flow_adjoint in porefv.hip)
//   z_f    = g_q[f] - sum_{e of f} sgn_e mu_c(e)
//   grad_source = mu,   grad_bc_values = B^T z
//   grad_perm[r][s][c] = sum_{e = (c, f)} z_f w_f  t_f^2 sgn_e d_r n_s / (t_e^2 |d|^2)
//
// with w_f = d q_f / d t_f as ad_flux.inc defines it and the half-face derivative of tpfa.inc
// (tpfa_transmissibility_ad).  For a TPFA discretization grad_perm is the exact gradient of the discrete problem; for
// MPFA it is the two-point product rule of the reference's AdTpfaFlux -- the approximation ad_flux_system makes for its
// Jacobian --, NOT the derivative of the MPFA matrices: that one is grad_perm_exact of pfv_flow_adjoint_exact
// (mpfa_adjoint.inc), formed from the same mu and z.
//
// The transposed products gather over a column map of the CSR pattern (entries sorted by (column, row)); nothing here
// uses floating-point atomics, every sum has a fixed order.
namespace pfv {

// ---- 1. column map of a CSR pattern: one stable radix sort of the entry list by column (the CSR order is row-major, so
// the rows of a column come out ascending)
static void colmap_build(pfv_ctx_impl& c, const CsrPattern& P, ColMap& M) {
  stream_t s = c.stream;
  const int64_t nnz = P.nnz, ncols = P.ncols, nrows = P.nrows;
  if (nnz >= (int64_t(1) << 31))
    throw Error(PFV_ERR_UNSUPPORTED, "a pattern of 2^31 entries or more has no column map");
  M.ncols = ncols;
  M.nnz = nnz;
  int32_t* colptr = M.colptr.ensure((size_t)ncols + 1);
  int32_t* pos = M.pos.ensure((size_t)std::max<int64_t>(nnz, 1));
  int32_t* row = M.row.ensure((size_t)std::max<int64_t>(nnz, 1));
  const int32_t* ip = P.indptr;
  const int32_t* ix = P.indices;
  Buf<uint32_t> kin_, kout_;
  Buf<int32_t> vin_;
  uint32_t* kin = kin_.ensure((size_t)std::max<int64_t>(nnz, 1));
  uint32_t* kout = kout_.ensure((size_t)std::max<int64_t>(nnz, 1));
  int32_t* vin = vin_.ensure((size_t)std::max<int64_t>(nnz, 1));
  parallel_for(s, nnz, PFV_LAMBDA(int64_t e) {
    kin[e] = (uint32_t)ix[e];
    vin[e] = (int32_t)e;
  });
  int bits = 1;
  while ((int64_t(1) << bits) < ncols) ++bits;
  sort_pairs(s, c.scratch, kin, kout, vin, pos, (size_t)nnz, bits);
  parallel_for(s, ncols + 1, PFV_LAMBDA(int64_t j) {
    colptr[j] = (int32_t)lower_bound_idx<uint32_t>(kout, (int)nnz, (uint32_t)j);
  });
  parallel_for(s, nnz, PFV_LAMBDA(int64_t k) {
    row[k] = upper_bound_idx<int32_t>(ip, (int)nrows + 1, pos[k]) - 1;  // the last row that starts at or before the entry
  });
  be_sync(s);  // (the sort's staging buffers are freed on return)
}

// ---- 2. y = M^T x by gather over the column map: a group of L lanes per column, the lanes' partial sums (entries
// lane, lane + L, ... of the column) combined by a butterfly of fixed shape -- the result is a function of L and the
// map alone.  The value gathers val[pos[k]] are uncoalesced (one 64-byte line per entry when the rows are long).
#ifndef PFV_EMULATE
template <int L>
__global__ void __launch_bounds__(256) k_spmv_t(int64_t ncols, const int32_t* __restrict__ colptr,
                                                const int32_t* __restrict__ pos, const int32_t* __restrict__ row,
                                                const double* __restrict__ val, const double* __restrict__ x,
                                                double* __restrict__ y) {
  const int lane = threadIdx.x % L;
  const int64_t cols_per_grid = (int64_t)gridDim.x * (256 / L);
  for (int64_t col = (int64_t)blockIdx.x * (256 / L) + threadIdx.x / L; col < ncols; col += cols_per_grid) {
    const int a = colptr[col], b = colptr[col + 1];
    double sum = 0.0;
    for (int k = a + lane; k < b; k += 2 * L) {  // two (position, row) pairs in flight per lane
      const int k2 = k + L;
      const bool ok2 = k2 < b;
      const int p1 = pos[k], r1 = row[k];
      const int p2 = ok2 ? pos[k2] : p1, r2 = ok2 ? row[k2] : r1;
      const double v1 = val[p1] * x[r1];
      const double v2 = ok2 ? val[p2] * x[r2] : 0.0;
      sum += v1;
      sum += v2;
    }
#pragma unroll
    for (int o = L / 2; o > 0; o >>= 1) sum += __shfl_xor(sum, o, L);
    if (lane == 0) y[col] = sum;
  }
}
#endif

static void spmv_transposed(pfv_ctx_impl& c, const ColMap& M, const double* val, const double* x, double* y) {
  stream_t s = c.stream;
  const int64_t ncols = M.ncols;
  if (ncols == 0) return;
  const int32_t* colptr = M.colptr;
  const int32_t* pos = M.pos;
  const int32_t* row = M.row;
#ifdef PFV_EMULATE
  parallel_for(s, ncols, PFV_LAMBDA(int64_t col) {
    double sum = 0.0;
    for (int k = colptr[col]; k < colptr[col + 1]; ++k) sum += val[pos[k]] * x[row[k]];
    y[col] = sum;
  });
#else
  // lanes per column from the mean column length, as the SpMV picks its lanes per row (linalg.inc: spmv)
  const double avg = (double)M.nnz / (double)ncols;
  int L = 64;
  if (avg <= 6) L = 4; else if (avg <= 20) L = 8; else if (avg <= 160) L = 16; else if (avg <= 512) L = 32;
  const int cols_per_block = 256 / L;
  int64_t blocks = (ncols + cols_per_block - 1) / cols_per_block;
  if (blocks > 16384) blocks = 16384;
  switch (L) {
    case 4: PFV_LAUNCH(HIP_KERNEL_NAME(k_spmv_t<4>), dim3((unsigned)blocks), dim3(256), 0, s, ncols, colptr, pos, row, val, x, y); break;
    case 8: PFV_LAUNCH(HIP_KERNEL_NAME(k_spmv_t<8>), dim3((unsigned)blocks), dim3(256), 0, s, ncols, colptr, pos, row, val, x, y); break;
    case 16: PFV_LAUNCH(HIP_KERNEL_NAME(k_spmv_t<16>), dim3((unsigned)blocks), dim3(256), 0, s, ncols, colptr, pos, row, val, x, y); break;
    case 32: PFV_LAUNCH(HIP_KERNEL_NAME(k_spmv_t<32>), dim3((unsigned)blocks), dim3(256), 0, s, ncols, colptr, pos, row, val, x, y); break;
    default: PFV_LAUNCH(HIP_KERNEL_NAME(k_spmv_t<64>), dim3((unsigned)blocks), dim3(256), 0, s, ncols, colptr, pos, row, val, x, y); break;
  }
  PFV_HIP_CHECK(hipGetLastError());
#endif
}

// ---- what the call refuses, found on the device in one pass and read with one copy: the first Robin boundary face, the
// first face flagged internal, the lowest index of a non-finite entry of load_flux, load_pressure, p and of bc_values on
// a boundary face (0x7f7f7f7f: none)
struct FlowAdjointFindings {
  int32_t robin, internal, bad_gq, bad_gp, bad_p, bad_bc, pad[2];
};
PFV_HD inline bool flow_adjoint_finite(double v) { return v - v == 0.0; }  // false for NaN and for +-inf

// The (<= 2) half-faces of every face: `first` the entry of cell_faces with the lower index (= the lower cell), `last`
// the other (equal to `first` on a boundary face; both 0x7f7f7f7f on a face without cells).  This restates the ticket /
// second / nside preamble of ad_flux_system (ad_flux.inc keeps its own: its bits are pinned by fixtures); integer
// atomics only.
static void flow_adjoint_half_faces(pfv_ctx_impl& c, int32_t* first, int32_t* last, int32_t* ecell) {
  stream_t s = c.stream;
  const int64_t nc = c.nc, nf = c.nf, ncf = c.ncf;
  const int32_t* cf_ptr = c.cf_ptr;
  const int32_t* cf_idx = c.cf_idx;
  be_memset(first, 0x7f, sizeof(int32_t) * (size_t)nf, s);
  be_memset(last, 0xff, sizeof(int32_t) * (size_t)nf, s);
  parallel_for(s, ncf, PFV_LAMBDA(int64_t e) {
    atomic_min_i32(first + cf_idx[e], (int32_t)e);
    atomic_max_i32(last + cf_idx[e], (int32_t)e);
  });
  parallel_for(s, nc, PFV_LAMBDA(int64_t cell) {
    for (int e = cf_ptr[cell]; e < cf_ptr[cell + 1]; ++e) ecell[e] = (int32_t)cell;
  });
}

static FlowAdjointFindings flow_adjoint_check(pfv_ctx_impl& c, const int32_t* first, const int32_t* last,
                                              const double* d_p, const double* d_bc, const double* d_gq,
                                              const double* d_gp) {
  stream_t s = c.stream;
  const int64_t nc = c.nc, nf = c.nf;
  const uint8_t* bcflag = c.bcflag;
  int32_t* st = c.status.ensure(16);
  be_memset(st, 0x7f, sizeof(int32_t) * 8, s);
  parallel_for(s, nf, PFV_LAMBDA(int64_t f) {
    const unsigned fl = bcflag[f];
    const bool bnd = first[f] >= 0 && first[f] != 0x7f7f7f7f && first[f] == last[f];
    if (bnd && (fl & PFV_BC_ROB)) atomic_min_i32(st + 0, (int32_t)f);
    if (fl & PFV_BC_INTERNAL) atomic_min_i32(st + 1, (int32_t)f);
    if (d_gq && !flow_adjoint_finite(d_gq[f])) atomic_min_i32(st + 2, (int32_t)f);
    if (bnd && !flow_adjoint_finite(d_bc[f])) atomic_min_i32(st + 5, (int32_t)f);
  });
  parallel_for(s, nc, PFV_LAMBDA(int64_t i) {
    if (d_gp && !flow_adjoint_finite(d_gp[i])) atomic_min_i32(st + 3, (int32_t)i);
    if (!flow_adjoint_finite(d_p[i])) atomic_min_i32(st + 4, (int32_t)i);
  });
  FlowAdjointFindings out;
  be_d2h(&out, st, sizeof(out), s);
  return out;
}

// ---- 3. face kernel: z_f and z_f w_f.  w_f = filter_f (p_diff_f + g_diff_f) - dir_f sgn_f bc_f, the sides of a face
// added in the order of ad_flux_system (lower cell_faces entry first).  vd: components of the vector source per cell.
static void flow_adjoint_faces(pfv_ctx_impl& c, const int32_t* first, const int32_t* last, const int32_t* ecell,
                               const double* d_p, const double* d_bc, const double* d_vs, int vd, const double* d_gq,
                               const double* d_mu, double* z, double* zw) {
  const int64_t nc = c.nc, nf = c.nf;
  const int8_t* cf_sgn = c.cf_sgn;
  const double* fcen = c.fcen;
  const double* ccen = c.ccen;
  const uint8_t* bcflag = c.bcflag;
  parallel_for(c.stream, nf, PFV_LAMBDA(int64_t f) {
    const int e1 = first[f], e2 = last[f];
    double zf = d_gq ? d_gq[f] : 0.0;
    if (e1 == 0x7f7f7f7f || e2 < 0) {  // a face without cells
      z[f] = zf;
      zw[f] = 0.0;
      return;
    }
    const int es[2] = {e1, e2};
    const int nside = e1 == e2 ? 1 : 2;
    double diff = 0.0, musum = 0.0;
    for (int k = 0; k < nside; ++k) {
      const int e = es[k];
      const int cell = ecell[e];
      const double sg = (double)cf_sgn[e];
      double proj = 0.0;
      if (d_vs)
        for (int r = 0; r < vd; ++r)
          proj += (fcen[(int64_t)r * nf + f] - ccen[(int64_t)r * nc + cell]) * d_vs[(int64_t)cell * vd + r];
      diff += sg * (d_p[cell] + proj);
      musum += sg * d_mu[cell];
    }
    zf -= musum;
    const unsigned fl = bcflag[f];
    const bool bnd = nside == 1;
    const bool dir = bnd && (fl & PFV_BC_DIR) && !(fl & PFV_BC_INTERNAL);
    const double filter = (bnd && !dir) ? 0.0 : 1.0;  // Neumann faces: no two-point term
    const double sgn = bnd ? (double)cf_sgn[e1] : 0.0;
    const double w = filter * diff - (dir ? sgn * d_bc[f] : 0.0);
    z[f] = zf;
    zw[f] = zf * w;
  });
}

// ---- 4. grad_perm.  inv[e] = sgn_e / t_e per half-face (one double per entry of cell_faces; the 9 nnz(cell_faces)
// derivative array of tpfa_transmissibility_ad is never formed), then one pass over the cell's half-faces in the order
// of cell_faces: t_f = 1 / (inv[first] + inv[last]) recomputed per half-face, the nine sums kept in registers.
static void flow_adjoint_grad_perm(pfv_ctx_impl& c, const int32_t* first, const int32_t* last, const double* zw,
                                   double* inv, double* gperm) {
  stream_t s = c.stream;
  const int64_t nc = c.nc, nf = c.nf;
  const int32_t* cf_ptr = c.cf_ptr;
  const int32_t* cf_idx = c.cf_idx;
  const int8_t* cf_sgn = c.cf_sgn;
  const double* fnorm = c.fnorm;
  const double* fcen = c.fcen;
  const double* ccen = c.ccen;
  const double* perm = c.perm;
  parallel_for(s, nc, PFV_LAMBDA(int64_t cell) {
    double K[3][3];
    for (int r = 0; r < 3; ++r)
      for (int q = 0; q < 3; ++q) K[r][q] = perm[(3 * r + q) * nc + cell];
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
      inv[e] = (double)cf_sgn[e] * dist / num;  // sgn_e / t_e, as tpfa_transmissibility_ad forms it
    }
  });
  parallel_for(s, nc, PFV_LAMBDA(int64_t cell) {
    double acc[9];
    for (int r = 0; r < 9; ++r) acc[r] = 0.0;
    for (int e = cf_ptr[cell]; e < cf_ptr[cell + 1]; ++e) {
      const int f = cf_idx[e];
      const double g = zw[f];
      double d[3], n[3], dist = 0.0;
      for (int r = 0; r < 3; ++r) {
        d[r] = fcen[r * nf + f] - ccen[r * nc + cell];
        n[r] = fnorm[r * nf + f];
        dist += d[r] * d[r];
      }
      const int e1 = first[f], e2 = last[f];
      double sum = inv[e1];
      if (e2 != e1) sum += inv[e2];
      const double tf = 1.0 / sum;
      // t_f^2 sgn_e / (t_e^2 |d|^2) = t_f^2 inv[e]^2 sgn_e / |d|^2
      const double wgt = g * (tf * tf * inv[e] * inv[e] * (double)cf_sgn[e] / dist);
      for (int r = 0; r < 3; ++r)
        for (int q = 0; q < 3; ++q) acc[3 * r + q] += wgt * d[r] * n[q];
    }
    for (int r = 0; r < 9; ++r) gperm[(int64_t)r * nc + cell] = acc[r];
  });
}

}  // namespace pfv
