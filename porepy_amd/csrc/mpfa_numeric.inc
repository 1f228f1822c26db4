// mpfa_numeric.inc — the MPFA-O interaction-region kernel and the face (stencil) kernel.
//
// What the reference does with ~50 global SpGEMMs (numerics/fv/mpfa.py:592-1156) is done
// here node by node.  For the interaction region of node v (cells c_j, j < deg, sub-faces
// s < n) the reference solves an (nd*deg)^2 system for sub-cell gradients
// (mpfa.py:997-1045).  We solve the algebraically identical CONDENSED system for the n
// continuity-point pressures lambda_s instead (n = nd*deg/2 for interior nodes, i.e. 8x
// fewer flops and 4x less LDS):
//
//   sub-cell j:  g_j = D_j^-1 (lambda_{faces of j} - p_j 1),  D_j rows d_h = x_cp(h) - x_c
//   flux continuity / Neumann   sum_{h in s} sgn_h omega_h . (lambda_(j) - p_j 1) = rhs
//   Robin                       ... - w A_s lambda_s                               = rhs
//   Dirichlet                   lambda_s = bc
//   with omega_h = nK_h D_j^-1 (1 x nd),  nK_h = (n_f / #nodes(f))^T K_c.
//
// The node kernel inverts A (row 1-norm scaled like the reference's
// diagonal_scaling_matrix, matrix_operations.py:1880-1906; partial pivoting) and stores the
// node's RESPONSE TABLE TV = A^-1 G (n x nd*deg): G[l][(j,b)] = sum of sgn_h nK_h[b] over the
// sub-half-faces h = (j, k) of sub-cell j on sub-face l (zero on Dirichlet rows) is the rhs a
// unit vector source in cell j leaves on the flux-continuity rows, so row s of TV is the
// pressure trace on sub-face s per unit vector source -- one row of bound_pressure_vector_source
// before the sum over the nodes of the face.  Everything else the face needs follows from rows
// of TV and two short vectors per sub-face / sub-cell:
//   vector_source row of s    QV_s = [j = j*] nK_{h*} - sum_k omega_{h*}[k] TV[r_k]   (r_k: the nd
//                             sub-faces of the sub-cell j* the flux is evaluated from)
//   flux, bound_pressure_cell q_s[j] = QV_s[j,:] . e_j,  t_s[j] = TV[s][j,:] . e_j,  e_j = D_j^-1 1
//                             (a cell pressure acts like the vector source e_j: mpfa.py:1062-1147
//                             builds both from the same nK D^-1 products)
// plus, for nodes on the boundary, the columns T[:, lb] beta_lb and A^-1[:, lb] beta_lb of the
// boundary sub-faces.  The face kernel then builds every CSR row of the six output matrices exactly
// once: contiguous 16-byte loads of the nd + 1 table rows per node of the face, one lane per output
// column, the <= nodes(f) contributions added in node order.  No atomics, no intermediate COO,
// deterministic summation order.
//
// Gauss-Jordan comes in two forms: a portable LDS-resident one (any n that fits LDS; also
// what the host emulation runs) and, on the device for n <= 64, a register-resident one
// (lane = matrix row, pivot row broadcast with v_readlane / ds_bpermute, no LDS traffic in
// the O(n^3) loop).

namespace pfv {

// carve typed arrays out of a work item's LDS block.  Pointer arithmetic only (no
// pointer<->integer casts): the compiler must keep seeing an LDS (addrspace 3) pointer,
// otherwise every access degrades to a flat_load / flat_store.
struct Carver {
  char* base;
  size_t off;
  PFV_FN explicit Carver(char* b) : base(b), off(0) {}
  template <class T>
  PFV_FN T* take(size_t n) {
    off = (off + 7) & ~size_t(7);
    T* r = reinterpret_cast<T*>(base + off);
    off += n * sizeof(T);
    return r;
  }
};

static size_t node_lds_bytes(int nmax, int degmax, int nd) {
  const size_t ld = (size_t)nmax | 1;
  size_t d = (size_t)nmax * ld + 7 * (size_t)nmax + 8 + 2 * (size_t)degmax * nd * nd;  // doubles
  size_t i = 4 * (size_t)nmax + 8;                                                 // int32 (ipiv is padded; 2 flag words)
  size_t b = (size_t)nmax + 3 * (size_t)degmax * nd;                               // bytes
  return d * 8 + i * 4 + b + 64;
}

// delta - (a0 b0 + a1 b1 + a2 b2) with the products and sums carried in double-double (error-free
// transformations: two-product by fma, two-sum): the residual of a 3 x 3 inverse to ~1e-30 instead of 1e-16
PFV_FN double residual_dd3(double delta, double a0, double b0, double a1, double b1, double a2, double b2) {
#ifdef __clang__
#pragma clang fp contract(off)  // the error-free transformations below need every product and sum rounded on its own
#endif
  double hi = delta, lo = 0.0;
  const double aa[3] = {a0, a1, a2}, bb[3] = {b0, b1, b2};
  for (int t = 0; t < 3; ++t) {
    const double p = -aa[t] * bb[t];
    const double pe = fma(-aa[t], bb[t], -p);  // exact error of the product
    const double sum = hi + p;
    const double bv = sum - hi;
    const double err = (hi - (sum - bv)) + (p - bv);  // exact error of the sum
    hi = sum;
    lo += err + pe;
  }
  return hi + lo;
}

// Inverse of the nd x nd matrix of a sub-cell's continuity-point distances (rows d_h).  Cofactor formula followed by
// one Newton step R += R (I - D R) with the residual in double-double: on sliver cells cond(D) reaches 1e3..1e5 and the
// plain formula's error cond(D) eps in omega = nK D^-1 is what the condensed system's accuracy against the reference's
// gradient-form solve is limited by (tools/fuzz_vs_reference.py, Delaunay grids: 4e-10 -> 1e-12); with the step the
// inverse is accurate to a few eps relative to its norm.  ~90 flops per sub-cell.
constexpr double kSmallCondRefine = 32.0;
PFV_FN bool invert_small(int nd, const double (*D)[3], double (*R)[3]) {
  if (nd == 2) {
    const double det = D[0][0] * D[1][1] - D[0][1] * D[1][0];
    const double id = 1.0 / det;
    double C[2][2];
    C[0][0] = D[1][1] * id;
    C[0][1] = -D[0][1] * id;
    C[1][0] = -D[1][0] * id;
    C[1][1] = D[0][0] * id;
    double E[2][2];
    for (int i = 0; i < 2; ++i)
      for (int k = 0; k < 2; ++k)
        E[i][k] = residual_dd3(i == k ? 1.0 : 0.0, D[i][0], C[0][k], D[i][1], C[1][k], 0.0, 0.0);
    for (int i = 0; i < 2; ++i)
      for (int k = 0; k < 2; ++k) R[i][k] = C[i][k] + (C[i][0] * E[0][k] + C[i][1] * E[1][k]);
    return det != 0.0 && det == det;
  }
  const double c00 = D[1][1] * D[2][2] - D[1][2] * D[2][1];
  const double c01 = D[1][2] * D[2][0] - D[1][0] * D[2][2];
  const double c02 = D[1][0] * D[2][1] - D[1][1] * D[2][0];
  const double det = D[0][0] * c00 + D[0][1] * c01 + D[0][2] * c02;
  const double id = 1.0 / det;
  double C[3][3];
  C[0][0] = c00 * id;
  C[1][0] = c01 * id;
  C[2][0] = c02 * id;
  C[0][1] = (D[0][2] * D[2][1] - D[0][1] * D[2][2]) * id;
  C[1][1] = (D[0][0] * D[2][2] - D[0][2] * D[2][0]) * id;
  C[2][1] = (D[0][1] * D[2][0] - D[0][0] * D[2][1]) * id;
  C[0][2] = (D[0][1] * D[1][2] - D[0][2] * D[1][1]) * id;
  C[1][2] = (D[0][2] * D[1][0] - D[0][0] * D[1][2]) * id;
  C[2][2] = (D[0][0] * D[1][1] - D[0][1] * D[1][0]) * id;
  if (!(det != 0.0 && det == det && id - id == 0.0)) {  // singular / non-finite: the caller flags the node
    for (int i = 0; i < 3; ++i)
      for (int k = 0; k < 3; ++k) R[i][k] = C[i][k];
    return false;
  }
  {
    // the Newton step pays on slivers only: with a Frobenius condition number ||D|| ||C|| below kSmallCondRefine the
    // cofactor inverse is already accurate to cond eps < 4e-15 of its norm (well-shaped cells: cond ~ 3..10), and the
    // ~400 instructions of the double-double residual are skipped (a wavefront in which no lane needs them jumps)
    double nd2 = 0.0, nc2 = 0.0;
    for (int i = 0; i < 3; ++i)
      for (int k = 0; k < 3; ++k) {
        nd2 += D[i][k] * D[i][k];
        nc2 += C[i][k] * C[i][k];
      }
    if (nd2 * nc2 < kSmallCondRefine * kSmallCondRefine) {
      for (int i = 0; i < 3; ++i)
        for (int k = 0; k < 3; ++k) R[i][k] = C[i][k];
      return true;
    }
  }
  double E[3][3];
  for (int i = 0; i < 3; ++i)
    for (int k = 0; k < 3; ++k)
      E[i][k] = residual_dd3(i == k ? 1.0 : 0.0, D[i][0], C[0][k], D[i][1], C[1][k], D[i][2], C[2][k]);
  for (int i = 0; i < 3; ++i)
    for (int k = 0; k < 3; ++k) R[i][k] = C[i][k] + (C[i][0] * E[0][k] + C[i][1] * E[1][k] + C[i][2] * E[2][k]);
  return true;
}

PFV_HD inline bool finite_pos(double x) { return x > 0.0 && x < 1.0e300; }
// Pivots of the row-scaled local systems (entries <= 1): below this a pivot is rounding noise of a singular system --
// the reference's LAPACK inverse raises on those (matrix_operations.py:1487-1490), so do we (status 1) instead of
// returning the inverse of noise.  Legitimate pivots of ill-conditioned but regular systems stay orders above it
// (tools/fuzz_vs_reference.py: where the verdicts differ from the reference's, both sides' matrices are garbage).
constexpr double kPivotTiny = 1.0e-13;
PFV_HD inline bool usable_pivot(double x) { return x > kPivotTiny && x < 1.0e300; }
// The condensed system is an (unpivoted) block elimination of the reference's gradient system: on badly shaped cells
// (slivers of Delaunay grids) its condition number kappa = ||A^-1||_inf (rows of A are scaled to unit 1-norm) reaches
// 1e5...1e7 while the reference's system stays at ~1e2, and the plain Gauss-Jordan inverse then loses kappa * eps
// (tools/replay_fuzz_case.py 7024: bound_flux 4e-7 off the reference).  The loss is not in the data: A is sparse (<= 2 nd
// entries per row, each a sum of <= 2 products), so residuals A x - b evaluated from the omega coefficients are
// accurate componentwise and ONE step of iterative refinement of every response column, x += A^-1 (b - A x), brings the
// result back to ~1e-12 of the reference (two steps beyond kappa 1e6).  Nodes below kRefineKappa skip it: on regular
// grids (every benchmark grid: kappa 30 typical, 1.7e3 at worst) the step costs nothing.
// Acceptance of an inverse X computed WITHOUT row exchanges (node_gj_reg2d_np): |v - A X v|_inf <= kNoPivotResidual * kappa
// for the fixed vector v of freivalds_v (|v|_inf < 2).  A stable elimination leaves ~n eps kappa = 4e-15 kappa; element
// growth of ~10 still passes, the relative error of an accepted X v stays below ~3e-14 kappa (1e-11 at kappa = 300).
constexpr double kNoPivotResidual = 5.0e-14;
constexpr int kNodeGjDefault = 5;  // PFV_NODE_GJ (3: pivoted lane grid, 5: unpivoted + verified, mpfa_numeric.inc: node_gj_reg2d_np)
constexpr double kRefineContrast = 1.0e5;  // (ratio to the first row: fires for max / min >= 1e10, may fire from 1e5 on; the 100 : 1 anisotropy times the heterogeneity of the benchmark stays below)
constexpr double kRefineKappa = 1024.0;
constexpr double kRefineKappa2 = 1.0e6;
PFV_HD inline int refine_steps_for(double kappa, int mode) {
  if (mode < 0) return 0;               // PFV_NODE_REFINE=-1: never (A/B)
  if (mode > 0) return mode;            // PFV_NODE_REFINE=k: always k steps (tests)
  return kappa > kRefineKappa2 ? 2 : (kappa > kRefineKappa ? 1 : 0);
}

struct NodeArgs {
  int nd;
  int64_t nc, nf, nn;
  double eta;
  const int32_t *order, *hp, *fp, *node_sf, *node_face, *sf_face, *fn_ptr, *nsides, *h_cell, *bp;
  const uint8_t *h_lf, *h_first, *bcflag, *bls;
  const int8_t* h_sgn;
  const double *robin, *farea, *fnorm, *fcen, *ccen, *nodes, *perm, *eta_sub;
  const double* fshift;      // periodic faces (nullptr: none), see pfv_set_periodic
  const int32_t* fnative;
  const int64_t *tptr, *tbptr;
  double *tab, *tabb;
  SfRec* rec;
  int32_t* st;
  int ablate;  // profiling only (PFV_NODE_ABLATE): 1 skip Gauss-Jordan, 2 skip finish, 4 skip setup
  const uint8_t* active;  // partial discretization: only nodes with active[v] != 0 (nullptr = all)
  int sub_bc;             // conditions per sub-face: bcflag / robin are indexed by sub-face id
  int refine;             // 0: refine where kappa asks for it; -1 never; k > 0: always k steps
  int32_t* redo;          // unpivoted elimination: nodes that fail its check, left to the pivoted body (count in st[2])
  // ... and its acceptance, kNoPivotResidual times PFV_NODE_NP_TOLX (an integer, read per call like PFV_MPSA_NP_TOLX; default
  // 1: the constant itself, bit for bit; 0: no region passes, every one of the unpivoted classes goes through the redo list)
  double np_tol = kNoPivotResidual * (double)env_int("PFV_NODE_NP_TOLX", 1);
};

// L.bg: right-hand side of sub-face lf(j, k) per unit source component b in sub-cell j, stored sub-cell by sub-cell,
// [j][k][b] (nd x nd doubles per sub-cell, contiguous: node_finish reads them as one run per (row, sub-cell) item)
PFV_HD inline int bg_index(int nd, int k, int x) {  // x = nd * j + b
  const int j = x / nd;
  return (j * nd + k) * nd + (x - j * nd);
}

struct NodeLds {
  double *A, *scale, *rowk, *colk, *robw, *etal, *beta, *om, *bg, *prow;
  int32_t *fid, *sfid, *ipiv, *firstjk, *flag;
  uint8_t *type, *lfL, *fsL;
  int8_t* sgL;
};

PFV_FN void node_carve(char* lds, int n, int ld, int nh, int nd, NodeLds& L) {
  Carver cv(lds);
  L.A = cv.take<double>((size_t)n * ld);
  L.scale = cv.take<double>(n);
  L.rowk = cv.take<double>(n);
  L.colk = cv.take<double>(n);
  L.robw = cv.take<double>(n);
  L.etal = cv.take<double>(n);
  L.beta = cv.take<double>(n);
  L.om = cv.take<double>((size_t)nh * nd);
  L.bg = cv.take<double>((size_t)nh * nd);  // [j][k][b]: rhs of sub-face lf(j,k) per unit source b in cell j (bg_index)
  L.prow = cv.take<double>(n + 8);  // pivot row of the register Gauss-Jordan (16-byte aligned: A is)
  L.fid = cv.take<int32_t>(n);
  L.sfid = cv.take<int32_t>(n);
  L.ipiv = cv.take<int32_t>(n + 4);  // the register Gauss-Jordan pads n up to a multiple of 4
  L.firstjk = cv.take<int32_t>(n);
  L.flag = cv.take<int32_t>(2);  // [0]: refinement steps asked for by the Gauss-Jordan (see kRefineKappa)
  L.type = cv.take<uint8_t>(n);
  L.lfL = cv.take<uint8_t>(nh);
  L.sgL = cv.take<int8_t>(nh);
  L.fsL = cv.take<uint8_t>(nh);
}

// classification, geometry, coefficient tables, the sub-face records, and the row-scaled matrix A in
// LDS (ND is a template parameter so that the small per-sub-cell matrices live in registers).
// ADJ (mpfa_adjoint.inc): the same geometry and coefficients for the exact permeability gradient -- nothing is written
// outside the LDS block (no table row, no sub-face record), and the sub-cell's D^-1 (adj_di, [j][i][k]) and the
// sub-half-faces' normals n_h (adj_nrm, [hh][i]) are kept in LDS beside the rest.
template <int ND, bool ADJ = false>
PFV_FN void node_setup(const NodeArgs& a, const WaveCtx& w, const NodeLds& L, int v, int h0, int nh,
                              int f0, int n, int ld, int64_t t0, double* adj_di = nullptr, double* adj_nrm = nullptr) {
  constexpr int nd = ND;
  const int deg = nh / nd;
  const int ldt = (nh + 1) & ~1;
  const int64_t nc = a.nc, nf = a.nf, nn = a.nn;
  // ---- sub-faces of the node: classify rows (mpfa.py:1452-1454 for internal faces)
  PFV_LANES(l, n) {
    const int sf = a.node_sf[f0 + l];
    const int f = a.node_face[f0 + l];
    const int nnf = a.fn_ptr[f + 1] - a.fn_ptr[f];
    const bool bnd = a.nsides[f] == 1;
    const unsigned fl = a.bcflag[a.sub_bc ? sf : f];
    const bool is_int = (fl & PFV_BC_INTERNAL) != 0;
    int t = 0;
    if (bnd) {
      if ((fl & PFV_BC_DIR) && !is_int) t = 1;
      else if ((fl & PFV_BC_ROB) && !is_int) t = 3;
      else if ((fl & PFV_BC_NEU) || is_int) t = 2;
      else { t = 2; atomic_max_i32(a.st + 1, 1); }  // boundary face without a condition
    }
    L.type[l] = (uint8_t)t;
    L.fid[l] = f;
    L.sfid[l] = sf;
    L.robw[l] = a.robin[a.sub_bc ? sf : f] * a.farea[f] / nnf;
    // continuity point: scalar eta is forced to 0 on the boundary (_fvutils.py:257-268)
    L.etal[l] = a.eta_sub ? a.eta_sub[sf] : (bnd ? 0.0 : a.eta);
    if (l == 0) L.flag[0] = 0;
  }
  w.lsync();

  // ---- sub-cells: nK, distances, omega = nK D^-1, e = D^-1 1; G entries; sub-face records
  PFV_LANES(j, deg) {
    const int cell = a.h_cell[h0 + nd * j];
    double K[3][3], D[3][3], Di[3][3], nK[3][3];
    double xc[3], xv[3];
    for (int i = 0; i < 3; ++i)
      for (int k = 0; k < 3; ++k) D[i][k] = 0.0;
    for (int i = 0; i < nd; ++i) {
      xc[i] = a.ccen[i * nc + cell];
      xv[i] = a.nodes[i * nn + v];
      for (int b = 0; b < nd; ++b) K[i][b] = a.perm[(3 * i + b) * nc + cell];
    }
    int lfj[3] = {0, 0, 0};
    for (int k = 0; k < nd; ++k) {
      const int l = a.h_lf[h0 + nd * j + k];
      lfj[k] = l;
      const int f = L.fid[l];
      const double inn = 1.0 / (a.fn_ptr[f + 1] - a.fn_ptr[f]);
      double nrm[3];
      for (int i = 0; i < nd; ++i) nrm[i] = a.fnorm[i * nf + f] * inn;
      if constexpr (ADJ)
        for (int i = 0; i < nd; ++i) adj_nrm[(nd * j + k) * nd + i] = nrm[i];
      for (int b = 0; b < nd; ++b) {
        double t = 0.0;
        for (int i = 0; i < nd; ++i) t += nrm[i] * K[i][b];
        nK[k][b] = t;
      }
      for (int i = 0; i < nd; ++i) {
        double xf = a.fcen[i * nf + f];
        if (a.fshift && a.fnative[f] >= 0 && a.fnative[f] != cell) xf -= a.fshift[i * nf + f];
        D[k][i] = xf + L.etal[l] * (xv[i] - xf) - xc[i];
      }
    }
    if (!invert_small(nd, D, Di)) atomic_max_i32(a.st + 0, v + 1);
    if constexpr (ADJ) {
      for (int i = 0; i < nd; ++i)
        for (int k2 = 0; k2 < nd; ++k2) adj_di[(nd * j + i) * nd + k2] = Di[i][k2];
    } else {
      // e_j = D^-1 1: row n of the node's table
      for (int i = 0; i < nd; ++i) {
        double e = 0.0;
        for (int k2 = 0; k2 < nd; ++k2) e += Di[i][k2];
        a.tab[t0 + (int64_t)n * ldt + nd * j + i] = e;
      }
    }
    for (int k = 0; k < nd; ++k) {
      const int hh = nd * j + k;
      const int h = h0 + hh;
      const int l = lfj[k];
      const double sg = (double)a.h_sgn[h];
      double om[3] = {0.0, 0.0, 0.0};
      for (int k2 = 0; k2 < nd; ++k2) {
        double t = 0.0;
        for (int i = 0; i < nd; ++i) t += nK[k][i] * Di[i][k2];
        om[k2] = t;
        L.om[hh * nd + k2] = t;
      }
      L.lfL[hh] = (uint8_t)l;
      L.sgL[hh] = a.h_sgn[h];
      L.fsL[hh] = a.h_first[h];
      const bool isdir = L.type[l] == 1;
      for (int b = 0; b < nd; ++b) L.bg[(j * nd + k) * nd + b] = isdir ? 0.0 : sg * nK[k][b];
      if (a.h_first[h]) L.firstjk[l] = hh;
      if constexpr (!ADJ) if (a.h_first[h]) {
        SfRec R;
        R.toff = t0;
        R.n = (uint8_t)n;
        R.ls = (uint8_t)l;
        R.jstar = (uint8_t)j;
        R.deg = (uint8_t)deg;
        R.pad = 0;
        for (int k2 = 0; k2 < 3; ++k2) {
          R.r[k2] = (uint8_t)(k2 < nd ? lfj[k2] : 0);
          R.om[k2] = om[k2];
          R.nk[k2] = k2 < nd ? nK[k][k2] : 0.0;
        }
        a.rec[L.sfid[l]] = R;
      }
    }
  }
  PFV_LANES(i, n * ld) L.A[i] = 0.0;
  w.lsync();

  // ---- assemble A: one side of every sub-face per pass -> no two lanes share a row
  for (int pass = 1; pass >= 0; --pass) {
    PFV_LANES(hh, nh) {
      if ((int)L.fsL[hh] == pass) {
        const int l = L.lfL[hh];
        if (L.type[l] != 1) {
          const int j = hh / nd;
          const double sg = (double)L.sgL[hh];
          for (int k2 = 0; k2 < nd; ++k2) L.A[l * ld + L.lfL[j * nd + k2]] += sg * L.om[hh * nd + k2];
        }
      }
    }
    w.lsync();
  }
  PFV_LANES(l, n) {
    const int t = L.type[l];
    const int f = L.fid[l];
    // Neumann / Robin data per face are shared by its sub-faces; per sub-face they are taken as given
    const double inn = a.sub_bc ? 1.0 : 1.0 / (a.fn_ptr[f + 1] - a.fn_ptr[f]);
    double beta = 0.0;
    if (t == 1) { L.A[l * ld + l] = 1.0; beta = 1.0; }
    else if (t == 2) { beta = -inn; }
    else if (t == 3) { L.A[l * ld + l] -= L.robw[l]; beta = -inn; }
    L.beta[l] = beta;
  }
  w.lsync();
  // ---- row scaling (matrix_operations.py:1880-1906)
  PFV_LANES(r, n) {
    double sum = 0.0;
    for (int cc = 0; cc < n; ++cc) sum += fabs(L.A[r * ld + cc]);
    if (!finite_pos(sum)) atomic_max_i32(a.st + 0, v + 1);
    const double sc = 1.0 / sum;
    L.scale[r] = sc;
    for (int cc = 0; cc < n; ++cc) L.A[r * ld + cc] *= sc;
  }
  w.lsync();
}

// in-place Gauss-Jordan with partial pivoting on the LDS-resident matrix
// new value of A[i][c] in pivot step k: row k becomes rowk; column k of the other rows becomes
// -f * pivinv = 0 - f * rowk[k]; everything else a - f * rowk[c]
PFV_FN double gj_new(double a, double f, double rk, bool is_row_k, bool is_col_k) {
  return is_row_k ? rk : ((is_col_k ? 0.0 : a) - f * rk);
}
// rows r0, r0 + rstep, ... of column c; four rows per trip with every LDS read issued before the
// first write, so the loads overlap instead of serialising on LDS latency (the store to A may
// alias the next load as far as the compiler knows)
PFV_FN void gj_eliminate_column(double* A, int ld, int n, int k, int c, int r0, int rstep,
                                const double* rowk, const double* colk) {
  const double rk = rowk[c];
  const bool ck = (c == k);
  int i = r0;
  for (; i + 3 * rstep < n; i += 4 * rstep) {
    const int i0 = i, i1 = i + rstep, i2 = i + 2 * rstep, i3 = i + 3 * rstep;
    const double f0 = colk[i0], f1 = colk[i1], f2 = colk[i2], f3 = colk[i3];
    const double a0 = A[i0 * ld + c], a1 = A[i1 * ld + c], a2 = A[i2 * ld + c], a3 = A[i3 * ld + c];
    A[i0 * ld + c] = gj_new(a0, f0, rk, i0 == k, ck);
    A[i1 * ld + c] = gj_new(a1, f1, rk, i1 == k, ck);
    A[i2 * ld + c] = gj_new(a2, f2, rk, i2 == k, ck);
    A[i3 * ld + c] = gj_new(a3, f3, rk, i3 == k, ck);
  }
  for (; i < n; i += rstep) A[i * ld + c] = gj_new(A[i * ld + c], colk[i], rk, i == k, ck);
}

PFV_FN void node_gj_lds(const WaveCtx& w, const NodeLds& L, int n, int ld, int v, int32_t* st, int refine = -1) {
  double* A = L.A;
  // lanes tile the block: one column per lane, the rows split over width / n lane groups (all 256
  // lanes of an MPSA workgroup stay busy); narrower groups loop over the columns instead
  const int rgroups = w.width >= n ? w.width / n : 1;
  for (int k = 0; k < n; ++k) {
    double best;
    int p = w.argmax_abs(A + k, ld, k, n, &best);
    if (!usable_pivot(best)) {
      if (w.lane0()) atomic_max_i32(st + 0, v + 1);
    }
    if (p < k || p >= n) p = k;  // (a column of NaNs leaves the device's reduction without an index: see gj_wide, mpsa.inc)
    if (w.lane0()) L.ipiv[k] = p;
    if (p != k) {
      PFV_LANES(cc, n) {
        const double t = A[k * ld + cc];
        A[k * ld + cc] = A[p * ld + cc];
        A[p * ld + cc] = t;
      }
      w.sync();
    }
    const double pivinv = 1.0 / A[k * ld + k];
    PFV_LANES(cc, n) {
      L.rowk[cc] = (cc == k) ? pivinv : A[k * ld + cc] * pivinv;
      L.colk[cc] = A[cc * ld + k];
    }
    w.sync();
    if (w.width >= n) {
      const int cc = w.lane % n, rg = w.lane / n;
      if (rg < rgroups) gj_eliminate_column(A, ld, n, k, cc, rg, rgroups, L.rowk, L.colk);
    } else {
      PFV_LANES(cc, n) gj_eliminate_column(A, ld, n, k, cc, 0, 1, L.rowk, L.colk);
    }
    w.sync();
  }
  for (int k = n - 1; k >= 0; --k) {
    const int p = L.ipiv[k];
    if (p != k) {
      PFV_LANES(r, n) {
        const double t = A[r * ld + k];
        A[r * ld + k] = A[r * ld + p];
        A[r * ld + p] = t;
      }
      w.sync();
    }
  }
  // kappa = ||A^-1||_inf of the row-scaled system -> refinement steps of node_finish (callers without a
  // refinement stage pass refine < 0 and have no flag word)
  if (refine >= 0) {
    for (int want = 1; want <= 2; ++want) {  // (all lanes that write in one round write the same value)
      PFV_LANES(r, n) {
        double sum = 0.0;
        for (int cc = 0; cc < n; ++cc) sum += fabs(A[r * ld + cc]);
        if (refine_steps_for(sum, refine) >= want) L.flag[0] = want;
      }
      w.sync();
    }
  }
}

#ifndef PFV_EMULATE
// value of x held by lane `src` (index within the lane group)
template <int G>
__device__ __forceinline__ double bcast_row(double x, int src, int gbase) {
  if constexpr (G == 64) {
    // src is wave-uniform and already in an SGPR: v_readlane with a scalar lane select
    const int lo = __builtin_amdgcn_readlane(__double2loint(x), src);
    const int hi = __builtin_amdgcn_readlane(__double2hiint(x), src);
    return __hiloint2double(hi, lo);
  } else {
    return __shfl(x, gbase + src, 64);
  }
}

// 64-bit unsigned max over a lane group with DPP moves (no LDS round trips): quad permutes, row
// rotations inside each 16-lane row, then the row broadcasts of the GFX9 DPP set.
template <int CTRL>
__device__ __forceinline__ unsigned long long dpp_move_u64(unsigned long long x) {
  int lo = (int)(unsigned)x, hi = (int)(unsigned)(x >> 32);
  lo = __builtin_amdgcn_mov_dpp(lo, CTRL, 0xf, 0xf, false);
  hi = __builtin_amdgcn_mov_dpp(hi, CTRL, 0xf, 0xf, false);
  return ((unsigned long long)(unsigned)hi << 32) | (unsigned)lo;
}
__device__ __forceinline__ unsigned long long umax64(unsigned long long a, unsigned long long b) {
  return a > b ? a : b;
}
template <int G>
__device__ __forceinline__ unsigned long long group_max_u64(unsigned long long k, int gbase) {
  k = umax64(k, dpp_move_u64<0xb1>(k));                       // quad_perm [1,0,3,2]
  k = umax64(k, dpp_move_u64<0x4e>(k));                       // quad_perm [2,3,0,1]
  if constexpr (G == 8) {
    k = umax64(k, __shfl_xor(k, 4, 8));
  } else {
    k = umax64(k, dpp_move_u64<0x124>(k));                    // row_ror:4
    k = umax64(k, dpp_move_u64<0x128>(k));                    // row_ror:8  -> every lane: row max
    if constexpr (G > 16) k = umax64(k, dpp_move_u64<0x142>(k));  // row_bcast:15
    if constexpr (G > 32) k = umax64(k, dpp_move_u64<0x143>(k));  // row_bcast:31
    if constexpr (G == 64) {
      const int lo = __builtin_amdgcn_readlane((int)(unsigned)k, 63);
      const int hi = __builtin_amdgcn_readlane((int)(unsigned)(k >> 32), 63);
      k = ((unsigned long long)(unsigned)hi << 32) | (unsigned)lo;
    } else if constexpr (G == 32) {
      k = __shfl(k, gbase + 31, 64);
    }
  }
  return k;
}

// 32-bit variant (the pivot search compares single-precision images of |a|: which of two nearly equal
// candidates wins is immaterial for partial pivoting, and v_max_u32 takes its DPP operand directly)
template <int CTRL>
__device__ __forceinline__ unsigned dpp_move_u32(unsigned x) {
  return (unsigned)__builtin_amdgcn_mov_dpp((int)x, CTRL, 0xf, 0xf, false);
}
__device__ __forceinline__ unsigned umax32(unsigned a, unsigned b) { return a > b ? a : b; }
template <int G>
__device__ __forceinline__ unsigned group_max_u32(unsigned k, int gbase) {
  k = umax32(k, dpp_move_u32<0xb1>(k));  // quad_perm [1,0,3,2]
  k = umax32(k, dpp_move_u32<0x4e>(k));  // quad_perm [2,3,0,1]
  if constexpr (G == 8) {
    k = umax32(k, (unsigned)__shfl_xor((int)k, 4, 8));
  } else {
    k = umax32(k, dpp_move_u32<0x124>(k));  // row_ror:4
    k = umax32(k, dpp_move_u32<0x128>(k));  // row_ror:8  -> every lane: row max
    if constexpr (G > 16) k = umax32(k, dpp_move_u32<0x142>(k));  // row_bcast:15
    if constexpr (G > 32) k = umax32(k, dpp_move_u32<0x143>(k));  // row_bcast:31
    if constexpr (G == 64) {
      k = (unsigned)__builtin_amdgcn_readlane((int)k, 63);
    } else if constexpr (G == 32) {
      k = (unsigned)__shfl((int)k, gbase + 31, 64);
    }
  }
  return k;
}

// Register-resident Gauss-Jordan: lane r of the group owns row r (G >= n registers per lane).
// Column slots rotate every step so the pivot column is always slot 0 and all register indices
// are static; pivot rows are never moved (implicit pivoting) and stay unscaled until the end.
// The system is padded with identity rows/columns to a multiple of 4 so that the unrolled
// column loop needs one uniform branch per 4 columns instead of one per column.
// Result (inverse of the row-scaled matrix) is written back to L.A in natural order.
// NR = column registers per lane (a multiple of 4, >= the padded size of every system of the launch):
// the kernel's VGPR budget, i.e. its occupancy, follows NR, not the lane-group width.
// BC = variant: 0 = pivot row broadcast with v_readlane / ds_bpermute per entry (two 32-bit moves per
// double), pivot search on the 64-bit image of |a|; 1 = the pivot lane stores its row to LDS once and
// every lane reads it back with broadcast loads (measured slower: 12.9 vs 11.3 ms, kept for A/B);
// 2 = as 0 with the pivot search on single-precision images (7 DPP max steps instead of ~60 instructions).
template <int G, int NR, int BC>
__device__ __forceinline__ void node_gj_reg(const WaveCtx& w, const NodeLds& L, int n, int ld, int v,
                                            int32_t* st, int refine) {
  constexpr int CH = 4;
  static_assert(NR % CH == 0 && NR <= 64, "NR");
  const int r = w.lane;
  const int gbase = (((int)threadIdx.x & 63) / G) * G;  // lane-group base inside the wavefront
  const int np = (n + CH - 1) & ~(CH - 1);  // padded size
  const int last_chunk = np / CH - 1;
  double* prow = L.prow;
  double a[NR + 1];
  a[NR] = 0.0;
#pragma unroll
  for (int c = 0; c < NR; ++c) a[c] = (r < n && c < n) ? L.A[r * ld + c] : ((r == c && r < np) ? 1.0 : 0.0);
  bool used = r >= np;
  double mypivinv = 1.0;
  int mystep = 0;
  bool bad = false;
  for (int k = 0; k < np; ++k) {
    // pivot = unused row with the largest |a[0]|: order-preserving bit pattern of |a[0]| with the
    // low 6 mantissa bits replaced by (63 - row) as tie-break; 0 marks rows that cannot be chosen
    const double mag = fabs(a[0]);
    int idx;
    if constexpr (BC == 2) {
      unsigned key = 0u;
      if (!used && mag > kPivotTiny && mag < 1.0e300) {
        const unsigned bits = __float_as_uint((float)mag) & ~63u;
        key = (bits < 64u ? 64u : bits) | (unsigned)(63 - r);
      }
      key = group_max_u32<G>(key, gbase);
      if (key == 0u) bad = true;
      idx = key ? 63 - (int)(key & 63u) : 0;
    } else {
      unsigned long long key = 0ull;
      if (!used && mag > kPivotTiny && mag < 1.0e300)
        key = ((unsigned long long)__double_as_longlong(mag) & ~63ull) | (unsigned long long)(63 - r);
      key = group_max_u64<G>(key, gbase);
      if (key == 0ull) bad = true;  // singular (or non-finite) system: flagged, result discarded
      idx = key ? 63 - (int)(key & 63ull) : 0;
    }
    int src = idx;
    if constexpr (G == 64) src = __builtin_amdgcn_readfirstlane(idx);
    const bool is_p = (r == idx);
    double piv;
    if constexpr (BC == 1) {
      if (is_p) {
#pragma unroll
        for (int cb = 0; cb < NR / CH; ++cb) {
          if (cb <= last_chunk) {
#pragma unroll
            for (int i = 0; i < CH; ++i) prow[cb * CH + i] = a[cb * CH + i];
          }
        }
      }
      // other lanes read what the pivot lane stored: no instruction is needed for that inside one
      // wavefront, but the compiler must not move the loads above the (to each lane: foreign) stores
      __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
      piv = prow[0];
    } else {
      piv = bcast_row<G>(a[0], src, gbase);
    }
    const double pivinv = 1.0 / piv;
    const double g = is_p ? 0.0 : a[0] * pivinv;
    if (is_p) {
      used = true;
      mypivinv = pivinv;
      mystep = k;
    }
    if (r == 0) L.ipiv[k] = idx;
    const double newcol = is_p ? 1.0 : -g;
#pragma unroll
    for (int cb = 0; cb < NR / CH; ++cb) {
      if (cb <= last_chunk) {
        if constexpr (BC == 1) {
          double pr[CH];  // prow[np] (read by the last chunk) is inside the buffer; its product is discarded
#pragma unroll
          for (int i = 0; i < CH; ++i) pr[i] = prow[cb * CH + 1 + i];
#pragma unroll
          for (int i = 0; i < CH - 1; ++i) {
            const int c = cb * CH + 1 + i;
            a[c - 1] = fma(-g, pr[i], a[c]);
          }
          const int clast = cb * CH + CH;
          const double upd = fma(-g, pr[CH - 1], a[clast]);
          a[clast - 1] = (cb == last_chunk) ? newcol : upd;
        } else {
#pragma unroll
          for (int i = 0; i < CH - 1; ++i) {
            const int c = cb * CH + 1 + i;
            a[c - 1] = fma(-g, bcast_row<G>(a[c], src, gbase), a[c]);
          }
          const int clast = cb * CH + CH;  // reads slot clast (a[NR] is a zero dummy), writes clast - 1
          const double upd = fma(-g, bcast_row<G>(a[clast], src, gbase), a[clast]);
          a[clast - 1] = (cb == last_chunk) ? newcol : upd;
        }
      }
    }
  }
  if (bad && r == 0) atomicMax(st + 0, v + 1);
  w.lsync();  // ipiv complete; every lane consumed its LDS row long ago
  if (r < n) {
    double rowsum = 0.0;  // row of A^-1 -> kappa = ||A^-1||_inf, see kRefineKappa
#pragma unroll
    for (int c = 0; c < NR; ++c) {
      if (c < n) {
        const double e = a[c] * mypivinv;
        L.A[mystep * ld + L.ipiv[c]] = e;
        rowsum += fabs(e);
      }
    }
    if (refine >= 0) {
      const int steps = refine_steps_for(rowsum, refine);
      if (steps >= 1) L.flag[0] = 1;
      __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
      if (steps >= 2) L.flag[0] = 2;
    }
  }
  w.lsync();
}

// ---- Register Gauss-Jordan on a two-dimensional lane grid (one node per wavefront, 32 < n <= 64).
// The lane = row form above keeps n of the 64 lanes busy and pays two v_readlane per FMA to bring the pivot row
// to every lane.  Here the 64 lanes form an 8 x 8 grid, lane (gi, gj) = 8 gi + gj holds the entries
// W[gi + 8 bi][gj + 8 bj], bi, bj < B (cyclic in both directions: B x B registers per lane, B = 5 for the 36
// unknowns of an interior node of a tetrahedral grid: 25 FMAs per lane and pivot step on all 64 lanes instead of 40
// on 36 of them).  What a pivot step moves between lanes is one row segment down the grid columns and one column
// segment along the grid rows -- 2 B values per lane through the LDS crossbar (ds_bpermute, no memory) instead of
// 2 n v_readlane.  The algorithm is the same as above value for value: implicit partial pivoting (rows never move,
// pivot rows stay unscaled until the end), the same single-precision pivot keys with the row number as tie-break,
// the same in-place inverse column; local column slots rotate once per 8 steps so that the pivot column is slot 0
// of grid column k % 8 and every register index is static.  (numpy model of the index logic: profiles/r04_gj2d_model.py)
__device__ __forceinline__ double bperm_f64(double x, int addr) {
  const int lo = __builtin_amdgcn_ds_bpermute(addr, __double2loint(x));
  const int hi = __builtin_amdgcn_ds_bpermute(addr, __double2hiint(x));
  return __hiloint2double(hi, lo);
}
__device__ __forceinline__ double readlane_f64(double x, int src) {
  const int lo = __builtin_amdgcn_readlane(__double2loint(x), src);
  const int hi = __builtin_amdgcn_readlane(__double2hiint(x), src);
  return __hiloint2double(hi, lo);
}
// 1 / x for a wave-uniform x: v_rcp_f64 and two Newton steps (full double accuracy up to the last bit; the pivot
// reciprocal only scales a row, an ulp there is below the rounding of the elimination itself)
__device__ __forceinline__ double fast_rcp_f64(double x) {
  double r = __builtin_amdgcn_rcp(x);
  r = fma(fma(-x, r, 1.0), r, r);
  r = fma(fma(-x, r, 1.0), r, r);
  return r;
}

template <int B>
__device__ __forceinline__ void node_gj_reg2d(const WaveCtx& w, const NodeLds& L, int n, int ld, int v,
                                              int32_t* st, int refine) {
  static_assert(B >= 1 && B <= 8, "B");
  const int lane = (int)threadIdx.x & 63;
  const int gi = lane >> 3, gj = lane & 7;
  double a[B][B];
#pragma unroll
  for (int bi = 0; bi < B; ++bi) {
#pragma unroll
    for (int s = 0; s < B; ++s) {
      const int r = gi + 8 * bi, c = gj + 8 * s;
      a[bi][s] = (r < n && c < n) ? L.A[r * ld + c] : (r == c ? 1.0 : 0.0);
    }
  }
  unsigned tie[B];     // 63 - row: the low bits of the pivot key
  bool used[B];
  int mystep[B];
  double mypivinv[B];
#pragma unroll
  for (int bi = 0; bi < B; ++bi) {
    const int r = gi + 8 * bi;
    tie[bi] = (unsigned)(63 - r);
    used[bi] = r >= n;
    mystep[bi] = 0;
    mypivinv[bi] = 1.0;
  }
  bool bad = false;
  const int col_addr = (lane & ~7) << 2;  // byte address (ds_bpermute) of lane (gi, 0)
  for (int k = 0; k < n; ++k) {
    const int jk = k & 7;
    const bool incol = gj == jk;
    // the pivot column's entries of my rows, from lane (gi, jk): issued first, needed only after the search
    double gc[B];
    const int gaddr = col_addr + (jk << 2);
#pragma unroll
    for (int bi = 0; bi < B; ++bi) gc[bi] = bperm_f64(a[bi][0], gaddr);
    // pivot = unused row with the largest |W[r][k]| (single-precision image, row number as tie-break)
    unsigned key = 0u;
#pragma unroll
    for (int bi = 0; bi < B; ++bi) {
      const unsigned bits = __float_as_uint((float)fabs(a[bi][0])) & ~63u;
      const unsigned kk = (bits < 64u ? 64u : bits) | tie[bi];
      key = umax32(key, used[bi] ? 0u : kk);
    }
    key = incol ? key : 0u;
    key = group_max_u32<64>(key, 0);
    const int p = 63 - (int)(key & 63u);  // wave-uniform
    const int ip = p & 7, bp = p >> 3;
    const int paddr = ((ip << 3) + gj) << 2;  // lane (ip, gj)
    const int plane = (ip << 3) + jk;         // lane holding the pivot itself
    double prow[B], piv = 1.0;
#pragma unroll
    for (int q = 0; q < B; ++q) {
      if (bp == q) {  // (scalar branch: bp is uniform)
        piv = readlane_f64(a[q][0], plane);
#pragma unroll
        for (int s = 0; s < B; ++s) prow[s] = bperm_f64(a[q][s], paddr);
      }
    }
    const double mag = fabs(piv);
    if (!(key != 0u && mag > kPivotTiny && mag < 1.0e300)) bad = true;  // singular / non-finite: flagged below
    const double pivinv = fast_rcp_f64(piv);
    const bool prow_lane = gi == ip;
    double g[B];
#pragma unroll
    for (int bi = 0; bi < B; ++bi) g[bi] = gc[bi] * pivinv;
    double newcol[B];
#pragma unroll
    for (int bi = 0; bi < B; ++bi) newcol[bi] = -g[bi];
#pragma unroll
    for (int q = 0; q < B; ++q) {
      if (bp == q) {
        g[q] = prow_lane ? 0.0 : g[q];
        newcol[q] = prow_lane ? 1.0 : newcol[q];
        used[q] = used[q] || prow_lane;
        mystep[q] = prow_lane ? k : mystep[q];
        mypivinv[q] = prow_lane ? pivinv : mypivinv[q];
      }
    }
    if (lane == 0) L.ipiv[k] = p;
#pragma unroll
    for (int bi = 0; bi < B; ++bi) {
      const double upd0 = fma(-g[bi], prow[0], a[bi][0]);
      a[bi][0] = incol ? newcol[bi] : upd0;
#pragma unroll
      for (int s = 1; s < B; ++s) a[bi][s] = fma(-g[bi], prow[s], a[bi][s]);
    }
    if (jk == 7) {  // the 8 columns of this block are done: next block's columns move to slot 0
#pragma unroll
      for (int bi = 0; bi < B; ++bi) {
        const double t = a[bi][0];
#pragma unroll
        for (int s = 0; s + 1 < B; ++s) a[bi][s] = a[bi][s + 1];
        a[bi][B - 1] = t;
      }
    }
  }
  for (int rot = n >> 3; rot < B; ++rot) {  // back to the natural slot order (B rotations in all)
#pragma unroll
    for (int bi = 0; bi < B; ++bi) {
      const double t = a[bi][0];
#pragma unroll
      for (int s = 0; s + 1 < B; ++s) a[bi][s] = a[bi][s + 1];
      a[bi][B - 1] = t;
    }
  }
  if (bad && lane == 0) atomicMax(st + 0, v + 1);
  w.lsync();  // ipiv complete; every lane consumed its entries of A long ago
  // A^-1[step of row r][pivot row of step c] = W[r][c] / pivot of r; kappa = max row sum of |A^-1|
  int steps = 0;
#pragma unroll
  for (int bi = 0; bi < B; ++bi) {
    const int r = gi + 8 * bi;
    double rowsum = 0.0;
#pragma unroll
    for (int s = 0; s < B; ++s) {
      const int c = gj + 8 * s;
      if (r < n && c < n) {
        const double e = a[bi][s] * mypivinv[bi];
        L.A[mystep[bi] * ld + L.ipiv[c]] = e;
        rowsum += fabs(e);
      }
    }
    if (refine >= 0) {  // sum over the 8 lanes of the grid row
      rowsum += __shfl_xor(rowsum, 1, 64);
      rowsum += __shfl_xor(rowsum, 2, 64);
      rowsum += __shfl_xor(rowsum, 4, 64);
      const int sneed = r < n ? refine_steps_for(rowsum, refine) : 0;
      steps = sneed > steps ? sneed : steps;
    }
  }
  if (refine >= 0) {
    if (steps >= 1) L.flag[0] = 1;
    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
    if (steps >= 2) L.flag[0] = 2;
  }
  w.lsync();
}
#endif

#ifndef PFV_EMULATE
// ---- The same elimination WITHOUT the pivot search (PFV_NODE_GJ=5: "optimistic", verified afterwards).
// The pivot of step k is the diagonal entry: row k = register row cb = k / 8 of the lanes with gi == k % 8, column k =
// the slot of column block cb in the lanes with gj == k % 8 -- with the loops over cb and jk = k % 8 unrolled EVERY
// register index, lane number and select is a compile-time constant: no keys, no DPP reduction, no scalar branch on
// the pivot's register row, no slot rotation (block cb simply addresses slot (s + cb) % B).  ~70 instructions per step
// instead of ~180.  The condensed systems of well-shaped cells are far from needing row exchanges (sub-face s pairs with
// its own flux-continuity row), but nothing guarantees it: the caller checks the inverse a posteriori -- one
// Freivalds-type product, r = v - A (X v) evaluated from the defining coefficients (node_residual_update), against
// a tolerance that admits the rounding of a stable elimination with growth <= 64 and nothing more -- and hands a node
// that fails to the pivoted body (the redo list).  Returns X = A^-1 in L.A (natural order),
// t = X v in tv[0..n), kappa = ||X||_inf (wave-uniform); `degenerate`: a pivot was zero / tiny / non-finite.
PFV_HD inline double freivalds_v(int c) { return 1.0 + 0.0625 * (double)((c * 11) & 15); }

template <int B, int CB, int JK>
__device__ __forceinline__ void gj_np_step(double (&a)[B][B], double (&mypivinv)[B], int n, int gi, int gj, int col_addr,
                                           bool& degenerate) {
  constexpr int k = 8 * CB + JK;
  if (k < n) {  // (wave-uniform)
    double gc[B], prow[B];
    const int gaddr = col_addr + (JK << 2);       // lane (gi, JK)
    const int paddr = ((JK << 3) + gj) << 2;      // lane (JK, gj)
#pragma unroll
    for (int bi = 0; bi < B; ++bi) gc[bi] = bperm_f64(a[bi][CB], gaddr);
#pragma unroll
    for (int s = 0; s < B; ++s) prow[s] = bperm_f64(a[CB][(s + CB) % B], paddr);
    const double piv = readlane_f64(a[CB][CB], 9 * JK);  // lane (JK, JK)
    const double mag = fabs(piv);
    if (!(mag > kPivotTiny && mag < 1.0e300)) degenerate = true;
    const double pivinv = fast_rcp_f64(piv);
    const bool prow_lane = gi == JK;
    const bool incol = gj == JK;
    double g[B];
#pragma unroll
    for (int bi = 0; bi < B; ++bi) g[bi] = gc[bi] * pivinv;
    g[CB] = prow_lane ? 0.0 : g[CB];
    mypivinv[CB] = prow_lane ? pivinv : mypivinv[CB];
#pragma unroll
    for (int bi = 0; bi < B; ++bi) {
      const double newcol = (bi == CB && prow_lane) ? 1.0 : -g[bi];
      const double upd0 = fma(-g[bi], prow[0], a[bi][CB]);
      a[bi][CB] = incol ? newcol : upd0;
#pragma unroll
      for (int s = 1; s < B; ++s) a[bi][(s + CB) % B] = fma(-g[bi], prow[s], a[bi][(s + CB) % B]);
    }
  }
}
template <int B, int CB>
__device__ __forceinline__ void gj_np_block(double (&a)[B][B], double (&mypivinv)[B], int n, int gi, int gj, int col_addr,
                                            bool& degenerate) {
  if constexpr (CB < B) {
    if (8 * CB < n) {
      gj_np_step<B, CB, 0>(a, mypivinv, n, gi, gj, col_addr, degenerate);
      gj_np_step<B, CB, 1>(a, mypivinv, n, gi, gj, col_addr, degenerate);
      gj_np_step<B, CB, 2>(a, mypivinv, n, gi, gj, col_addr, degenerate);
      gj_np_step<B, CB, 3>(a, mypivinv, n, gi, gj, col_addr, degenerate);
      gj_np_step<B, CB, 4>(a, mypivinv, n, gi, gj, col_addr, degenerate);
      gj_np_step<B, CB, 5>(a, mypivinv, n, gi, gj, col_addr, degenerate);
      gj_np_step<B, CB, 6>(a, mypivinv, n, gi, gj, col_addr, degenerate);
      gj_np_step<B, CB, 7>(a, mypivinv, n, gi, gj, col_addr, degenerate);
      gj_np_block<B, CB + 1>(a, mypivinv, n, gi, gj, col_addr, degenerate);
    }
  }
}

template <int B>
__device__ __forceinline__ double node_gj_reg2d_np(const WaveCtx& w, const NodeLds& L, int n, int ld, double* tv,
                                                   bool& degenerate) {
  static_assert(B >= 1 && B <= 8, "B");
  const int lane = (int)threadIdx.x & 63;
  const int gi = lane >> 3, gj = lane & 7;
  double a[B][B];
#pragma unroll
  for (int bi = 0; bi < B; ++bi) {
#pragma unroll
    for (int s = 0; s < B; ++s) {
      const int r = gi + 8 * bi, c = gj + 8 * s;
      a[bi][s] = (r < n && c < n) ? L.A[r * ld + c] : (r == c ? 1.0 : 0.0);
    }
  }
  double mypivinv[B];
#pragma unroll
  for (int bi = 0; bi < B; ++bi) mypivinv[bi] = 1.0;
  degenerate = false;
  const int col_addr = (lane & ~7) << 2;  // byte address (ds_bpermute) of lane (gi, 0)
  gj_np_block<B, 0>(a, mypivinv, n, gi, gj, col_addr, degenerate);
  w.lsync();  // every lane consumed its entries of A long ago
  // X[r][c] = W[r][c] / pivot of row r (natural order: no row ever moved); kappa = max row sum of |X|; t = X v
  double kmax = 0.0;
#pragma unroll
  for (int bi = 0; bi < B; ++bi) {
    const int r = gi + 8 * bi;
    double rowsum = 0.0, tsum = 0.0;
#pragma unroll
    for (int s = 0; s < B; ++s) {
      const int c = gj + 8 * s;
      if (r < n && c < n) {
        const double e = a[bi][s] * mypivinv[bi];
        L.A[r * ld + c] = e;
        rowsum += fabs(e);
        tsum = fma(e, freivalds_v(c), tsum);
      }
    }
    rowsum += __shfl_xor(rowsum, 1, 64);
    tsum += __shfl_xor(tsum, 1, 64);
    rowsum += __shfl_xor(rowsum, 2, 64);
    tsum += __shfl_xor(tsum, 2, 64);
    rowsum += __shfl_xor(rowsum, 4, 64);
    tsum += __shfl_xor(tsum, 4, 64);
    if (r < n && gj == 0) tv[r] = tsum;
    kmax = (r < n && rowsum > kmax) ? rowsum : kmax;
  }
  // (a NaN row sum compares false everywhere: it surfaces through the residual test, which treats NaN as a failure)
  const unsigned long long kb = group_max_u64<64>((unsigned long long)__double_as_longlong(kmax), 0);
  w.lsync();
  return __longlong_as_double((long long)kb);
}
#endif

// r -= A t for the row-scaled condensed matrix A, evaluated from its defining coefficients (omega, Robin weight,
// Dirichlet identity rows) instead of a stored copy: the Gauss-Jordan has overwritten A with its inverse, and these
// few-term sums are accurate componentwise, which is what makes the refinement step of node_finish work.
PFV_FN void node_residual_update(const WaveCtx& w, const NodeLds& L, int nh, int n, int nd, const double* t, double* r) {
  for (int pass = 1; pass >= 0; --pass) {  // one side of every sub-face per pass: no two lanes share a row
    PFV_LANES(hh, nh) {
      if ((int)L.fsL[hh] == pass) {
        const int l = L.lfL[hh];
        if (L.type[l] != 1) {
          const int jb = (hh / nd) * nd;
          double sum = 0.0;
          for (int k2 = 0; k2 < nd; ++k2) sum += L.om[hh * nd + k2] * t[L.lfL[jb + k2]];
          r[l] -= L.scale[l] * (double)L.sgL[hh] * sum;
        }
      }
    }
    w.lsync();
  }
  PFV_LANES(l, n) {
    const int ty = L.type[l];
    if (ty == 1) r[l] -= L.scale[l] * t[l];
    else if (ty == 3) r[l] += L.scale[l] * L.robw[l] * t[l];
  }
  w.lsync();
}

// (S A)^-1 S = A^-1: the column scaling goes into the right-hand sides.  Table rows TV = A^-1 G and,
// for nodes on the boundary, the boundary columns of T = -omega* A^-1 and A^-1 times beta.
template <int ND>
PFV_FN void node_finish(const NodeArgs& a, const WaveCtx& w, const NodeLds& L, int v, int nh, int n, int ld,
                        int64_t t0) {
  constexpr int nd = ND;
  const int ldt = (nh + 1) & ~1;
  const double* A = L.A;
  PFV_LANES(t, nd * nh) {  // entry t = (j nd + k) nd + b: sub-half-face hh = j nd + k
    L.bg[t] *= L.scale[L.lfL[t / nd]];
  }
  w.lsync();
  const int refine = a.refine >= 0 ? L.flag[0] : 0;
  const int b0 = a.bp[v], nb = a.bp[v + 1] - b0;
  if (refine > 0) {
    // ---- ill-conditioned node (kRefineKappa): every response column x = A^-1 b is followed by `refine` steps of
    // x += A^-1 (b - A x); one column at a time, x in L.rowk, the residual in L.colk (both free after the inverse)
    double* xv = L.rowk;
    double* rv = L.colk;
    const int64_t tb0 = nb > 0 ? a.tbptr[v] : 0;
    for (int col = 0; col < nh + nb; ++col) {
      const bool table = col < nh;
      const int x = col, kb = col - nh;
      const int jb = table ? (x / nd) * nd : 0;
      const int lb = table ? 0 : (int)a.bls[b0 + kb];
      const double sb = table ? 0.0 : L.scale[lb] * L.beta[lb];
      PFV_LANES(r, n) {
        double t = 0.0;
        if (table) {
          for (int k = 0; k < nd; ++k) t += A[r * ld + L.lfL[jb + k]] * L.bg[bg_index(nd, k, x)];
        } else {
          t = A[r * ld + lb] * sb;
        }
        xv[r] = t;
      }
      w.lsync();
      for (int it = 0; it < refine; ++it) {
        PFV_LANES(r, n) rv[r] = (!table && r == lb) ? sb : 0.0;
        w.lsync();
        if (table) {
          PFV_LANES(k, nd) rv[L.lfL[jb + k]] = L.bg[bg_index(nd, k, x)];
          w.lsync();
        }
        node_residual_update(w, L, nh, n, nd, xv, rv);
        PFV_LANES(r, n) {  // (reads rv and A^-1 only: every lane updates its own entries of x)
          double t = 0.0;
          for (int l = 0; l < n; ++l) t += A[r * ld + l] * rv[l];
          xv[r] += t;
        }
        w.lsync();
      }
      if (table) {
        PFV_LANES(r, n) a.tab[t0 + (int64_t)r * ldt + x] = xv[r];
      } else {
        PFV_LANES(r, n) {
          const int hh = L.firstjk[r];
          const int jq = (hh / nd) * nd;
          double t = 0.0;
          for (int k2 = 0; k2 < nd; ++k2) t -= L.om[hh * nd + k2] * xv[L.lfL[jq + k2]];
          a.tabb[tb0 + (int64_t)r * nb + kb] = t;
          a.tabb[tb0 + (int64_t)n * nb + (int64_t)r * nb + kb] = xv[r];
        }
      }
      w.lsync();
    }
    // ---- the response to a unit pressure in cell j is TV[:, (j, :)] . e_j with e_j = D_j^-1 1 of order cond(D_j) / h:
    // the face kernel's dot product turns the (independent) errors of the refined columns into |e_j| times as much in
    // bound_pressure_cell (measured 4e-9 on a Delaunay sliver).  So that response is solved for as a column of its own,
    // t_j = A^-1 c_j with c_j[l] = sgn_h (omega_h . 1), refined like the others, and the table entry of the largest
    // component of e_j is nudged (by ~|t| eps |e| / |e|: within its own rounding) so that the dot product returns t_j.
    double* ev0 = L.etal;  // e_j, read back by the lanes that wrote it in node_setup; nh <= 2 n entries in two arrays
    double* ev1 = L.prow;
    const int deg = nh / nd;
    PFV_LANES(j, deg) {
      for (int i = 0; i < nd; ++i) {
        const int q = nd * j + i;
        const double e = a.tab[t0 + (int64_t)n * ldt + q];
        if (q < n) ev0[q] = e; else ev1[q - n] = e;
      }
    }
    w.lsync();
    for (int j = 0; j < deg; ++j) {
      const int jb = nd * j;
      PFV_LANES(r, n) {
        double t = 0.0;
        for (int k = 0; k < nd; ++k) {
          const int hh = jb + k, l = L.lfL[hh];
          if (L.type[l] == 1) continue;
          double c = 0.0;
          for (int k2 = 0; k2 < nd; ++k2) c += L.om[hh * nd + k2];
          t += A[r * ld + l] * (L.scale[l] * (double)L.sgL[hh] * c);
        }
        xv[r] = t;
      }
      w.lsync();
      for (int it = 0; it < refine; ++it) {
        PFV_LANES(r, n) rv[r] = 0.0;
        w.lsync();
        PFV_LANES(k, nd) {
          const int hh = jb + k, l = L.lfL[hh];
          double c = 0.0;
          for (int k2 = 0; k2 < nd; ++k2) c += L.om[hh * nd + k2];
          rv[l] = (L.type[l] == 1) ? 0.0 : L.scale[l] * (double)L.sgL[hh] * c;
        }
        w.lsync();
        node_residual_update(w, L, nh, n, nd, xv, rv);
        PFV_LANES(r, n) {
          double t = 0.0;
          for (int l = 0; l < n; ++l) t += A[r * ld + l] * rv[l];
          xv[r] += t;
        }
        w.lsync();
      }
      PFV_LANES(r, n) {  // (every lane re-reads the table entries it wrote itself)
        double cur = 0.0, ebest = 0.0;
        int bbest = 0;
        for (int b = 0; b < nd; ++b) {
          const int q = jb + b;
          const double e = q < n ? ev0[q] : ev1[q - n];
          cur += a.tab[t0 + (int64_t)r * ldt + q] * e;
          if (fabs(e) > fabs(ebest)) { ebest = e; bbest = b; }
        }
        if (ebest != 0.0) a.tab[t0 + (int64_t)r * ldt + jb + bbest] += (xv[r] - cur) / ebest;
      }
      w.lsync();
    }
    return;
  }
  {
    // one item per (table row r, sub-cell j): the nd entries TV[r][nd j .. nd j + nd) are the 1 x nd row
    // (A^-1[r][lf(j, k)])_k times the nd x nd block of L.bg of the sub-cell.  A lane keeps ONE sub-cell for the whole
    // loop -- lane = g deg + j, g < G = width / deg rows per trip (deg = 24: two rows, 48 of 64 lanes) -- so that the
    // block of L.bg and the nd column positions sit in registers: a trip is nd reads of A^-1, nd^2 FMAs and nd stores.
    const int deg = nh / nd;
    const int G = deg > 0 ? w.width / deg : 0;
    if (G >= 1) {
      const int g = w.lane / deg, j = w.lane - g * deg;
      if (g < G) {
        const int jb = j * nd;
        int lf[nd];
        double bgr[nd][nd];
#pragma unroll
        for (int k = 0; k < nd; ++k) {
          lf[k] = L.lfL[jb + k];
#pragma unroll
          for (int b = 0; b < nd; ++b) bgr[k][b] = L.bg[(jb + k) * nd + b];
        }
        for (int r = g; r < n; r += G) {
          double ak[nd], t[nd];
#pragma unroll
          for (int k = 0; k < nd; ++k) ak[k] = A[r * ld + lf[k]];
#pragma unroll
          for (int b = 0; b < nd; ++b) t[b] = 0.0;
#pragma unroll
          for (int k = 0; k < nd; ++k) {  // (k outer, as the sum always ran: same rounding)
#pragma unroll
            for (int b = 0; b < nd; ++b) t[b] += ak[k] * bgr[k][b];
          }
          double* dst = a.tab + t0 + (int64_t)r * ldt + jb;
#pragma unroll
          for (int b = 0; b < nd; ++b) dst[b] = t[b];
        }
      }
    } else {  // more sub-cells than lanes: items strided over the lanes
      const int tot = n * deg;
      int idx = w.lane;
      int r = idx / deg, j = idx - r * deg;
      for (; idx < tot; idx += w.width) {
        const int jb = j * nd;
        double ak[nd], t[nd];
#pragma unroll
        for (int k = 0; k < nd; ++k) ak[k] = A[r * ld + L.lfL[jb + k]];
        const double* bgj = L.bg + jb * nd;
#pragma unroll
        for (int b = 0; b < nd; ++b) t[b] = 0.0;
#pragma unroll
        for (int k = 0; k < nd; ++k) {
#pragma unroll
          for (int b = 0; b < nd; ++b) t[b] += ak[k] * bgj[k * nd + b];
        }
        double* dst = a.tab + t0 + (int64_t)r * ldt + jb;
#pragma unroll
        for (int b = 0; b < nd; ++b) dst[b] = t[b];
        j += w.width;
        while (j >= deg) { j -= deg; ++r; }
      }
    }
  }
  if (nb > 0) {
    const int64_t tb0 = a.tbptr[v];
    PFV_LANES(idx, n * nb) {
      const int r = idx / nb, kb = idx - r * nb;
      const int lb = a.bls[b0 + kb];
      const double sb = L.scale[lb] * L.beta[lb];
      const int hh = L.firstjk[r];
      const int jb = (hh / nd) * nd;
      double t = 0.0;
      for (int k2 = 0; k2 < nd; ++k2) t -= L.om[hh * nd + k2] * A[L.lfL[jb + k2] * ld + lb];
      a.tabb[tb0 + idx] = t * sb;
      a.tabb[tb0 + (int64_t)n * nb + idx] = A[r * ld + lb] * sb;
    }
  }
}

// MODE 0: LDS Gauss-Jordan (portable); MODE G > 0: register Gauss-Jordan, G lanes per node, NR column
// registers per lane, pivot row broadcast through LDS if BC
template <int MODE, int ND, int NR = 64, int BC = 0>
PFV_FN void node_body(const NodeArgs& a, const WaveCtx& w, int64_t first) {
  int v = a.order[first + w.item];
  if (a.active && !a.active[v]) return;
  int h0 = a.hp[v], nh = a.hp[v + 1] - h0;
  int f0 = a.fp[v], n = a.fp[v + 1] - f0;
#ifndef PFV_EMULATE
  if constexpr (MODE == 0 || MODE == 64) {
    // one node per wavefront: tell the compiler these are wave-uniform (SGPRs, scalar branches)
    v = __builtin_amdgcn_readfirstlane(v);
    h0 = __builtin_amdgcn_readfirstlane(h0);
    nh = __builtin_amdgcn_readfirstlane(nh);
    f0 = __builtin_amdgcn_readfirstlane(f0);
    n = __builtin_amdgcn_readfirstlane(n);
  }
#endif
  if (n == 0) return;
  const int ld = n | 1;
  const int64_t t0 = a.tptr[v];
  NodeLds L;
  node_carve(w.lds, n, ld, nh, a.nd, L);
  if (!(a.ablate & 4)) node_setup<ND>(a, w, L, v, h0, nh, f0, n, ld, t0);
  if (!(a.ablate & 1)) {
#ifndef PFV_EMULATE
    if constexpr (MODE == 64 && BC == 5) {
      // optimistic elimination without row exchanges, checked afterwards (node_gj_reg2d_np)
      bool degenerate;
      const double kappa = node_gj_reg2d_np<(NR + 7) / 8>(w, L, n, ld, L.rowk, degenerate);
      PFV_LANES(l, n) L.colk[l] = freivalds_v(l);
      w.lsync();
      node_residual_update(w, L, nh, n, ND, L.rowk, L.colk);  // colk = v - A (X v), A from its defining coefficients
      const double tol = a.np_tol * (kappa > 1.0 ? kappa : 1.0);
      bool off = false;
      PFV_LANES(l, n) off = off || !(fabs(L.colk[l]) <= tol);  // (NaN fails)
      const bool failed = degenerate || __ballot(off) != 0ull || !(kappa == kappa);
      if (failed) {  // (wave-uniform) left to the pivoted body: check_node_status launches it over the redo list
        if (w.lane0()) a.redo[atomic_fetch_add_i32(a.st + 2, 1)] = v;
        return;
      }
      if (a.refine >= 0) {
        const int steps = refine_steps_for(kappa, a.refine);
        if (w.lane0()) L.flag[0] = steps;
      }
      w.lsync();
    } else if constexpr (MODE == 64 && BC == 3) {
      node_gj_reg2d<(NR + 7) / 8>(w, L, n, ld, v, a.st, a.refine);
    } else if constexpr (MODE > 0) {
      node_gj_reg<MODE, (NR < MODE ? NR : MODE), (BC == 3 ? 2 : BC)>(w, L, n, ld, v, a.st, a.refine);
    } else
#endif
    {
      node_gj_lds(w, L, n, ld, v, a.st, a.refine);
    }
  }
  if (!(a.ablate & 1) && a.refine == 0) {
    // Contrast trigger of the refinement (round 5): kappa is taken of the ROW-scaled system and does not see a badly
    // scaled column -- permeabilities of the cells around a node that differ by >= 1e12 left errors of up to 3e-8
    // against the reference with kappa well below kRefineKappa (tools/fuzz_vs_reference.py ... contrast), and one
    // refinement step removes them (9e-13).  The row scales 1 / |row|_1 of the flux-continuity rows carry the
    // magnitudes of K: a region whose scales differ from the first such row's by more than kRefineContrast refines.
    int ref = -1;
    for (int l = 0; l < n && ref < 0; ++l) ref = (L.type[l] != 1) ? l : -1;
    if (ref >= 0) {
      const double s0 = L.scale[ref];
      PFV_LANES(l, n) {
        const double sl = L.scale[l];
        if (L.type[l] != 1 && (sl > kRefineContrast * s0 || s0 > kRefineContrast * sl) && L.flag[0] < 1) L.flag[0] = 1;
      }
      w.lsync();
    }
  }
  if (!(a.ablate & 2)) node_finish<ND>(a, w, L, v, nh, n, ld, t0);
}

template <int G, int ND, int NR, int BC>
static void launch_node_class_reg(stream_t s, const NodeArgs& a, int64_t b0, int64_t count, size_t lds) {
#ifdef PFV_EMULATE
  wave_for<64>(s, count, lds, PFV_LAMBDA(const WaveCtx& w) { node_body<0, ND>(a, w, b0); });
#else
  if constexpr (G == 64 && BC >= 3) {
    // (the lane-grid forms: 3 wavefronts per SIMD kept by the register allocation; the unpivoted one, BC 5, hands the
    // nodes that fail its check to a.redo)
    wave_for_occ<G, 3>(s, count, lds, PFV_LAMBDA(const WaveCtx& w) { node_body<G, ND, NR, BC>(a, w, b0); });
  } else {
    wave_for<G>(s, count, lds, PFV_LAMBDA(const WaveCtx& w) { node_body<G, ND, NR, BC>(a, w, b0); });
  }
#endif
}
// mode: 0 LDS Gauss-Jordan, 1 register Gauss-Jordan with lane broadcasts, 2 with the pivot row through
// LDS, 3 lane broadcasts + 32-bit pivot search, 4 as 3 with the 8 x 8 lane grid for one-node wavefronts,
// 5 as 4 without row exchanges for 32 < n <= 48 (verified, failures to a.redo)
template <int G, int NR = G>
static void launch_node_class(stream_t s, const NodeArgs& a, int64_t b0, int64_t count, size_t lds, int mode) {
  if (mode == 0) {
    if (a.nd == 2) wave_for<64>(s, count, lds, PFV_LAMBDA(const WaveCtx& w) { node_body<0, 2>(a, w, b0); });
    else wave_for<64>(s, count, lds, PFV_LAMBDA(const WaveCtx& w) { node_body<0, 3>(a, w, b0); });
  } else if (mode == 2) {
    if (a.nd == 2) launch_node_class_reg<G, 2, NR, 1>(s, a, b0, count, lds);
    else launch_node_class_reg<G, 3, NR, 1>(s, a, b0, count, lds);
  } else if (mode == 3) {
    if (a.nd == 2) launch_node_class_reg<G, 2, NR, 2>(s, a, b0, count, lds);
    else launch_node_class_reg<G, 3, NR, 2>(s, a, b0, count, lds);
  } else if (mode == 5 && G == 64 && NR <= 48) {
    if constexpr (G == 64 && NR <= 48) {  // unpivoted lane grid, verified (node_gj_reg2d_np)
      if (a.nd == 2) launch_node_class_reg<G, 2, NR, 5>(s, a, b0, count, lds);
      else launch_node_class_reg<G, 3, NR, 5>(s, a, b0, count, lds);
    }
  } else if (mode == 4 || mode == 5) {
    if constexpr (G == 64) {
      if (a.nd == 2) launch_node_class_reg<G, 2, NR, 3>(s, a, b0, count, lds);
      else launch_node_class_reg<G, 3, NR, 3>(s, a, b0, count, lds);
    } else {
      if (a.nd == 2) launch_node_class_reg<G, 2, NR, 2>(s, a, b0, count, lds);
      else launch_node_class_reg<G, 3, NR, 2>(s, a, b0, count, lds);
    }
  } else {
    if (a.nd == 2) launch_node_class_reg<G, 2, NR, 0>(s, a, b0, count, lds);
    else launch_node_class_reg<G, 3, NR, 0>(s, a, b0, count, lds);
  }
}

// launches only (on stream s, which may be the handle's second stream); check_node_status reads the flags.
static void launch_node_kernel(pfv_ctx_impl& c, const uint8_t* active, stream_t s) {
  const int nd = c.nd;
  c.tab.ensure(std::max<int64_t>(c.tab_len, 2));
  c.tabb.ensure(std::max<int64_t>(c.tabb_len, 2));
  c.sf_rec.ensure(std::max<int64_t>(c.nsf, 1));
  be_memset(c.status.p, 0, sizeof(int32_t) * 4, s);

  NodeArgs a;
  a.nd = nd; a.nc = c.nc; a.nf = c.nf; a.nn = c.nn; a.eta = c.eta;
  a.order = c.node_order; a.hp = c.node_hptr; a.fp = c.node_fptr; a.node_sf = c.node_sf; a.node_face = c.node_face;
  a.sf_face = c.sf_face; a.fn_ptr = c.fn_ptr; a.nsides = c.face_nsides; a.h_cell = c.h_cell;
  a.bp = c.node_bptr; a.bls = c.node_bls;
  a.h_lf = c.h_lf; a.h_first = c.h_first; a.bcflag = c.bcflag; a.h_sgn = c.h_sgn;
  a.robin = c.robin; a.farea = c.farea; a.fnorm = c.fnorm; a.fcen = c.fcen; a.ccen = c.ccen;
  a.nodes = c.nodes; a.perm = c.perm; a.eta_sub = c.have_eta_sub ? c.eta_sub.p : nullptr;
  a.fshift = c.periodic ? c.face_shift.p : nullptr; a.fnative = c.periodic ? c.face_native.p : nullptr;
  a.tptr = c.node_tptr; a.tbptr = c.node_tbptr; a.tab = c.tab; a.tabb = c.tabb; a.rec = c.sf_rec;
  a.st = c.status;
  a.ablate = std::getenv("PFV_NODE_ABLATE") ? std::atoi(std::getenv("PFV_NODE_ABLATE")) : 0;
  a.active = active;
  a.sub_bc = c.subface_bc ? 1 : 0;
  a.refine = env_int("PFV_NODE_REFINE", 0);
  if (c.subface_bc) {
    a.bcflag = c.bcflag_s;
    a.robin = c.robin_s;
  }

#ifndef PFV_EMULATE
  static const bool force_lds = std::getenv("PFV_NODE_LDS_GJ") != nullptr;  // A/B switch for profiling
#else
  const bool force_lds = true;
#endif
  a.redo = nullptr;
  c.node_redo_launch = nullptr;
  size_t redo_lds = 0;
  int redo_nr = 0;
  for (int cls = 0; cls < kNumClasses; ++cls) {
    const int64_t b0 = c.class_begin[cls], b1 = c.class_begin[cls + 1];
    if (b1 <= b0) continue;
    const int nmax = std::min(kClassBounds[cls], std::max(c.max_block, 1));
    const int degmax = std::max(1, std::min(c.max_deg, 2 * nmax / nd));
    const size_t lds = node_lds_bytes(nmax, degmax, nd);
    if (lds > 160 * 1024)
      throw Error(PFV_ERR_UNSUPPORTED, "interaction region too large for LDS (more than ~140 faces meet in a node)");
#ifndef PFV_EMULATE
    {
      // PFV_NODE_GJ=5: the classes with 32 < n <= 48 eliminate without row exchanges and verify (node_gj_reg2d_np);
      // nodes that fail the check go to the redo list, which check_node_status hands to the pivoted body
      const bool optimistic = !force_lds && env_int("PFV_NODE_GJ", kNodeGjDefault) == 5 && nmax > 32 && nmax <= 48 &&
                              (a.ablate & 1) == 0;
      a.redo = optimistic ? c.node_redo.ensure(std::max<int64_t>(c.nn, 1)) : nullptr;
      if (optimistic) {
        redo_lds = std::max(redo_lds, lds);
        redo_nr = std::max(redo_nr, nmax <= 40 ? 40 : 48);
      }
    }
#endif
    // 0: lane broadcasts with a 64-bit pivot key; 1: pivot row through LDS; 2 (default): lane broadcasts, the pivot search
    // on single-precision keys (7 instead of ~60 instructions per step; near-ties within 2^-18 go to the lower row --
    // irrelevant for partial pivoting on the row-scaled systems): 11.0 against 11.3 ms, same parity
    const int gjv = env_int("PFV_NODE_GJ", kNodeGjDefault);
    // 3: as 2, and the one-node-per-wavefront classes (32 < n <= 64) on the 8 x 8 lane grid (node_gj_reg2d)
    // 5: as 3, and the classes with 32 < n <= 48 WITHOUT the pivot search, verified afterwards (node_gj_reg2d_np)
    const int mode = (force_lds || nmax > 64) ? 0 : (gjv == 1 ? 2 : (gjv == 2 ? 3 : (gjv == 3 ? 4 : (gjv == 5 ? 5 : 1))));
    const int64_t cnt = b1 - b0;
    if (nmax <= 8) launch_node_class<8>(s, a, b0, cnt, lds, mode);
    else if (nmax <= 16) launch_node_class<16>(s, a, b0, cnt, lds, mode);
    else if (nmax <= 32) launch_node_class<32>(s, a, b0, cnt, lds, mode);
    else if (nmax <= 40) launch_node_class<64, 40>(s, a, b0, cnt, lds, mode);
    else if (nmax <= 48) launch_node_class<64, 48>(s, a, b0, cnt, lds, mode);
    else launch_node_class<64, 64>(s, a, b0, cnt, lds, mode);
  }
#ifndef PFV_EMULATE
  if (redo_lds > 0) {
    NodeArgs a2 = a;
    a2.order = c.node_redo.p;
    a2.redo = nullptr;
    const int nr = redo_nr;
    const size_t lds2 = redo_lds;
    c.node_redo_launch = [a2, nr, lds2](stream_t s2, int64_t count) {
      if (nr <= 40) launch_node_class<64, 40>(s2, a2, 0, count, lds2, 4);
      else launch_node_class<64, 48>(s2, a2, 0, count, lds2, 4);
    };
  }
#endif
}

static void check_node_status(pfv_ctx_impl& c, stream_t s) {
  int32_t sth[4];
  be_d2h(sth, c.status.p, sizeof(sth), s);
  c.stats_node_redo = 0;
  if (c.node_redo_launch && sth[2] > 0 && !sth[0] && !sth[1]) {
    // nodes the unpivoted elimination left (its check failed): the pivoted body
    c.stats_node_redo = sth[2];
    c.node_redo_launch(s, sth[2]);
    be_d2h(sth, c.status.p, sizeof(sth), s);
  }
  c.node_redo_launch = nullptr;
  c.stats.node_redo = c.stats_node_redo;
  if (sth[1]) throw Error(PFV_ERR_ARGUMENT, "Boundary values should be either Dirichlet, Neumann or Robin");
  if (sth[0]) {
    // same failure the reference reports (matrix_operations.py:1487-1490)
    throw Error(PFV_ERR_SINGULAR, "Error in inversion of local linear systems (node " +
                                      std::to_string(sth[0] - 1) + ")");
  }
}

static void run_node_kernel(pfv_ctx_impl& c, const uint8_t* active = nullptr) {
  launch_node_kernel(c, active, c.stream);
  check_node_status(c, c.stream);
}

// ------------------------------------------------------------------------------------ face
struct FaceArgs {
  const int32_t *fn_ptr, *fn_idx, *ip, *bip, *bix, *bp, *bfc, *order;
  const uint8_t* colpairs;
  int64_t cp_stride;
  const SfRec* rec;
  const int64_t* tbptr;
  const double *tab, *tabb;
  double *vq, *vt, *vqb, *vtb, *vqv, *vtv;
  int maxrow, maxbrow, maxfn, maxpairs;
};

struct alignas(16) D2 { double x, y; };

struct FaceLds {  // byte offsets into the work item's LDS block
  size_t rec, qv, tv, ev, off, off2, bidx, total;
};
static FaceLds face_lds_layout(int maxfn, int maxpairs, int maxbrow, int nd) {
  FaceLds L;
  size_t o = 0;
  L.rec = o; o += sizeof(SfRec) * (size_t)maxfn;
  L.qv = o; o += 8 * (size_t)nd * maxpairs;  // [(node, cell) pair][component]
  L.tv = o; o += 8 * (size_t)nd * maxpairs;
  L.ev = o; o += 8 * (size_t)nd * maxpairs;
  L.off = o; o += 4 * (size_t)(maxfn + 1);
  L.off2 = o; o += 4 * (size_t)(maxfn + 1);
  L.bidx = o; o += 4 * (size_t)maxbrow;
  L.total = (o + 15) & ~size_t(15);
  return L;
}

// One wavefront per face.  Lanes first run over pairs of table columns of the face's nodes: for
// (node i, columns x, x + 1) the nd rows r_k of the node's table and its e-row are read with 16-byte
// loads (contiguous over the lanes), combined into the vector-source entries QV, the trace entries TV
// (already averaged over the nodes of the face) and e, and left in LDS indexed by (pair, component).
// Then lanes run over the CSR row; the symbolic phase recorded for every column which pair of each node
// feeds it, so a column adds its <= nodes(f) contributions in node order: deterministic, coalesced
// stores, no searches, ~5 KB of LDS per face.
template <int ND>
PFV_FN void face_body(const FaceArgs& A, const FaceLds& SL, const WaveCtx& w) {
  const int64_t f = A.order[w.item];
  int a = A.fn_ptr[f], nnf = A.fn_ptr[f + 1] - a;
  int p0 = A.ip[f], len = A.ip[f + 1] - p0;
  int q0 = A.bip[f], blen = A.bip[f + 1] - q0;
#ifndef PFV_EMULATE
  if (w.width == 64) {  // one face per wavefront: wave-uniform values belong in SGPRs
    a = __builtin_amdgcn_readfirstlane(a);
    nnf = __builtin_amdgcn_readfirstlane(nnf);
    p0 = __builtin_amdgcn_readfirstlane(p0);
    len = __builtin_amdgcn_readfirstlane(len);
    q0 = __builtin_amdgcn_readfirstlane(q0);
    blen = __builtin_amdgcn_readfirstlane(blen);
  }
#endif
  const double inn = 1.0 / nnf;
  SfRec* recL = reinterpret_cast<SfRec*>(w.lds + SL.rec);
  double* QV = reinterpret_cast<double*>(w.lds + SL.qv);
  double* TV = reinterpret_cast<double*>(w.lds + SL.tv);
  double* EV = reinterpret_cast<double*>(w.lds + SL.ev);
  int32_t* offL = reinterpret_cast<int32_t*>(w.lds + SL.off);
  int32_t* off2 = reinterpret_cast<int32_t*>(w.lds + SL.off2);
  int32_t* bidx = reinterpret_cast<int32_t*>(w.lds + SL.bidx);
  const int maxfn = A.maxfn;

  {  // the records of the face's sub-faces: nnf contiguous 64-byte lines
    const double* src = reinterpret_cast<const double*>(A.rec + a);
    double* dst = reinterpret_cast<double*>(recL);
    PFV_LANES(t, nnf * 8) dst[t] = src[t];
  }
  PFV_LANES(i, blen) bidx[i] = A.bix[q0 + i];
  w.sync();
  int m = 0, m2 = 0;
  for (int i = 0; i < nnf; ++i) {
    if (w.lane0()) { offL[i] = m; off2[i] = m2; }
    const int deg = recL[i].deg;
    m += deg;
    m2 += (ND * deg + 1) >> 1;
  }
  if (w.lane0()) { offL[nnf] = m; off2[nnf] = m2; }
  w.sync();

  // ---- table rows -> QV, TV, e per (pair, component)
  PFV_LANES(t, m2) {
    int i = 0;
    while (i + 1 < nnf && t >= off2[i + 1]) ++i;
    const int x0 = 2 * (t - off2[i]);
    const SfRec& R = recL[i];
    const int nh = ND * (int)R.deg, ldt = (nh + 1) & ~1;
    const double* base = A.tab + R.toff;
    D2 rv[ND];
#pragma unroll
    for (int k = 0; k < ND; ++k) rv[k] = *reinterpret_cast<const D2*>(base + (int)R.r[k] * ldt + x0);
    const D2 ee = *reinterpret_cast<const D2*>(base + (int)R.n * ldt + x0);
    const int ls = R.ls, js = R.jstar;
    int ksel = 0;
#pragma unroll
    for (int k = 1; k < ND; ++k) ksel = ((int)R.r[k] == ls) ? k : ksel;
    double tvx = rv[0].x, tvy = rv[0].y;
#pragma unroll
    for (int k = 1; k < ND; ++k) {
      tvx = (ksel == k) ? rv[k].x : tvx;
      tvy = (ksel == k) ? rv[k].y : tvy;
    }
    double sx = 0.0, sy = 0.0;
#pragma unroll
    for (int k = 0; k < ND; ++k) {
      sx += R.om[k] * rv[k].x;
      sy += R.om[k] * rv[k].y;
    }
    const int flat = ND * offL[i] + x0;
    {
      const int j = x0 / ND, b = x0 - ND * j;
      QV[flat] = ((j == js) ? R.nk[b] : 0.0) - sx;
      TV[flat] = tvx * inn;
      EV[flat] = ee.x;
    }
    if (x0 + 1 < nh) {
      const int j = (x0 + 1) / ND, b = x0 + 1 - ND * j;
      QV[flat + 1] = ((j == js) ? R.nk[b] : 0.0) - sy;
      TV[flat + 1] = tvy * inn;
      EV[flat + 1] = ee.y;
    }
  }
  w.sync();

  // ---- CSR rows: add the pairs feeding every column in node order; coalesced stores
  const uint8_t* cp = A.colpairs + (A.cp_stride ? f * A.cp_stride : (int64_t)p0 * maxfn);
  if (A.vq) {
    PFV_LANES(k, len) {
      double q = 0.0, t = 0.0;
      for (int i = 0; i < nnf; ++i) {
        const int e = cp[k * maxfn + i];
        if (e != 0xff) {
#pragma unroll
          for (int b = 0; b < ND; ++b) {
            const double ev = EV[ND * e + b];
            q += QV[ND * e + b] * ev;
            t += TV[ND * e + b] * ev;
          }
        }
      }
      A.vq[p0 + k] = q;
      A.vt[p0 + k] = t;
    }
  }
  if (A.vqv) {
    PFV_LANES(x, len * ND) {
      const int k = x / ND, b = x - k * ND;
      double qv = 0.0, tv = 0.0;
      for (int i = 0; i < nnf; ++i) {
        const int e = cp[k * maxfn + i];
        if (e != 0xff) {
          qv += QV[ND * e + b];
          tv += TV[ND * e + b];
        }
      }
      A.vqv[(int64_t)p0 * ND + x] = qv;
      A.vtv[(int64_t)p0 * ND + x] = tv;
    }
  }
  // ---- boundary-face columns (bound_flux, bound_pressure_face); only faces near the boundary
  if (A.vqb) {
    PFV_LANES(pos, blen) {
      const int fb = bidx[pos];
      double q = 0.0, t = 0.0;
      for (int i = 0; i < nnf; ++i) {
        const int v = A.fn_idx[a + i];
        const int b0 = A.bp[v], nb = A.bp[v + 1] - b0;
        const int k = lower_bound_idx<int32_t>(A.bfc + b0, nb, fb);
        if (k < nb && A.bfc[b0 + k] == fb) {
          const int64_t tb0 = A.tbptr[v] + (int64_t)recL[i].ls * nb + k;
          q += A.tabb[tb0];
          t += A.tabb[tb0 + (int64_t)recL[i].n * nb];
        }
      }
      A.vqb[q0 + pos] = q;
      A.vtb[q0 + pos] = t * inn;
    }
  }
}

#ifndef PFV_EMULATE
// ---- The same face computation as a software-pipelined persistent kernel (device only; face_body above
// stays the portable statement, the path of partial updates and 2-D grids, and the A/B reference:
// PFV_FACE_PIPE=0).  face_body spends 84 % of its wave cycles parked on five dependent memory levels per
// face (order -> row pointers -> sub-face records -> table rows -> column map; PMC: SQ_WAIT_ANY).  Here a
// wavefront walks its faces with the levels of the NEXT faces already in flight: the face record two
// faces ahead, the sub-face records and the column map one face ahead, both parked in registers; only the
// table rows remain a dependent load.  A workgroup is one wavefront, so LDS phases are separated by a
// wavefront-scope fence (LDS operations of one wavefront execute in order) instead of __syncthreads(),
// whose vmcnt(0) would drain the prefetches.
struct FacePipeArgs {
  const FaceRec* frec;
  const SfRec* rec;
  const uint8_t* colpairs;
  const double *tab, *tabb;
  const int64_t* tbptr;
  const int32_t *fn_idx, *bix, *bp, *bfc;
  double *vq, *vt, *vqb, *vtb, *vqv, *vtv;
  int64_t n;
  int64_t cp_stride;  // bytes between the column maps of consecutive faces (0: compact, at indptr * maxfn)
  int maxfn;
  FaceLds SL;
  size_t cpw_off;  // LDS offset of the column-map words
  int run;         // consecutive faces of the processing order one wavefront takes per grab (PFV_FACE_RUN)
  int32_t* ctr;    // != nullptr: runs are handed out by one atomic counter per XCD (64 bytes apart) instead of by a
                   // fixed stride -- the wavefronts of an XCD then stay within one narrow window of the order
                   // whatever their individual speeds (PFV_FACE_DYN)
};

__device__ __forceinline__ void wave_sync_lds() {
  __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
  __builtin_amdgcn_wave_barrier();
}

// CSR rows of one face from the LDS arrays.  NNF > 0: every face node contributes (static unroll, all
// LDS reads of a column issued together; a missing pair reads slot 0 with weight 0); NNF = 0: any face.
template <int ND, int NNF>
__device__ __forceinline__ void face_pipe_columns(const FacePipeArgs& P, const uint8_t* cp, const double* QV,
                                                  const double* TV, const double* EV, int lane, int len, int p0,
                                                  int nnf_dyn = NNF, int maxfn_dyn = NNF) {
  const int nnf = NNF > 0 ? NNF : nnf_dyn;
  const int maxfn = NNF > 0 ? NNF : maxfn_dyn;
  if (P.vq) {
    for (int k = lane; k < len; k += 64) {
      double q = 0.0, t = 0.0;
      if constexpr (NNF > 0) {
        int e[NNF];
#pragma unroll
        for (int i = 0; i < NNF; ++i) e[i] = cp[k * NNF + i];
        double qa[NNF][ND], ta[NNF][ND], ea[NNF][ND];
#pragma unroll
        for (int i = 0; i < NNF; ++i) {
          const int ee = e[i] == 0xff ? 0 : e[i];
#pragma unroll
          for (int b = 0; b < ND; ++b) {
            qa[i][b] = QV[ND * ee + b];
            ta[i][b] = TV[ND * ee + b];
            ea[i][b] = EV[ND * ee + b];
          }
        }
#pragma unroll
        for (int i = 0; i < NNF; ++i) {
          if (e[i] != 0xff) {  // (selects: the loads above are unconditional)
#pragma unroll
            for (int b = 0; b < ND; ++b) {
              q += qa[i][b] * ea[i][b];
              t += ta[i][b] * ea[i][b];
            }
          }
        }
      } else {
        for (int i = 0; i < nnf; ++i) {
          const int e = cp[k * maxfn + i];
          if (e != 0xff) {
#pragma unroll
            for (int b = 0; b < ND; ++b) {
              const double ev = EV[ND * e + b];
              q += QV[ND * e + b] * ev;
              t += TV[ND * e + b] * ev;
            }
          }
        }
      }
      P.vq[p0 + k] = q;
      P.vt[p0 + k] = t;
    }
  }
  if (P.vqv) {
    for (int x = lane; x < len * ND; x += 64) {
      const int k = x / ND, b = x - k * ND;
      double qv = 0.0, tv = 0.0;
      if constexpr (NNF > 0) {
        int e[NNF];
#pragma unroll
        for (int i = 0; i < NNF; ++i) e[i] = cp[k * NNF + i];
        double qa[NNF], ta[NNF];
#pragma unroll
        for (int i = 0; i < NNF; ++i) {
          const int ee = e[i] == 0xff ? 0 : e[i];
          qa[i] = QV[ND * ee + b];
          ta[i] = TV[ND * ee + b];
        }
#pragma unroll
        for (int i = 0; i < NNF; ++i) {
          qv += (e[i] != 0xff) ? qa[i] : 0.0;
          tv += (e[i] != 0xff) ? ta[i] : 0.0;
        }
      } else {
        for (int i = 0; i < nnf; ++i) {
          const int e = cp[k * maxfn + i];
          if (e != 0xff) {
            qv += QV[ND * e + b];
            tv += TV[ND * e + b];
          }
        }
      }
      P.vqv[(int64_t)p0 * ND + x] = qv;
      P.vtv[(int64_t)p0 * ND + x] = tv;
    }
  }
}

template <int ND>
__global__ void __launch_bounds__(64) k_face_pipe(const FacePipeArgs P) {
  extern __shared__ __attribute__((aligned(16))) char pfv_lds[];
  const int lane = (int)threadIdx.x;
  SfRec* recL = reinterpret_cast<SfRec*>(pfv_lds + P.SL.rec);
  double* recW = reinterpret_cast<double*>(recL);
  double* QV = reinterpret_cast<double*>(pfv_lds + P.SL.qv);
  double* TV = reinterpret_cast<double*>(pfv_lds + P.SL.tv);
  double* EV = reinterpret_cast<double*>(pfv_lds + P.SL.ev);
  int32_t* bidx = reinterpret_cast<int32_t*>(pfv_lds + P.SL.bidx);
  uint32_t* cpW = reinterpret_cast<uint32_t*>(pfv_lds + P.cpw_off);
  const uint8_t* cpB = reinterpret_cast<const uint8_t*>(cpW);
  const int maxfn = P.maxfn;
  const double* recG = reinterpret_cast<const double*>(P.rec);
  const uint32_t* cpG = reinterpret_cast<const uint32_t*>(P.colpairs);  // (allocated with 8 spare bytes)

  // the faces of this wavefront: one contiguous range of the processing order per XCD (block b runs on XCD b % 8)
  const int64_t chunk = (P.n + 7) >> 3;
  const int64_t xcd = blockIdx.x & 7, slot = blockIdx.x >> 3, per_xcd = gridDim.x >> 3;
  const int64_t base_item = xcd * chunk;
  const int64_t lim = (base_item + chunk < P.n ? base_item + chunk : P.n) - base_item;  // items of this XCD
  const int RUN = P.run;
  int32_t* const ctr = P.ctr ? P.ctr + 16 * xcd : nullptr;
  if (!ctr && slot * RUN >= lim) return;
  // (index clamped instead of a branch per field: one scalar 32-byte load per record)
  auto load_frec = [&](int64_t b) {
    FaceRec r = P.frec[base_item + (b < lim ? b : lim - 1)];
    if (b >= lim) r.f = -1;
    return r;
  };
  // successive positions of this wavefront: runs of RUN consecutive items; a run is slot + g * per_xcd (static) or the
  // next value of the XCD's counter, fetched one run ahead so that the atomic's latency is never waited for
  int64_t g = 0, cur = 0;
  int left = 0;
  int pend = 0;  // lane 0: number of the run after the current one (dynamic)
  if (ctr && lane == 0) pend = atomicAdd(ctr, 1);
  auto next_pos = [&]() -> int64_t {
    if (left == 0) {
      int64_t run_no;
      if (ctr) {
        run_no = __builtin_amdgcn_readfirstlane(pend);
        if (lane == 0) pend = atomicAdd(ctr, 1);
      } else {
        run_no = slot + g * per_xcd;
        ++g;
      }
      cur = run_no * RUN;
      left = RUN;
    }
    --left;
    return cur++;
  };
  FaceRec F0 = load_frec(next_pos());
  FaceRec F1 = load_frec(next_pos());
  double R0 = 0.0;
  uint32_t C0a = 0u, C0b = 0u;
  if (F0.f >= 0) {
    if (lane < (int)F0.nnf * 8) R0 = recG[(int64_t)F0.a * 8 + lane];
    const int64_t b0 = P.cp_stride ? (int64_t)F0.f * P.cp_stride : (int64_t)F0.p0 * maxfn;
    const int nw = (int)(((b0 & 3) + (int64_t)(F0.lens & 0xffffu) * maxfn + 3) >> 2);
    if (lane < nw) C0a = cpG[(b0 >> 2) + lane];
    if (lane + 64 < nw) C0b = cpG[(b0 >> 2) + lane + 64];
  }
  while (F0.f >= 0) {
    // ---- current face: park what was prefetched for it in LDS (this consumes registers loaded one
    // face ago, before anything newer is issued)
    const int nnf = (int)F0.nnf;
    const int len = (int)(F0.lens & 0xffffu);
    const int blen = (int)(F0.lens >> 16);
    const int p0 = F0.p0;
    const int q0 = F0.q0;
    const int a = F0.a;
    const double inn = 1.0 / nnf;
    if (lane < nnf * 8) recW[lane] = R0;
    cpW[lane] = C0a;
    cpW[lane + 64] = C0b;
    // ---- prefetch: face record two ahead (scalar loads), sub-face records and column map one ahead
    const FaceRec F2 = load_frec(next_pos());
    double R1 = 0.0;
    uint32_t C1a = 0u, C1b = 0u;
    if (F1.f >= 0) {
      if (lane < (int)F1.nnf * 8) R1 = recG[(int64_t)F1.a * 8 + lane];
      const int64_t b1 = P.cp_stride ? (int64_t)F1.f * P.cp_stride : (int64_t)F1.p0 * maxfn;
      const int nw1 = (int)(((b1 & 3) + (int64_t)(F1.lens & 0xffffu) * maxfn + 3) >> 2);
      if (lane < nw1) C1a = cpG[(b1 >> 2) + lane];
      if (lane + 64 < nw1) C1b = cpG[(b1 >> 2) + lane + 64];
    }
    for (int i = lane; i < blen; i += 64) bidx[i] = P.bix[q0 + i];
    wave_sync_lds();
    int offs[kMaxFaceNodes + 1], offs2[kMaxFaceNodes + 1];
    int m2 = 0;
    {
      int m = 0;
#pragma unroll
      for (int i = 0; i < kMaxFaceNodes; ++i) {
        offs[i] = m;
        offs2[i] = m2;
        if (i < nnf) {
          const int deg = recL[i].deg;
          m += deg;
          m2 += (ND * deg + 1) >> 1;
        }
      }
      offs[kMaxFaceNodes] = m;
      offs2[kMaxFaceNodes] = m2;
    }
    for (int t = lane; t < m2; t += 64) {
      int i = 0;
#pragma unroll
      for (int ii = 1; ii < kMaxFaceNodes; ++ii) i += (ii < nnf && t >= offs2[ii]) ? 1 : 0;
      int o2 = 0, o1 = 0;
#pragma unroll
      for (int ii = 0; ii < kMaxFaceNodes; ++ii) {
        o2 = (ii == i) ? offs2[ii] : o2;
        o1 = (ii == i) ? offs[ii] : o1;
      }
      const int x0 = 2 * (t - o2);
      const SfRec& R = recL[i];
      const int nh = ND * (int)R.deg, ldt = (nh + 1) & ~1;
      const double* base = P.tab + R.toff;
      D2 rv[ND];
#pragma unroll
      for (int k = 0; k < ND; ++k) rv[k] = *reinterpret_cast<const D2*>(base + (int)R.r[k] * ldt + x0);
      const D2 ee = *reinterpret_cast<const D2*>(base + (int)R.n * ldt + x0);
      const int ls = R.ls, js = R.jstar;
      int ksel = 0;
#pragma unroll
      for (int k = 1; k < ND; ++k) ksel = ((int)R.r[k] == ls) ? k : ksel;
      double tvx = rv[0].x, tvy = rv[0].y;
#pragma unroll
      for (int k = 1; k < ND; ++k) {
        tvx = (ksel == k) ? rv[k].x : tvx;
        tvy = (ksel == k) ? rv[k].y : tvy;
      }
      double sx = 0.0, sy = 0.0;
#pragma unroll
      for (int k = 0; k < ND; ++k) {
        sx += R.om[k] * rv[k].x;
        sy += R.om[k] * rv[k].y;
      }
      const int flat = ND * o1 + x0;
      {
        const int j = x0 / ND, b = x0 - ND * j;
        QV[flat] = ((j == js) ? R.nk[b] : 0.0) - sx;
        TV[flat] = tvx * inn;
        EV[flat] = ee.x;
      }
      if (x0 + 1 < nh) {
        const int j = (x0 + 1) / ND, b = x0 + 1 - ND * j;
        QV[flat + 1] = ((j == js) ? R.nk[b] : 0.0) - sy;
        TV[flat + 1] = tvy * inn;
        EV[flat + 1] = ee.y;
      }
    }
    wave_sync_lds();
    const int cpo = (int)((P.cp_stride ? (int64_t)F0.f * P.cp_stride : (int64_t)p0 * maxfn) & 3);
    if (nnf == 3 && maxfn == 3) face_pipe_columns<ND, 3>(P, cpB + cpo, QV, TV, EV, lane, len, p0);
    else if (nnf == 4 && maxfn == 4) face_pipe_columns<ND, 4>(P, cpB + cpo, QV, TV, EV, lane, len, p0);
    else face_pipe_columns<ND, 0>(P, cpB + cpo, QV, TV, EV, lane, len, p0, nnf, maxfn);
    if (P.vqb && blen > 0) {
      for (int pos = lane; pos < blen; pos += 64) {
        const int fb = bidx[pos];
        double q = 0.0, t = 0.0;
        for (int i = 0; i < nnf; ++i) {
          const int v = P.fn_idx[a + i];
          const int b0 = P.bp[v], nb = P.bp[v + 1] - b0;
          const int k = lower_bound_idx<int32_t>(P.bfc + b0, nb, fb);
          if (k < nb && P.bfc[b0 + k] == fb) {
            const int64_t tb0 = P.tbptr[v] + (int64_t)recL[i].ls * nb + k;
            q += P.tabb[tb0];
            t += P.tabb[tb0 + (int64_t)recL[i].n * nb];
          }
        }
        P.vqb[q0 + pos] = q;
        P.vtb[q0 + pos] = t * inn;
      }
    }
    wave_sync_lds();  // the LDS arrays are rewritten for the next face
    F0 = F1;
    F1 = F2;
    R0 = R1;
    C0a = C1a;
    C0b = C1b;
  }
}

static bool launch_face_pipe(pfv_ctx_impl& c, const FaceArgs& A, const FaceLds& SL, int64_t nitems) {
  // limits of the register-parked prefetches: 8 nodes per face, 512 bytes of column map per row
  if (c.nd != 3 || nitems < 4096 || A.maxfn > kMaxFaceNodes || (int64_t)A.maxrow * A.maxfn + 3 > 512) return false;
  FacePipeArgs P;
  P.frec = c.face_rec.p; P.rec = A.rec; P.colpairs = A.colpairs; P.tab = A.tab; P.tabb = A.tabb; P.tbptr = A.tbptr;
  P.fn_idx = A.fn_idx; P.bix = A.bix; P.bp = A.bp; P.bfc = A.bfc;
  P.vq = A.vq; P.vt = A.vt; P.vqb = A.vqb; P.vtb = A.vtb; P.vqv = A.vqv; P.vtv = A.vtv;
  P.n = nitems; P.maxfn = A.maxfn; P.SL = SL; P.cp_stride = A.cp_stride;
  P.cpw_off = SL.total;
  P.run = std::max(1, env_int("PFV_FACE_RUN", 4));
  P.ctr = nullptr;
  if (env_int("PFV_FACE_DYN", 1) != 0) {
    // (one set of 8 counters per launch in flight: face kernels may follow each other on the stream, but a counter set
    // is zeroed by a memset ENQUEUED before its launch -- 32 sets, cycled)
    int32_t* base = c.face_ctr.ensure(32 * 8 * 16);
    P.ctr = base + (size_t)(c.face_ctr_next++ % 32) * 8 * 16;
    be_memset(P.ctr, 0, sizeof(int32_t) * 8 * 16, c.stream);
  }
  const size_t lds = SL.total + 512;
  if (lds > 64 * 1024) return false;
  // persistent: exactly the wavefronts that are resident at once, so that the 8 ranges are swept once
  // (a second generation of workgroups would walk the tables a second time, long after L2 dropped them)
  static int num_cu = 0;
  if (!num_cu) PFV_HIP_CHECK(hipDeviceGetAttribute(&num_cu, hipDeviceAttributeMultiprocessorCount, c.device));
  int occ = 0;
  PFV_HIP_CHECK(hipOccupancyMaxActiveBlocksPerMultiprocessor(&occ, k_face_pipe<3>, 64, lds));
  if (occ < 1) return false;
  int64_t blocks = (int64_t)num_cu * occ;
  blocks = std::min<int64_t>(blocks, env_int("PFV_FACE_PIPE_BLOCKS", 1 << 30));
  blocks = std::max<int64_t>((blocks + 7) & ~int64_t(7), 8);
  PFV_LAUNCH(HIP_KERNEL_NAME(k_face_pipe<3>), dim3((unsigned)blocks), dim3(64), lds, c.stream, P);
  PFV_HIP_CHECK(hipGetLastError());
  return true;
}
#endif

// subset != nullptr: only the n_subset listed faces (partial discretization)
static void run_face_kernel(pfv_ctx_impl& c, bool with_vs, const int32_t* subset = nullptr, int64_t n_subset = 0) {
  stream_t s = c.stream;
  const int nd = c.nd;
  FaceArgs A;
  // conditions per sub-face: matrices 0-3 keep sub-face rows (run_subface_kernel); only the
  // vector-source matrices are collapsed to faces here
  A.vq = c.subface_bc ? nullptr : c.val[PFV_MAT_FLUX].ensure(c.pat_flux.nnz);
  A.vt = c.subface_bc ? nullptr : c.val[PFV_MAT_BOUND_PRESSURE_CELL].ensure(c.pat_flux.nnz);
  A.vqb = c.subface_bc ? nullptr : c.val[PFV_MAT_BOUND_FLUX].ensure(c.pat_bound.nnz);
  A.vtb = c.subface_bc ? nullptr : c.val[PFV_MAT_BOUND_PRESSURE_FACE].ensure(c.pat_bound.nnz);
  A.vqv = with_vs ? c.val[PFV_MAT_VECTOR_SOURCE].ensure(c.pat_vs.nnz) : nullptr;
  A.vtv = with_vs ? c.val[PFV_MAT_BOUND_PRESSURE_VECTOR_SOURCE].ensure(c.pat_vs.nnz) : nullptr;
  A.fn_ptr = c.fn_ptr; A.fn_idx = c.fn_idx;
  A.ip = c.pat_flux.indptr;
  A.bip = c.pat_bound.indptr; A.bix = c.pat_bound.indices;
  A.order = subset ? subset : c.face_order.p;
  A.bp = c.node_bptr; A.bfc = c.node_bfaces;
  A.colpairs = c.flux_colpairs;
  A.cp_stride = c.cp_stride;
  A.rec = c.sf_rec; A.tbptr = c.node_tbptr; A.tab = c.tab; A.tabb = c.tabb;
  A.maxrow = std::max(c.pat_flux.max_row, 1);
  A.maxbrow = std::max(c.pat_bound.max_row, 1);
  A.maxfn = std::max(c.max_face_nodes, 1);
  A.maxpairs = A.maxfn * std::max(c.max_deg, 1);
  const FaceLds SL = face_lds_layout(A.maxfn, A.maxpairs, A.maxbrow, nd);
  const int64_t nitems = subset ? n_subset : c.nf;
  if (nitems <= 0) return;
  // faces run along the Morton curve (face_order): one contiguous range of it per XCD keeps the tables of
  // the nodes a range shares in that XCD's L2
  const bool xcd = !subset && env_int("PFV_FACE_XCD", 1) != 0;
  bool launched = false;
#ifndef PFV_EMULATE
  // all faces of a 3-D grid: the software-pipelined persistent kernel (k_face_pipe)
  launched = !subset && env_int("PFV_FACE_PIPE", 1) != 0 && launch_face_pipe(c, A, SL, nitems);
#endif
  if (launched) {
  } else if (nd == 2) {
    wave_for<64>(s, nitems, SL.total, PFV_LAMBDA(const WaveCtx& w) { face_body<2>(A, SL, w); });
  } else if (xcd) {
    wave_for_xcd(s, nitems, SL.total, PFV_LAMBDA(const WaveCtx& w) { face_body<3>(A, SL, w); });
  } else {
    wave_for<64>(s, nitems, SL.total, PFV_LAMBDA(const WaveCtx& w) { face_body<3>(A, SL, w); });
  }
  c.filled[PFV_MAT_FLUX] = c.filled[PFV_MAT_BOUND_PRESSURE_CELL] = true;
  c.filled[PFV_MAT_BOUND_FLUX] = c.filled[PFV_MAT_BOUND_PRESSURE_FACE] = true;
  c.filled[PFV_MAT_VECTOR_SOURCE] = c.filled[PFV_MAT_BOUND_PRESSURE_VECTOR_SOURCE] = with_vs;
}

// ---- boundary conditions per sub-face (mpfa.py:761-768, 1117-1125): flux / bound_flux / the two trace
// matrices keep one row per sub-face s = (face, node) -- the node's rows applied to the node's
// coefficient tables, no sum over the nodes of the face.
//   row s of flux / bound_pressure_cell:        columns = cells of the node
//   row s of bound_flux / bound_pressure_face:  columns = boundary sub-faces of the node
static void build_subface_symbolic(pfv_ctx_impl& c) {
  stream_t s = c.stream;
  const int nd = c.nd;
  const int64_t nsf = c.nsf;
  const int32_t* fn_idx = c.fn_idx;  // node of every sub-face
  const int32_t* hp = c.node_hptr;
  const int32_t* fp = c.node_fptr;
  const int32_t* bp = c.node_bptr;
  const int32_t* ncl = c.node_cells;
  const int32_t* nsfid = c.node_sf;
  const uint8_t* bls = c.node_bls;
  Buf<int32_t> l1, l2;
  Buf<int64_t> p1, p2;
  int32_t* a1 = l1.ensure(nsf + 1);
  int32_t* a2 = l2.ensure(nsf + 1);
  p1.ensure(nsf + 1);
  p2.ensure(nsf + 1);
  parallel_for(s, nsf, PFV_LAMBDA(int64_t sf) {
    const int v = fn_idx[sf];
    a1[sf] = (hp[v + 1] - hp[v]) / nd;
    a2[sf] = bp[v + 1] - bp[v];
  });
  exclusive_scan<int32_t, int64_t>(s, c.scratch, a1, p1.p, (size_t)nsf);
  exclusive_scan<int32_t, int64_t>(s, c.scratch, a2, p2.p, (size_t)nsf);
  finish_pattern(c, c.pat_sflux, p1, nsf, c.nc);
  finish_pattern(c, c.pat_sbound, p2, nsf, nsf);
  c.pat_sflux.max_row = std::max(c.max_deg, 1);
  c.pat_sbound.max_row = std::max(c.max_bnd_per_node, 1);
  const int32_t* ip = c.pat_sflux.indptr;
  int32_t* ix = c.pat_sflux.indices;
  const int32_t* bip = c.pat_sbound.indptr;
  int32_t* bix = c.pat_sbound.indices;
  parallel_for(s, nsf, PFV_LAMBDA(int64_t sf) {
    const int v = fn_idx[sf];
    const int deg = (hp[v + 1] - hp[v]) / nd;
    for (int j = 0; j < deg; ++j) ix[ip[sf] + j] = ncl[hp[v] / nd + j];
    const int nb = bp[v + 1] - bp[v];
    for (int i = 0; i < nb; ++i) bix[bip[sf] + i] = nsfid[fp[v] + bls[bp[v] + i]];  // ascending with the face id
  });
  c.have_sub_symbolic = true;
}

static void run_subface_kernel(pfv_ctx_impl& c) {
  stream_t s = c.stream;
  const int nd = c.nd;
  double* vq = c.val[PFV_MAT_FLUX].ensure(std::max<int64_t>(c.pat_sflux.nnz, 1));
  double* vt = c.val[PFV_MAT_BOUND_PRESSURE_CELL].ensure(std::max<int64_t>(c.pat_sflux.nnz, 1));
  double* vqb = c.val[PFV_MAT_BOUND_FLUX].ensure(std::max<int64_t>(c.pat_sbound.nnz, 1));
  double* vtb = c.val[PFV_MAT_BOUND_PRESSURE_FACE].ensure(std::max<int64_t>(c.pat_sbound.nnz, 1));
  const int32_t* fn_idx = c.fn_idx;
  const int32_t* bp = c.node_bptr;
  const SfRec* rec = c.sf_rec;
  const int64_t* tbptr = c.node_tbptr;
  const double* tab = c.tab;
  const double* tabb = c.tabb;
  const int32_t* ip = c.pat_sflux.indptr;
  const int32_t* bip = c.pat_sbound.indptr;
  wave_for<16>(s, c.nsf, 16, PFV_LAMBDA(const WaveCtx& w) {
    const int64_t sf = w.item;
    const SfRec R = rec[sf];
    const int v = fn_idx[sf];
    const int nh = nd * (int)R.deg, ldt = (nh + 1) & ~1;
    const double* base = tab + R.toff;
    PFV_LANES(j, (int)R.deg) {
      double q = 0.0, t = 0.0;
      for (int b = 0; b < nd; ++b) {
        const int x = nd * j + b;
        double sacc = 0.0;
        for (int k = 0; k < nd; ++k) sacc += R.om[k] * base[(int)R.r[k] * ldt + x];
        const double qv = ((j == (int)R.jstar) ? R.nk[b] : 0.0) - sacc;
        const double e = base[(int)R.n * ldt + x];
        q += qv * e;
        t += base[(int)R.ls * ldt + x] * e;
      }
      vq[ip[sf] + j] = q;
      vt[ip[sf] + j] = t;
    }
    const int nb = bp[v + 1] - bp[v];
    const int64_t tb0 = tbptr[v] + (int64_t)R.ls * nb;
    PFV_LANES(i, nb) {
      vqb[bip[sf] + i] = tabb[tb0 + i];
      vtb[bip[sf] + i] = tabb[tb0 + (int64_t)R.n * nb + i];
    }
  });
  c.filled[PFV_MAT_FLUX] = c.filled[PFV_MAT_BOUND_PRESSURE_CELL] = true;
  c.filled[PFV_MAT_BOUND_FLUX] = c.filled[PFV_MAT_BOUND_PRESSURE_FACE] = true;
}

}  // namespace pfv
