// mpsa.inc — MPSA-W stress discretization (numerics/fv/mpsa.py:531-782 of the reference) on the
// device, in the same condensed form as the MPFA kernels: per interaction region (node v) the
// unknowns are the continuity-point displacements Lambda_{s,a} (n = nd * #sub-faces instead of the
// reference's nd^2 * #sub-cells gradients; 108 instead of 216 on tetrahedra).
//
//   sub-cell j:  grad u_a = D_j^-1 (Lambda_{faces(j),a} - u_{j,a} 1)
//   Tsym_i(h) . G_j  = sum_{a,k} Omega_h[i][a][k] (Lambda_{lf(j,k),a} - u_{j,a})
//        Omega_h[i][a][k] = sum_l (n_h^T Csym_c[nd i : nd i + nd, nd a + l]) D^-1[l][k]
//   P[q] (node average of the asymmetric stress, mpsa.py:1599-1667)
//        = sum_j sum_{a,k} Pi_j[q][a][k] (Lambda_{lf(j,k),a} - u_{j,a}),
//        Pi_j[q][a][k] = w_j sum_l Casym_j[q, nd a + l] D_j^-1[l][k],  w_j = node-volume weight
//   rows: interior (s,i):  sum_h sgn_h Tsym_i(h).G = 0
//         Neumann  (s,i):  sgn_h (Tsym_i(h).G + e_i sum_k' n_h[k'] P[nd i + k']) = bc / #nodes(f)
//                          (e_i = 0 when the corner rule of mpsa.py:1932-2000 drops the term)
//         Dirichlet (s,a): Lambda_{s,a} = bc
//   outputs from the first side h* of each sub-face:
//         traction_i = Tsym_i(h*).G + e sum_k' n_h*[k'] P[nd i + k'],   trace = Lambda_{s,a}.
//
// The node kernel runs one 256-thread workgroup per node (the n x n system of a tetrahedral grid
// needs 94 KB of LDS, so only one node fits a CU anyway), inverts A with the portable LDS
// Gauss-Jordan, and writes for every sub-face row the already expanded coefficients over the
// node's cells (stress and trace) and boundary faces.  The face kernel then only adds the <= nodes(f)
// contributions of every CSR entry; the CSR patterns are nd x nd block expansions of the MPFA ones.

namespace pfv {

struct MpsaArgs {
  int nd;
  int64_t nc, nf, nn;
  double eta;
  const double* eta_sub;    // continuity points per sub-face (nullptr: the scalar eta, 0 on the boundary)
  double hf_eta;            // reconstruction_eta (with Et2 != nullptr)
  const double* hf_eta_sub; // ... per sub-face, used as given also on the boundary (nullptr: the scalar, 0 on the boundary)
  double *Et2, *Etb2;       // displacement traces reconstructed at the hf_eta points (nullptr: the continuity-point traces serve)
  const int32_t *order, *hp, *fp, *node_sf, *node_face, *sf_face, *fn_ptr, *nsides, *h_cell, *bp, *cell_nnodes;
  const uint8_t *h_lf, *h_first, *dirbits, *neubits, *bls;
  const uint8_t* robbits;   // Robin flags per component (nullptr: none)
  int sub_bc;               // conditions per sub-face: the flag / weight arrays are indexed by the global sub-face id
  int64_t nbc;              // columns of the condition arrays (Nf, or Nsf with sub_bc)
  const double* robw;       // [nd*nd][Nf] Robin weights W_ia(f) (nullptr: identity)
  const double* farea;
  const double* basis;      // [nd*nd][Nf] boundary basis B_kc(f) (nullptr: Cartesian)
  const int8_t* h_sgn;
  const double *fnorm, *fcen, *ccen, *nodes, *stiff, *cvol;
  const int64_t *eptr, *ebptr;
  double *Es, *Et, *Esb, *Etb;
  int32_t* st;
  // Biot coupling terms (numerics/fv/biot.py:714-878), one set per coupling tensor alpha_kappa
  int nalpha;                 // 0: pure mechanics
  const double* alpha;        // [nalpha][9][Nc]  (SecondOrderTensor.values layout)
  const int64_t *dptr, *dbptr, *cptr;  // per-node offsets of the divergence rows (cells / boundary / pressure)
  int64_t tot_p, tot_d, tot_db, tot_c;  // per-key strides of the arrays below
  double *Esp, *Etp, *DD, *BDD, *CONS;
  int ablate;  // profiling only (PFV_MPSA_ABLATE = k): leave the kernel after stage k
  int lds_gj;  // A/B switch (PFV_MPSA_LDS_GJ): LDS-resident Gauss-Jordan on the device too
  const uint8_t* active;  // partial discretization: only nodes with active[v] != 0 (nullptr = all)
  int refine;             // iterative refinement of the inverse: 0 where kappa asks for it, -1 never, k > 0 always k steps
  int32_t* redo;          // lean launches: nodes left to the full body (count in st[2])
  int nopivot;            // lean launches: elimination without the pivot search, verified afterwards (mpsa_gj_reg_np)
  const uint8_t* wide;    // != nullptr: regions with wide[v] != 0 are left to the double-double body (mpsa_contrast_scan)
  const uint8_t* wide_exp;  // wide body: binary exponent of the region's stiffness contrast (0: none) -> pivot threshold
  double np_tol;          // ... acceptance: scaled residual <= np_tol * kappa
};

// T: the arithmetic of the body -- double, or dd (dd.h) for the regions of high stiffness contrast
template <class T>
struct MpsaLdsT {
  T *A, *scale, *rowk, *colk, *Om, *Pi, *PL, *PU, *AG, *PLA, *PLAG, *Ptot, *Pb, *nvec, *wj, *beta;
  T *Dinv, *Lp, *Pp;  // D_j^-1 per sub-cell; Biot: Lambda response to cell pressures, P response
  T* basisL;          // [nsf][nd][nd] basis of every sub-face (identity off the boundary)
  T* gjx;             // register Gauss-Jordan exchange: pivot column [128] | pivot row [128] | key [8] | pivot step of every row [128 x int32]
  T *EtW, *EtbW;      // T != double only: the trace responses in working precision (a.Et / a.Etb take their FP64 roundings)
  double* keyd;       // T != double only: |pivot candidates| of a column in FP64 (pivot search)
  int32_t *ipiv, *fid, *sideh, *firsth;
  uint8_t *type, *lfL;
  int8_t* sgL;
};
using MpsaLds = MpsaLdsT<double>;

// Elements set aside for L.A.  The unpivoted elimination (mpsa_gj_reg_np) keeps its two exchange buffers of 256 doubles in
// L.A while the matrix sits in registers: a system of n <= 22 unknowns (n * ld < 512: every node of a 2-D grid, the
// boundary nodes of a 3-D one with at most 7 faces) is smaller than they are.  Sized by n * ld alone the buffers ran over
// L.scale, L.rowk, L.colk and L.Om, the a-posteriori check read what they left there, never passed, and every such region
// was computed a second time by the full body (right results, twice the work: all 2 116 regions of a 45 x 45 triangle
// grid on the redo list).
constexpr size_t kMpsaExchangeElems = 512;
PFV_HD inline size_t mpsa_a_elems(size_t n, size_t ld) { return n * ld > kMpsaExchangeElems ? n * ld : kMpsaExchangeElems; }

PFV_HD inline size_t mpsa_lds_bytes(int nsfmax, int degmax, int nbmax, int nd, bool biot = false, size_t tsize = 8) {
  const size_t n = (size_t)nd * nsfmax, ld = n | 1, n2 = (size_t)nd * nd, nh = (size_t)degmax * nd;
  const size_t ncu = (size_t)nd * degmax, ncb = (size_t)nd * nbmax;
  // Pi is dead once PL / PU exist; AG and PLA (built after the inversion) reuse its space
  const size_t pi_sz = (size_t)degmax * n2 * n2, ag_sz = 2 * n * n2;
  const size_t pi_or_ag = pi_sz > ag_sz ? pi_sz : ag_sz;
  // one region for everything that is dead once the stress / trace rows are out: Pi|AG|PLA, PU, PLAG,
  // Ptot, Pb; the Biot tail keeps Lp | Pp there
  size_t u = pi_or_ag + n2 * ncu /*PU*/ + n2 * n2 /*PLAG*/ + n2 * ncu /*Ptot*/ + n2 * (ncb + 1) /*Pb*/;
  const size_t ub = n * (size_t)degmax /*Lp*/ + n2 * (size_t)degmax /*Pp*/;
  if (biot && ub > u) u = ub;
  size_t d = mpsa_a_elems(n, ld) + 3 * n + nh * nd * n2 /*Om: nh*nd^3*/ + u + n2 * n /*PL*/ + nh * nd /*nvec*/ +
             degmax /*wj*/ + n /*beta*/ + (size_t)degmax * n2 /*Dinv*/ + 328 /*gjx*/ + (size_t)nsfmax * n2 /*basisL*/;
  size_t i = n + 4 + (size_t)nsfmax * 4;
  size_t b = n + 2 * nh;
  if (tsize != 8) {  // working copies of Et / Etb, FP64 pivot keys
    d += n * (ncu + ncb);
    i += 2 * n + 2;
  }
  return d * tsize + i * 4 + b + 128 + 64;
}

template <class T>
PFV_FN void mpsa_carve(char* lds, int nsf, int deg, int nb, int nd, MpsaLdsT<T>& L, bool biot) {
  const size_t n = (size_t)nd * nsf, ld = n | 1, n2 = (size_t)nd * nd, nh = (size_t)deg * nd;
  const size_t ncu = (size_t)nd * deg, ncb = (size_t)nd * nb;
  Carver cv(lds);
  L.A = cv.take<T>(mpsa_a_elems(n, ld));  // (at least the exchange buffers of mpsa_gj_reg_np)
  L.scale = cv.take<T>(n);
  L.rowk = cv.take<T>(n);
  L.colk = cv.take<T>(n);
  L.Om = cv.take<T>(nh * nd * n2);   // [h][i][a][k]
  {
    const size_t pi_sz = (size_t)deg * n2 * n2, ag_sz = 2 * n * n2;
    const size_t pi_or_ag = pi_sz > ag_sz ? pi_sz : ag_sz;
    size_t u = pi_or_ag + n2 * ncu + n2 * n2 + n2 * ncu + n2 * (ncb + 1);
    const size_t ub = n * (size_t)deg + n2 * (size_t)deg;
    if (biot && ub > u) u = ub;
    T* U = cv.take<T>(u);
    L.Pi = U;  // [j][q][a][k]; later AG | PLA
    L.AG = L.Pi;
    L.PLA = L.Pi + n * n2;
    L.PU = U + pi_or_ag;
    L.PLAG = L.PU + n2 * ncu;
    L.Ptot = L.PLAG + n2 * n2;
    L.Pb = L.Ptot + n2 * ncu;
    L.Lp = biot ? U : nullptr;  // Biot tail: everything above is dead by then
    L.Pp = biot ? U + n * (size_t)deg : nullptr;
  }
  L.PL = cv.take<T>(n2 * n);
  L.nvec = cv.take<T>(nh * nd);
  L.wj = cv.take<T>(deg);
  L.beta = cv.take<T>(n);
  L.Dinv = cv.take<T>((size_t)deg * n2);
  L.gjx = cv.take<T>(328);
  L.basisL = cv.take<T>((size_t)nsf * n2);
  L.EtW = L.EtbW = nullptr;
  L.keyd = nullptr;
  if constexpr (!std::is_same<T, double>::value) {
    L.EtW = cv.take<T>(n * ncu);
    L.EtbW = cv.take<T>(n * ncb + 1);
    L.keyd = cv.take<double>(n + 1);
  }
  L.ipiv = cv.take<int32_t>(n + 4);
  L.fid = cv.take<int32_t>(nsf);
  L.sideh = cv.take<int32_t>((size_t)nsf * 2);
  L.firsth = cv.take<int32_t>(nsf);
  L.type = cv.take<uint8_t>(n);   // per (s, component): 0 interior, 1 Dirichlet, 2 Neumann, 3 Robin
  L.lfL = cv.take<uint8_t>(nh);
  L.sgL = cv.take<int8_t>(nh);
}

#ifndef PFV_EMULATE
// Register-resident Gauss-Jordan for the 256-thread MPSA workgroup, n <= 128.  The matrix is dealt
// out block-cyclically: thread t = 16 J + I holds the 8 x 8 entries (I + 16 i', J + 16 j'), static
// register indices only.  Per pivot step a thread then needs 8 multipliers and 8 pivot-row entries
// for its 64 FMAs -- 16 LDS reads instead of the 64 of a row-per-thread layout, whose broadcast of
// the pivot row (256 threads x 64 doubles = 128 KB per step through a 128 B/clk LDS) was the bound
// of the first versions (5 300, with rotating slots 3 900 cycles per step; one wavefront per SIMD
// hides nothing).
// Step k = 16 j' + kk (j' unrolled, so the local column index is static): the 16 threads with J = kk
// publish their 8 entries of column k and the DPP maximum of their (32-bit) keys -> pivot row p (implicit
// pivoting: rows never move); the 16 threads with I = p mod 16 publish their 8 entries of row p
// (local row p / 16 is workgroup-uniform: a scalar branch picks the registers); everybody updates
//   a[i'][j'] -= g[i'] * prow[j'],   g = a[r][k] / piv  (other rows),  g = 1 - 1/piv  (the pivot row),
//   prow[k] := piv + 1,
// which leaves -g resp. 1/piv in column k and the pivot row normalised -- the in-place inversion
// step.  Two workgroup barriers per step.
__device__ __forceinline__ void mpsa_gj_reg(const WaveCtx& w, const MpsaLds& L, int n, int ld, int v, int32_t* st) {
  const int t = (int)threadIdx.x;
  const int I = t & 15, J = t >> 4;
  const bool act = t < 256;  // wavefronts beyond the fourth (512-thread workgroups) only keep the barriers company
  double* gcolT = L.gjx;                // [8 i'][16 I]: column k (natural row order: conflict-free across I)
  double* prowT = L.gjx + 128;          // [8 j'][16 J]: row p
  unsigned* keys = reinterpret_cast<unsigned*>(L.gjx + 256);  // [1] (+ spare)
  int32_t* rowstep = reinterpret_cast<int32_t*>(L.gjx + 264);                     // [128] step at which a row was pivot
  double a[8][8];
#pragma unroll
  for (int i = 0; i < 8; ++i)
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const int r = I + 16 * i, col = J + 16 * j;
      a[i][j] = (act && r < n && col < n) ? L.A[r * ld + col] : 0.0;
    }
  unsigned used = 0;  // bit i': row I + 16 i' has been a pivot row (or lies beyond n)
#pragma unroll
  for (int i = 0; i < 8; ++i)
    if (I + 16 * i >= n) used |= 1u << i;
  bool bad = false;
  w.sync();  // all entries are in registers: L.A is free for the result
#pragma unroll
  for (int jp = 0; jp < 8; ++jp) {
    for (int kk = 0; kk < 16; ++kk) {
      const int k = 16 * jp + kk;
      if (k >= n) break;
      if (act && J == kk) {
        // keys: single-precision image of |a| (which of two nearly equal candidates wins is immaterial
        // for partial pivoting; v_max_u32 takes its DPP operand directly) | 127 - row
        unsigned key = 0u;
#pragma unroll
        for (int i = 0; i < 8; ++i) {
          const double x = a[i][jp];
          gcolT[16 * i + I] = x;
          const float mag = fabsf((float)x);
          unsigned cand = 0u;
          if (!((used >> i) & 1u) && mag > (float)kPivotTiny && mag < 1.0e38f)
            cand = (__float_as_uint(mag) & ~127u) | (unsigned)(127 - (I + 16 * i));
          key = umax32(key, cand);
        }
        key = group_max_u32<16>(key, 0);
        if (I == 0) keys[0] = key;
      }
      w.sync();
      double g[8];
      if (act) {
      const unsigned key = keys[0];
      if (key == 0u) bad = true;
      const int p = __builtin_amdgcn_readfirstlane(key ? 127 - (int)(key & 127u) : 0);
      const int pi = p & 15, pq = p >> 4;
      const double piv = gcolT[16 * pq + pi];
      // 1 / piv: hardware estimate + two Newton steps (the rows are scaled, no range handling needed;
      // the IEEE division sequence is 3x as long and sits on the critical path of every step)
      double pivinv = __builtin_amdgcn_rcp(piv);
      pivinv = fma(fma(-piv, pivinv, 1.0), pivinv, pivinv);
      pivinv = fma(fma(-piv, pivinv, 1.0), pivinv, pivinv);
#pragma unroll
      for (int i = 0; i < 8; ++i) g[i] = gcolT[16 * i + I] * pivinv;
      if (I == pi) {
#pragma unroll
        for (int i = 0; i < 8; ++i) {
          if (pq == i) {  // workgroup-uniform
            g[i] = 1.0 - pivinv;
            used |= 1u << i;
#pragma unroll
            for (int j = 0; j < 8; ++j) prowT[16 * j + J] = (j == jp && J == kk) ? a[i][j] + 1.0 : a[i][j];
          }
        }
        if (J == 0) {
          L.ipiv[k] = p;
          rowstep[p] = k;
        }
      }
      }
      w.sync();
      if (act) {
        double pr[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) pr[j] = prowT[16 * j + J];
#pragma unroll
        for (int i = 0; i < 8; ++i)
#pragma unroll
          for (int j = 0; j < 8; ++j) a[i][j] = fma(-g[i], pr[j], a[i][j]);
      }
    }
  }
  if (bad && t == 0) atomicMax(st + 0, v + 1);
  w.sync();  // ipiv, rowstep complete
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    const int r = I + 16 * i;
    if (act && r < n) {
      const int ms = rowstep[r];
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const int col = J + 16 * j;
        if (col < n) L.A[ms * ld + L.ipiv[col]] = a[i][j];
      }
    }
  }
  w.sync();
}
#endif

constexpr int kMpsaNoPivotDefault = 1;  // PFV_MPSA_GJ_NP (measured at configs[3]: node kernel 64.4 -> 52.3 ms, 6 of 91 125 regions to the redo list)
#ifndef PFV_EMULATE
// The same elimination WITHOUT the pivot search (lean launches, PFV_MPSA_GJ_NP): the pivot of step k is the diagonal
// entry, so the owners of column k (J == k % 16) and of row k (I == k % 16, register row k / 16) are known before the
// step and both publish at once -- ONE workgroup barrier per step instead of two, no keys, no DPP reduction, no scalar
// branch on the pivot's register row.  The exchange arrays are double-buffered (step k + 1 is published while slower
// wavefronts still read step k) and live in L.A, which is free while the matrix sits in registers.  Nothing guarantees
// that the condensed system tolerates the diagonal as pivots: the caller verifies the inverse a posteriori (one
// product with a fixed vector against the defining coefficients) and hands a region that fails to the pivoted body
// through the redo list of the lean launches.  Returns false when a pivot was zero / tiny / non-finite.
__device__ __forceinline__ bool mpsa_gj_reg_np(const WaveCtx& w, const MpsaLds& L, int n, int ld) {
  const int t = (int)threadIdx.x;
  const int I = t & 15, J = t >> 4;
  const bool act = t < 256;
  double a[8][8];
#pragma unroll
  for (int i = 0; i < 8; ++i)
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const int r = I + 16 * i, col = J + 16 * j;
      a[i][j] = (act && r < n && col < n) ? L.A[r * ld + col] : 0.0;
    }
  w.sync();  // all entries are in registers: L.A is free (exchange buffers now, the result at the end)
  double* xbuf = L.A;  // [2][gcolT 128 | prowT 128]
  bool degenerate = false;
  int buf = 0;
  if (act && J == 0) {
#pragma unroll
    for (int i = 0; i < 8; ++i) xbuf[16 * i + I] = a[i][0];
  }
  if (act && I == 0) {
#pragma unroll
    for (int j = 0; j < 8; ++j) xbuf[128 + 16 * j + J] = (j == 0 && J == 0) ? a[0][j] + 1.0 : a[0][j];
  }
  w.sync();
#pragma unroll
  for (int jp = 0; jp < 8; ++jp) {
    for (int kk = 0; kk < 16; ++kk) {
      const int k = 16 * jp + kk;
      if (k >= n) break;
      const double* gcolT = xbuf + 256 * buf;
      const double* prowT = gcolT + 128;
      double* gn = xbuf + 256 * (buf ^ 1);
      if (act) {
        const double piv = gcolT[16 * jp + kk];
        const double mag = fabs(piv);
        if (!(mag > kPivotTiny && mag < 1.0e300)) degenerate = true;
        double pivinv = __builtin_amdgcn_rcp(piv);
        pivinv = fma(fma(-piv, pivinv, 1.0), pivinv, pivinv);
        pivinv = fma(fma(-piv, pivinv, 1.0), pivinv, pivinv);
        double g[8], pr[8];
#pragma unroll
        for (int i = 0; i < 8; ++i) g[i] = gcolT[16 * i + I] * pivinv;
        g[jp] = (I == kk) ? 1.0 - pivinv : g[jp];
#pragma unroll
        for (int j = 0; j < 8; ++j) pr[j] = prowT[16 * j + J];
#pragma unroll
        for (int i = 0; i < 8; ++i)
#pragma unroll
          for (int j = 0; j < 8; ++j) a[i][j] = fma(-g[i], pr[j], a[i][j]);
        // column / row of step k + 1 into the other buffer (owners known beforehand: no search)
        if (k + 1 < n) {
          if (kk < 15) {
            if (J == kk + 1) {
#pragma unroll
              for (int i = 0; i < 8; ++i) gn[16 * i + I] = a[i][jp];
            }
            if (I == kk + 1) {
#pragma unroll
              for (int j = 0; j < 8; ++j) gn[128 + 16 * j + J] = (j == jp && J == kk + 1) ? a[jp][j] + 1.0 : a[jp][j];
            }
          } else {
            constexpr int kLast = 7;
            const int jn = jp < kLast ? jp + 1 : kLast;  // (jp == 7 never gets here with k + 1 < n <= 128)
            if (J == 0) {
#pragma unroll
              for (int i = 0; i < 8; ++i) gn[16 * i + I] = a[i][jn];
            }
            if (I == 0) {
#pragma unroll
              for (int j = 0; j < 8; ++j) gn[128 + 16 * j + J] = (j == jn && J == 0) ? a[jn][j] + 1.0 : a[jn][j];
            }
          }
        }
      }
      w.sync();
      buf ^= 1;
    }
  }
  w.sync();  // (the last reads of the exchange buffers are done: L.A takes the result)
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    const int r = I + 16 * i;
    if (act && r < n) {
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const int col = J + 16 * j;
        if (col < n) L.A[r * ld + col] = a[i][j];
      }
    }
  }
  w.sync();
  return !degenerate;
}
#endif

// ---- pieces of the body that depend on its arithmetic T
// inverse of the nd x nd distance matrix: FP64 takes invert_small (cofactors + one Newton step in double-double where the
// cell is badly shaped); the wide arithmetic takes the cofactor formula as it stands (31 digits to start from)
template <class T>
PFV_FN bool invert_small_t(int nd, const T (*D)[3], T (*R)[3]) {
  if constexpr (std::is_same<T, double>::value) {
    return invert_small(nd, D, R);
  } else {
    if (nd == 2) {
      const T det = D[0][0] * D[1][1] - D[0][1] * D[1][0];
      const T id = T(1.0) / det;
      R[0][0] = D[1][1] * id;
      R[0][1] = -D[0][1] * id;
      R[1][0] = -D[1][0] * id;
      R[1][1] = D[0][0] * id;
      const double dh = t_dbl(det);
      return dh != 0.0 && dh == dh;
    }
    const T c00 = D[1][1] * D[2][2] - D[1][2] * D[2][1];
    const T c01 = D[1][2] * D[2][0] - D[1][0] * D[2][2];
    const T c02 = D[1][0] * D[2][1] - D[1][1] * D[2][0];
    const T det = D[0][0] * c00 + D[0][1] * c01 + D[0][2] * c02;
    const T id = T(1.0) / det;
    R[0][0] = c00 * id;
    R[1][0] = c01 * id;
    R[2][0] = c02 * id;
    R[0][1] = (D[0][2] * D[2][1] - D[0][1] * D[2][2]) * id;
    R[1][1] = (D[0][0] * D[2][2] - D[0][2] * D[2][0]) * id;
    R[2][1] = (D[0][1] * D[2][0] - D[0][0] * D[2][1]) * id;
    R[0][2] = (D[0][1] * D[1][2] - D[0][2] * D[1][1]) * id;
    R[1][2] = (D[0][2] * D[1][0] - D[0][0] * D[1][2]) * id;
    R[2][2] = (D[0][0] * D[1][1] - D[0][1] * D[1][0]) * id;
    const double dh = t_dbl(det), ih = t_dbl(id);
    return dh != 0.0 && dh == dh && ih - ih == 0.0;
  }
}

// In-place Gauss-Jordan with partial pivoting in the arithmetic T on a matrix in the work item's scratch (LDS or global
// memory), any lane count: the pivot search runs on the FP64 image of the column (keyd), the update over all n x n
// entries strided over the lanes.  The plain statement of node_gj_lds; the path of the few wide regions, not a hot one.
// A pivot below kPivotTiny of the row-scaled system is a singular input (status word 0), as everywhere else.
constexpr double kPivotTinyWide = 1.0e-28;
template <class T>
PFV_FN void gj_wide(const WaveCtx& w, T* A, T* rowk, T* colk, double* keyd, int32_t* ipiv, int n, int ld, int v,
                    int32_t* st, double tiny) {
  for (int k = 0; k < n; ++k) {
    PFV_LANES(i, n) {
      const double x = fabs(t_dbl(A[i * ld + k]));
      keyd[i] = (x == x) ? x : 0.0;  // (NaN: a candidate of magnitude zero -- argmax_abs takes |key|; rows below k are not scanned)
    }
    w.sync();
    double best;
    int p = w.argmax_abs(keyd, 1, k, n, &best);
    // (a column without a candidate -- every entry NaN after a zero pivot of a singular input -- leaves the device's
    // reduction without an index: the step then takes the diagonal, the status word already says "singular")
    if (p < k || p >= n) p = k;
    // (pivots of a regular region fall to ~1 / contrast of the row-scaled system; those of a singular one to the rounding
    // of the FP64 INPUTS, ~1e-16 -- the coordinates and tensors the system is an exact function of are themselves rounded,
    // so "singular" shows at that level whatever the arithmetic: `tiny` is the FP64 body's 1e-13 divided by the region's
    // contrast, floored at kPivotTinyWide.  A region without contrast -- a sliver, a failed unpivoted check -- keeps the
    // FP64 body's verdicts exactly)
    if (!(best > tiny && best < 1.0e300)) {
      if (w.lane0()) atomic_max_i32(st + 0, v + 1);
    }
    if (w.lane0()) ipiv[k] = p;
    if (p != k) {
      PFV_LANES(cc, n) {
        const T t = A[k * ld + cc];
        A[k * ld + cc] = A[p * ld + cc];
        A[p * ld + cc] = t;
      }
    }
    w.sync();
    const T pivinv = T(1.0) / A[k * ld + k];
    PFV_LANES(cc, n) {
      rowk[cc] = (cc == k) ? pivinv : A[k * ld + cc] * pivinv;
      colk[cc] = A[cc * ld + k];
    }
    w.sync();
    PFV_LANES(idx, n * n) {
      const int i = idx / n, c = idx - i * n;
      const T rk = rowk[c];
      A[i * ld + c] = (i == k) ? rk : (((c == k) ? T(0.0) : A[i * ld + c]) - colk[i] * rk);
    }
    w.sync();
  }
  for (int k = n - 1; k >= 0; --k) {
    const int p = ipiv[k];
    if (p != k) {
      PFV_LANES(r, n) {
        const T t = A[r * ld + k];
        A[r * ld + k] = A[r * ld + p];
        A[r * ld + p] = t;
      }
      w.sync();
    }
  }
}

// BASIS: boundary conditions in a face-wise basis (rows of a boundary sub-face mix the Cartesian
// components); without it every row involves its own component only and the inner loops collapse
// LEAN: the body without the stages that only special inputs take -- iterative refinement of ill-conditioned regions,
// continuity points per sub-face, reconstruction_eta, the Biot terms.  Compiled in, they cost the common path registers
// (256 VGPRs, 322 spilled SGPRs: 63 -> 68 ms at configs[3]).  A lean launch hands the nodes whose kappa asks for
// refinement to a redo list (a.redo / a.st[2]); the full body then runs on those alone.
template <int ND, bool BASIS, bool LEAN = false, class T = double>
PFV_FN void mpsa_node_body(const MpsaArgs& a, const WaveCtx& w, int64_t first) {
  constexpr bool kWide = !std::is_same<T, double>::value;  // dd arithmetic: no refinement stages, no register elimination
  static_assert(!(kWide && LEAN), "the wide body is a full body");
  constexpr int N2 = ND * ND;
  const double* const arg_eta_sub = LEAN ? nullptr : a.eta_sub;
  double* const arg_Et2 = LEAN ? nullptr : a.Et2;
  double* const arg_Etb2 = LEAN ? nullptr : a.Etb2;
  const int arg_nalpha = LEAN ? 0 : a.nalpha;
  const int v = a.order[first + w.item];
  if (a.active && !a.active[v]) return;
  if constexpr (!kWide) {
    if (a.wide && a.wide[v]) return;  // (assembled and eliminated in double-double by the launch over the wide list)
  }
  const int h0 = a.hp[v], nh = a.hp[v + 1] - h0, deg = nh / ND;
  const int f0 = a.fp[v], nsf = a.fp[v + 1] - f0;
  if (nsf == 0) return;
  const int b0 = a.bp[v], nb = a.bp[v + 1] - b0;
  const int n = ND * nsf, ld = n | 1, ncu = ND * deg, ncb = ND * nb;
  const int64_t nc = a.nc, nf = a.nf, nn = a.nn;
  MpsaLdsT<T> L;
  mpsa_carve(w.lds, nsf, deg, nb, ND, L, arg_nalpha > 0);

  // ---- sub-faces: classification per component, side lists
  PFV_LANES(l, nsf) {
    const int f = a.node_face[f0 + l];
    const int64_t bi = a.sub_bc ? a.node_sf[f0 + l] : f;  // column of the condition arrays
    const bool bnd = a.nsides[f] == 1;
    L.fid[l] = f;
    if (l == 0) L.ipiv[n + 1] = 0;  // refinement steps asked for by the inverse (below)
    L.sideh[2 * l] = -1;
    L.sideh[2 * l + 1] = -1;
    for (int c = 0; c < ND; ++c) {
      int t = 0;
      if (bnd) {
        if (a.dirbits[bi] & (1u << c)) t = 1;
        else if (a.neubits[bi] & (1u << c)) t = 2;
        else if (a.robbits && (a.robbits[bi] & (1u << c))) t = 3;
        else { t = 2; atomic_max_i32(a.st + 1, 1); }
      }
      L.type[ND * l + c] = (uint8_t)t;
      for (int c2 = 0; c2 < ND; ++c2)
        L.basisL[((size_t)l * ND + c) * ND + c2] =
            (bnd && a.basis) ? a.basis[(int64_t)(ND * c + c2) * a.nbc + bi] : (c == c2 ? 1.0 : 0.0);
    }
  }
  w.sync();
  // ---- sub-cells: D^-1, Omega, Pi (unweighted), normals, weights
  PFV_LANES(j, deg) {
    const int cell = a.h_cell[h0 + ND * j];
    T D[3][3], Di[3][3], nh_[3][3], xc[3], xv[3];
    for (int i = 0; i < 3; ++i)
      for (int k = 0; k < 3; ++k) D[i][k] = 0.0;
    for (int i = 0; i < ND; ++i) {
      xc[i] = a.ccen[i * nc + cell];
      xv[i] = a.nodes[i * nn + v];
    }
    for (int k = 0; k < ND; ++k) {
      const int hh = ND * j + k;
      const int l = a.h_lf[h0 + hh];
      const int f = L.fid[l];
      const bool bnd = a.nsides[f] == 1;
      const T inn = 1.0 / (a.fn_ptr[f + 1] - a.fn_ptr[f]);
      const T et = arg_eta_sub ? arg_eta_sub[a.node_sf[f0 + l]] : (bnd ? 0.0 : a.eta);
      for (int i = 0; i < ND; ++i) {
        nh_[k][i] = a.fnorm[i * nf + f] * inn;
        L.nvec[hh * ND + i] = nh_[k][i];
        const T xf = a.fcen[i * nf + f];
        D[k][i] = xf + et * (xv[i] - xf) - xc[i];
      }
      L.lfL[hh] = (uint8_t)l;
      L.sgL[hh] = a.h_sgn[h0 + hh];
      L.sideh[2 * l + (a.h_first[h0 + hh] ? 0 : 1)] = hh;
      if (a.h_first[h0 + hh]) L.firsth[l] = hh;
    }
    if (!invert_small_t<T>(ND, D, Di)) atomic_max_i32(a.st + 0, v + 1);
    for (int l = 0; l < ND; ++l)
      for (int k = 0; k < ND; ++k) L.Dinv[(size_t)j * N2 + l * ND + k] = Di[l][k];
    L.wj[j] = a.cvol[cell] / T((double)a.cell_nnodes[cell]);
  }
  w.sync();
  // stiffness of the cell (reference layout [9][9][Nc]; 2-D keeps rows/cols 0,1,3,4): one lane per
  // (sub-cell, stress row qi) -- 81 strided loads per sub-cell are a long serial chain for one lane;
  // the qk = 0, 1, 2 contributions to Omega stay in one lane, in order
  PFV_LANES(x, deg * ND) {
    const int j = x / ND, qi = x - j * ND;
    const int cell = a.h_cell[h0 + ND * j];
    T Di[3][3];
    for (int l = 0; l < ND; ++l)
      for (int k = 0; k < ND; ++k) Di[l][k] = L.Dinv[(size_t)j * N2 + l * ND + k];
    for (int qk = 0; qk < ND; ++qk) {
      const int q = qi * ND + qk;
      const int q9 = 3 * qi + qk;
      for (int aa = 0; aa < ND; ++aa) {
        T casym_l[3], csym_l[3];
        for (int l = 0; l < ND; ++l) {
          const int r = ND * aa + l, r9 = 3 * aa + l;
          const T cv_ = a.stiff[((int64_t)q9 * 9 + r9) * nc + cell];
          const bool sym = (q == r) || (qi == qk && aa == l);
          csym_l[l] = sym ? cv_ : 0.0;
          casym_l[l] = sym ? 0.0 : cv_;
        }
        for (int k = 0; k < ND; ++k) {
          T pa = 0.0;
          for (int l = 0; l < ND; ++l) pa += casym_l[l] * Di[l][k];
          L.Pi[((size_t)j * N2 + q) * N2 + aa * ND + k] = pa;
        }
        // Omega_h[i = qi][aa][k] += n_h[qk] * sum_l Csym[q][nd aa + l] Dinv[l][k]
        for (int kh = 0; kh < ND; ++kh) {
          const T nq = L.nvec[(ND * j + kh) * ND + qk];
          for (int k = 0; k < ND; ++k) {
            T s = 0.0;
            for (int l = 0; l < ND; ++l) s += csym_l[l] * Di[l][k];
            T* dst = L.Om + (((size_t)(ND * j + kh) * ND + qi) * ND + aa) * ND + k;
            if (qk == 0) *dst = nq * s; else *dst += nq * s;
          }
        }
      }
    }
  }
  w.sync();
  if (a.ablate == 1) return;
  T wsum = 0.0;
  for (int j = 0; j < deg; ++j) wsum += L.wj[j];
  const T winv = 1.0 / wsum;
  // corner rule (mpsa.py:1932-2000): per component, more Neumann (resp. Robin) boundary sub-faces
  // than sub-cells -> those rows lose the asymmetric part.  elim[t - 2][c], t = 2 Neumann, 3 Robin
  int elim[2][3] = {{1, 1, 1}, {1, 1, 1}};
  for (int c = 0; c < ND; ++c) {
    int cn = 0, cr = 0;
    for (int l = 0; l < nsf; ++l) {
      cn += (L.type[ND * l + c] == 2) ? 1 : 0;
      cr += (L.type[ND * l + c] == 3) ? 1 : 0;
    }
    if (cn > deg) elim[0][c] = 0;
    if (cr > deg) elim[1][c] = 0;
  }
  // ---- P as a linear map: PL (N2 x n) on Lambda, PU (N2 x ncu) on u
  PFV_LANES(x, N2 * n) {
    const int q = x / n, col = x - q * n;
    const int s = col / ND, aa = col - s * ND;
    T acc = 0.0;
    for (int sd = 0; sd < 2; ++sd) {
      const int hh = L.sideh[2 * s + sd];
      if (hh >= 0) {
        const int j = hh / ND, k = hh - j * ND;
        acc += L.wj[j] * winv * L.Pi[((size_t)j * N2 + q) * N2 + aa * ND + k];
      }
    }
    L.PL[x] = acc;
  }
  PFV_LANES(x, N2 * ncu) {
    const int q = x / ncu, cidx = x - q * ncu;
    const int j = cidx / ND, aa = cidx - j * ND;
    T acc = 0.0;
    for (int k = 0; k < ND; ++k) acc -= L.Pi[((size_t)j * N2 + q) * N2 + aa * ND + k];
    L.PU[x] = acc * L.wj[j] * winv;
  }
  PFV_LANES(i, n * ld) L.A[i] = 0.0;
  w.sync();
  // ---- assemble A row by row (one lane per row: no conflicts).  Row k of a boundary sub-face is
  //      sum_c B[k][c] (Cartesian row c) of its basis (numerics/fv/_fvutils.py:836-1083); the corner
  //      rule keeps indexing the asymmetric part by component number (mpsa.py:1968-1999)
  PFV_LANES(r, n) {
    const int s = r / ND, i = r - s * ND;
    const int t = L.type[r];
    const int f = L.fid[s];
    const T inn = 1.0 / (a.fn_ptr[f + 1] - a.fn_ptr[f]);
    const T* Bk = L.basisL + (size_t)r * ND;
    T* row = L.A + (size_t)r * ld;
    if (t == 1) {
      for (int c = 0; c < ND; ++c) row[ND * s + c] = Bk[c];
      L.beta[r] = 1.0;
    } else {
      L.beta[r] = (t >= 2) ? (a.sub_bc ? 1.0 : inn) : 0.0;  // data per sub-face are integrated over the sub-face (mpsa.py:1127-1138)
      if (t == 3) {  // Robin: + W B (area / #nodes) u(x_cp), and u(x_cp) is the unknown Lambda_s itself
        const T wa = a.farea[f] * inn;
        for (int aa = 0; aa < ND; ++aa) {
          T wb = 0.0;
          for (int jj = 0; jj < ND; ++jj)
            wb += (a.robw ? a.robw[((int64_t)(ND * i + jj)) * a.nbc + (a.sub_bc ? (int64_t)a.node_sf[f0 + s] : (int64_t)f)]
                          : (jj == i ? 1.0 : 0.0)) *
                  L.basisL[((size_t)s * ND + jj) * ND + aa];
          row[ND * s + aa] += wa * wb;
        }
      }
      for (int c = BASIS ? 0 : i; c < (BASIS ? ND : i + 1); ++c) {
        const T wgt = BASIS ? Bk[c] : 1.0;
        if (BASIS && wgt == 0.0) continue;
        const int tc = L.type[ND * s + c];
        const bool keep_asym = t >= 2 && !(tc >= 2 && !elim[tc - 2][c]);
        for (int sd = 0; sd < 2; ++sd) {
          const int hh = L.sideh[2 * s + sd];
          if (hh < 0) continue;
          const int j = hh / ND;
          const T sg = wgt * T((double)L.sgL[hh]);
          for (int aa = 0; aa < ND; ++aa)
            for (int k = 0; k < ND; ++k)
              row[ND * L.lfL[ND * j + k] + aa] += sg * L.Om[(((size_t)hh * ND + c) * ND + aa) * ND + k];
          if (keep_asym) {
            for (int kp = 0; kp < ND; ++kp) {
              const T g = sg * L.nvec[hh * ND + kp];
              const T* pl = L.PL + (size_t)(ND * c + kp) * n;
              for (int col = 0; col < n; ++col) row[col] += g * pl[col];
            }
          }
        }
      }
    }
  }
  w.sync();
  PFV_LANES(r, n) {
    T sum = 0.0;
    for (int cc = 0; cc < n; ++cc) sum += t_abs(L.A[r * ld + cc]);
    if (!finite_pos(t_dbl(sum))) atomic_max_i32(a.st + 0, v + 1);
    const T sc = 1.0 / sum;
    L.scale[r] = sc;
    for (int cc = 0; cc < n; ++cc) L.A[r * ld + cc] *= sc;
  }
  w.sync();
  if (a.ablate == 2) return;
  bool np_used = false, np_ok = true;
#ifndef PFV_EMULATE
  if constexpr (LEAN) {
    if (n <= 128 && !a.lds_gj && a.nopivot && a.redo) {
      np_used = true;
      np_ok = mpsa_gj_reg_np(w, L, n, ld);
    }
  }
  if (np_used) {
  } else if (!kWide && n <= 128 && !a.lds_gj) {
    if constexpr (!kWide) mpsa_gj_reg(w, L, n, ld, v, a.st);
  } else
#endif
  if constexpr (kWide) {
    {
      const int ex = a.wide_exp ? (int)a.wide_exp[v] : 0;
      double tiny = kPivotTiny;
      for (int e = 0; e < ex; ++e) tiny *= 0.5;
      gj_wide(w, L.A, L.rowk, L.colk, L.keyd, L.ipiv, n, ld, v, a.st, tiny > kPivotTinyWide ? tiny : kPivotTinyWide);
    }
  } else {
    NodeLds G;
    G.A = L.A; G.rowk = L.rowk; G.colk = L.colk; G.ipiv = L.ipiv;
    node_gj_lds(w, G, n, ld, v, a.st);
  }
  // kappa = ||(S A)^-1||_inf of the row-scaled system (mpfa_numeric.inc: kRefineKappa)
  if (!kWide && a.refine >= 0) {
    // (row sums once, four independent partial sums per lane: a plain loop waits for every LDS load before it issues
    // the next -- 2 x 108 exposed round trips per node, 2.3 ms of the 69 at configs[3])
    PFV_LANES(r, n) {
      const T* row = L.A + (size_t)r * ld;
      T s0 = 0.0, s1 = 0.0, s2 = 0.0, s3 = 0.0;
      int cc = 0;
      for (; cc + 3 < n; cc += 4) {
        s0 += t_abs(row[cc]);
        s1 += t_abs(row[cc + 1]);
        s2 += t_abs(row[cc + 2]);
        s3 += t_abs(row[cc + 3]);
      }
      for (; cc < n; ++cc) s0 += t_abs(row[cc]);
      L.rowk[r] = (s0 + s1) + (s2 + s3);
    }
    w.sync();
    for (int want = 1; want <= 2; ++want) {  // (all lanes that write in one round write the same value)
      PFV_LANES(r, n) {
        if (refine_steps_for(t_dbl(L.rowk[r]), a.refine) >= want) L.ipiv[n + 1] = want;
      }
      w.sync();
    }
  }
  PFV_LANES(idx, n * n) {
    const int r = idx / n, cc = idx - r * n;
    L.A[r * ld + cc] *= L.scale[cc];
  }
  w.sync();
  // ---- ill-conditioned interaction region (slivers): iterative refinement of the inverse, column by column,
  // x_c += X (e_c - A x_c), with A applied from its defining coefficients (Omega, PL, Robin / basis terms: the same
  // sums the assembly above forms, so the residual is accurate componentwise) -- the Gauss-Jordan overwrote A.
  // The columns already refined serve as part of the corrector X for the later ones.
  if constexpr (LEAN) {
    if (a.refine >= 0 && L.ipiv[n + 1] > 0) {  // (workgroup-uniform: the flag went through LDS and a barrier)
      if (w.lane0()) a.redo[atomic_fetch_add_i32(a.st + 2, 1)] = v;
      return;
    }
  }
  const int refine_steps = (LEAN || kWide) ? 0 : (a.refine >= 0 ? L.ipiv[n + 1] : 0);  // (106 bits need no refinement)
  // row r of the (unscaled) condensed matrix applied to x; y = PL x
  auto a_row_times = [&](int r, const T* xv, const T* yv) -> T {
    const int s = r / ND, i = r - s * ND;
    const int t = L.type[r];
    const int f = L.fid[s];
    const T inn = 1.0 / (a.fn_ptr[f + 1] - a.fn_ptr[f]);
    const T* Bk = L.basisL + (size_t)r * ND;
    T val = 0.0;
    if (t == 1) {
      for (int c = 0; c < ND; ++c) val += Bk[c] * xv[ND * s + c];
      return val;
    }
    if (t == 3) {
      const T wa = a.farea[f] * inn;
      for (int aa = 0; aa < ND; ++aa) {
        T wb = 0.0;
        for (int jj = 0; jj < ND; ++jj)
          wb += (a.robw ? a.robw[((int64_t)(ND * i + jj)) * a.nbc + (a.sub_bc ? (int64_t)a.node_sf[f0 + s] : (int64_t)f)]
                        : (jj == i ? 1.0 : 0.0)) *
                L.basisL[((size_t)s * ND + jj) * ND + aa];
        val += wa * wb * xv[ND * s + aa];
      }
    }
    for (int c = BASIS ? 0 : i; c < (BASIS ? ND : i + 1); ++c) {
      const T wgt = BASIS ? Bk[c] : 1.0;
      if (BASIS && wgt == 0.0) continue;
      const int tc = L.type[ND * s + c];
      const bool keep_asym = t >= 2 && !(tc >= 2 && !elim[tc - 2][c]);
      for (int sd = 0; sd < 2; ++sd) {
        const int hh = L.sideh[2 * s + sd];
        if (hh < 0) continue;
        const int j = hh / ND;
        const T sg = wgt * T((double)L.sgL[hh]);
        T acc = 0.0;
        for (int aa = 0; aa < ND; ++aa)
          for (int k = 0; k < ND; ++k)
            acc += L.Om[(((size_t)hh * ND + c) * ND + aa) * ND + k] * xv[ND * L.lfL[ND * j + k] + aa];
        if (keep_asym)
          for (int kp = 0; kp < ND; ++kp) acc += L.nvec[hh * ND + kp] * yv[ND * c + kp];
        val += sg * acc;
      }
    }
    return val;
  };
#ifndef PFV_EMULATE
  if constexpr (LEAN) {
    if (np_used) {
      // ---- a-posteriori check of the unpivoted inverse X (mpsa_gj_reg_np): with the fixed vector f of freivalds_v
      // and v = S^-1 f, the scaled residual S (v - A X v) = f - (S A)(S A)^-1 f must stay within the rounding of a
      // stable elimination, kNoPivotResidual * kappa (mpfa_numeric.inc); A is applied from its defining coefficients.
      unsigned* kw = reinterpret_cast<unsigned*>(L.gjx + 300);  // [0] kappa (float bits), [1] verdict
      if (w.lane0()) {
        kw[0] = 0u;
        kw[1] = 0u;
      }
      w.sync();
      if (!np_ok) kw[1] = 1u;
      PFV_LANES(r, n) atomicMax(kw, __float_as_uint((float)L.rowk[r]));  // (row sums of |(S A)^-1| from above)
      PFV_LANES(cc, n) L.colk[cc] = freivalds_v(cc) / L.scale[cc];
      w.sync();
      const T kappa = (T)__uint_as_float(kw[0]);
      T* tv = L.rowk;
      T* yv2 = L.gjx;
      PFV_LANES(r, n) {
        const T* row = L.A + (size_t)r * ld;
        T s0 = 0.0, s1 = 0.0;
        int cc = 0;
        for (; cc + 1 < n; cc += 2) {
          s0 = fma(row[cc], L.colk[cc], s0);
          s1 = fma(row[cc + 1], L.colk[cc + 1], s1);
        }
        for (; cc < n; ++cc) s0 = fma(row[cc], L.colk[cc], s0);
        tv[r] = s0 + s1;
      }
      w.sync();
      PFV_LANES(q, N2) {
        T acc = 0.0;
        for (int cc = 0; cc < n; ++cc) acc += L.PL[(size_t)q * n + cc] * tv[cc];
        yv2[q] = acc;
      }
      w.sync();
      const T tol = a.np_tol * (kappa > 1.0 ? kappa : 1.0);
      PFV_LANES(r, n) {
        const T res = (L.colk[r] - a_row_times(r, tv, yv2)) * L.scale[r];
        if (!(t_abs(res) <= tol)) kw[1] = 1u;  // (NaN fails)
      }
      w.sync();
      if (kw[1] != 0u) {  // (workgroup-uniform) left to the pivoted full body
        if (w.lane0()) a.redo[atomic_fetch_add_i32(a.st + 2, 1)] = v;
        return;
      }
    }
  }
#endif
  // `steps` rounds of x += X (b - A x) on the vector x (LDS, n entries); r and y are LDS scratch (n, N2)
  auto refine_vector = [&](T* xv, const T* bv, T* rv, T* yv, int steps) {
    for (int it = 0; it < steps; ++it) {
      PFV_LANES(q, N2) {
        T acc = 0.0;
        for (int cc = 0; cc < n; ++cc) acc += L.PL[(size_t)q * n + cc] * xv[cc];
        yv[q] = acc;
      }
      w.sync();
      PFV_LANES(r, n) rv[r] = bv[r] - a_row_times(r, xv, yv);
      w.sync();
      PFV_LANES(r, n) {  // (reads rv and X only: every lane updates its own entry of x)
        T acc = 0.0;
        for (int l = 0; l < n; ++l) acc += L.A[r * ld + l] * rv[l];
        xv[r] += acc;
      }
      w.sync();
    }
  };
  // entry [(s, k)][(i, kp)] of Gamma: what a unit averaged-asymmetric stress component leaves on the Neumann / Robin rows
  auto gamma_entry = [&](int row, int q) -> T {
    const int s = row / ND, k = row - s * ND;
    const int i = q / ND, kp = q - i * ND;
    if (L.type[row] < 2) return 0.0;
    const int tc = L.type[ND * s + i];
    if (tc >= 2 && !elim[tc - 2][i]) return 0.0;
    if (!BASIS && k != i) return 0.0;
    const T wgt = BASIS ? L.basisL[((size_t)s * ND + k) * ND + i] : 1.0;
    const int hh = L.sideh[2 * s];
    return wgt * T((double)L.sgL[hh]) * L.nvec[hh * ND + kp];
  };
  T* xv = L.rowk;
  T* rv = L.colk;
  T* bv = L.scale;  // (the row scales are dead from here on)
  T* yv = L.gjx;    // PL x (N2 values; the exchange area of the Gauss-Jordan is free)
  if (refine_steps > 0) {
    for (int col = 0; col < n; ++col) {
      PFV_LANES(r, n) {
        xv[r] = L.A[r * ld + col];
        bv[r] = (r == col) ? 1.0 : 0.0;
      }
      w.sync();
      refine_vector(xv, bv, rv, yv, refine_steps);
      PFV_LANES(r, n) L.A[r * ld + col] = xv[r];
      w.sync();
    }
  }
  if (a.ablate == 3) return;

  // ---- AG = Ainv Gamma (response of Lambda to the averaged-asymmetric rhs of the Neumann rows),
  //      PLA = PL Ainv, PLAG = PLA Gamma
  PFV_LANES(x, n * N2) {
    const int rho = x / N2, q = x - rho * N2;
    const int i = q / ND, kp = q - i * ND;
    T acc = 0.0;
    for (int s = 0; s < nsf; ++s) {
      const int tc = L.type[ND * s + i];
      if (tc >= 2 && !elim[tc - 2][i]) continue;  // asymmetric part of component i dropped on this sub-face
      const int hh = L.sideh[2 * s];
      for (int k = BASIS ? 0 : i; k < (BASIS ? ND : i + 1); ++k) {  // Neumann / Robin rows containing component i
        if (L.type[ND * s + k] < 2) continue;
        const T wgt = BASIS ? L.basisL[((size_t)s * ND + k) * ND + i] : 1.0;
        if (wgt != 0.0) acc += L.A[rho * ld + ND * s + k] * wgt * T((double)L.sgL[hh]) * L.nvec[hh * ND + kp];
      }
    }
    L.AG[x] = acc;
  }
  PFV_LANES(x, N2 * n) {
    const int q = x / n, col = x - q * n;
    T acc = 0.0;
    for (int rho = 0; rho < n; ++rho) acc += L.PL[(size_t)q * n + rho] * L.A[rho * ld + col];
    L.PLA[x] = acc;
  }
  w.sync();
  PFV_LANES(x, N2 * N2) {
    const int q = x / N2, q2 = x - q * N2;
    T acc = 0.0;
    for (int rho = 0; rho < n; ++rho) acc += L.PL[(size_t)q * n + rho] * L.AG[rho * N2 + q2];
    L.PLAG[x] = acc;
  }
  w.sync();
  if (a.ablate == 4) return;

  // ---- Lambda response to unit cell displacements (= trace rows), and P response
  // (FP64 body: the caller's arrays are the working arrays; wide body: its own, rounded into the caller's on the way)
  T* Et;
  if constexpr (kWide) Et = L.EtW; else Et = a.Et + a.eptr[v];
  double* const Et_out = a.Et + a.eptr[v];
  double* Es = a.Es + a.eptr[v];
  // One lane per cell column (j, aa) and slice of the rows: the N2 coefficients sg * sum Omega of the column
  // and its PU entries are formed once and kept in registers, every output then costs 2 N2 LDS reads
  // (the first version re-formed them per entry: ~75 reads each, the stage was LDS-bandwidth bound).
  {
    const int G = w.width / ncu > 0 ? w.width / ncu : 1;  // row slices
    for (int u = w.lane; u < ncu * G; u += w.width) {
      const int cidx = u % ncu, grp = u / ncu;
      const int j = cidx / ND, aa = cidx - j * ND;
      T coef[N2], puv[N2];
      int colm[N2];
      for (int kh = 0; kh < ND; ++kh) {
        const int hh = ND * j + kh;
        const int s = L.lfL[hh];
        const T sg = T((double)L.sgL[hh]);
        for (int kr = 0; kr < ND; ++kr) {
          T om = 0.0;
          for (int i = BASIS ? 0 : kr; i < (BASIS ? ND : kr + 1); ++i) {
            const T wgt = BASIS ? L.basisL[((size_t)s * ND + kr) * ND + i] : 1.0;
            if (BASIS && wgt == 0.0) continue;
            for (int k = 0; k < ND; ++k) om += wgt * L.Om[(((size_t)hh * ND + i) * ND + aa) * ND + k];
          }
          coef[kh * ND + kr] = sg * om;
          colm[kh * ND + kr] = (L.type[ND * s + kr] == 1) ? -1 : ND * s + kr;  // Dirichlet rows carry no cell term
        }
      }
      for (int q = 0; q < N2; ++q) puv[q] = L.PU[(size_t)q * ncu + cidx];
      for (int rho = grp; rho < n; rho += G) {
        T acc = 0.0;
        for (int m = 0; m < N2; ++m)
          if (colm[m] >= 0) acc += L.A[rho * ld + colm[m]] * coef[m];
        for (int q = 0; q < N2; ++q) acc -= L.AG[rho * N2 + q] * puv[q];
        Et[(size_t)rho * ncu + cidx] = acc;
        if constexpr (kWide) Et_out[(size_t)rho * ncu + cidx] = t_dbl(acc);
      }
      for (int q = grp; q < N2; q += G) {
        T acc = puv[q];
        for (int m = 0; m < N2; ++m)
          if (colm[m] >= 0) acc += L.PLA[(size_t)q * n + colm[m]] * coef[m];
        for (int q2 = 0; q2 < N2; ++q2) acc -= L.PLAG[q * N2 + q2] * puv[q2];
        L.Ptot[(size_t)q * ncu + cidx] = acc;
      }
    }
  }
  if (refine_steps > 0) {
    // the responses to unit cell displacements are X b with right-hand sides b ~ Omega ~ D^-1 that are large on
    // slivers: an accurate inverse is not enough (error eps |X| |b| against a result of order 1) -- refine every
    // column against its own right-hand side, then P = PU + PL Lambda from the refined column
    w.sync();  // Et of this node is read back
    for (int cidx = 0; cidx < ncu; ++cidx) {
      const int j = cidx / ND, aa = cidx - j * ND;
      PFV_LANES(r, n) {
        xv[r] = Et[(size_t)r * ncu + cidx];
        bv[r] = 0.0;
      }
      w.sync();
      PFV_LANES(m, N2) {  // (the nd sub-faces of a sub-cell are distinct: no two m share a row)
        const int kh = m / ND, kr = m - kh * ND;
        const int hh = ND * j + kh;
        const int s = L.lfL[hh];
        if (L.type[ND * s + kr] != 1) {
          T om = 0.0;
          for (int i = BASIS ? 0 : kr; i < (BASIS ? ND : kr + 1); ++i) {
            const T wgt = BASIS ? L.basisL[((size_t)s * ND + kr) * ND + i] : 1.0;
            if (BASIS && wgt == 0.0) continue;
            for (int k = 0; k < ND; ++k) om += wgt * L.Om[(((size_t)hh * ND + i) * ND + aa) * ND + k];
          }
          bv[ND * s + kr] = T((double)L.sgL[hh]) * om;
        }
      }
      w.sync();
      PFV_LANES(r, n) {
        T acc = 0.0;
        for (int q = 0; q < N2; ++q) acc += gamma_entry(r, q) * L.PU[(size_t)q * ncu + cidx];
        bv[r] -= acc;
      }
      w.sync();
      refine_vector(xv, bv, rv, yv, refine_steps);
      PFV_LANES(r, n) {
        Et[(size_t)r * ncu + cidx] = xv[r];
        if constexpr (kWide) Et_out[(size_t)r * ncu + cidx] = t_dbl(xv[r]);
      }
      PFV_LANES(q, N2) {
        T acc = L.PU[(size_t)q * ncu + cidx];
        for (int rho = 0; rho < n; ++rho) acc += L.PL[(size_t)q * n + rho] * xv[rho];
        L.Ptot[(size_t)q * ncu + cidx] = acc;
      }
      w.sync();
    }
  }
  T* Etb;
  if constexpr (kWide) Etb = L.EtbW; else Etb = a.Etb + a.ebptr[v];
  double* const Etb_out = a.Etb + a.ebptr[v];
  double* Esb = a.Esb + a.ebptr[v];
  PFV_LANES(x, n * ncb) {
    const int rho = x / ncb, bidx = x - rho * ncb;
    const int bi = bidx / ND, aa = bidx - bi * ND;
    const int col = ND * (int)a.bls[b0 + bi] + aa;
    Etb[x] = L.A[rho * ld + col] * L.beta[col];
    if constexpr (kWide) Etb_out[x] = t_dbl(Etb[x]);
  }
  PFV_LANES(x, N2 * ncb) {
    const int q = x / ncb, bidx = x - q * ncb;
    const int bi = bidx / ND, aa = bidx - bi * ND;
    const int col = ND * (int)a.bls[b0 + bi] + aa;
    L.Pb[x] = L.PLA[(size_t)q * n + col] * L.beta[col];
  }
  w.sync();  // Et / Etb of this node are read back below by other lanes of the workgroup
  if (a.ablate == 5) return;

  // ---- tractions from the first side of every sub-face
  {  // one lane per cell column and slice of the rows (no division by the run-time ncu per entry)
    const int G = w.width / ncu > 0 ? w.width / ncu : 1;
    for (int u = w.lane; u < ncu * G; u += w.width) {
      const int cidx = u % ncu, grp = u / ncu;
      const int j = cidx / ND, aa = cidx - j * ND;
      for (int rho = grp; rho < n; rho += G) {
        const int s = rho / ND, i = rho - s * ND;
        const int hh = L.firsth[s];
        const int js = hh / ND;
        T acc = 0.0;
        for (int a2 = 0; a2 < ND; ++a2)
          for (int k = 0; k < ND; ++k) {
            const T om = L.Om[(((size_t)hh * ND + i) * ND + a2) * ND + k];
            const size_t src = (size_t)(ND * L.lfL[ND * js + k] + a2) * ncu + cidx;
            acc += om * Et[src];
            if (j == js && a2 == aa) acc -= om;
          }
        const int e = (L.type[rho] >= 2 && !elim[L.type[rho] - 2][i]) ? 0 : 1;
        if (e)
          for (int kp = 0; kp < ND; ++kp) acc += L.nvec[hh * ND + kp] * L.Ptot[(size_t)(ND * i + kp) * ncu + cidx];
        Es[(size_t)rho * ncu + cidx] = t_dbl(acc);
      }
    }
  }
  PFV_LANES(x, n * ncb) {
    const int rho = x / ncb, bidx = x - rho * ncb;
    const int s = rho / ND, i = rho - s * ND;
    const int hh = L.firsth[s];
    const int js = hh / ND;
    T acc = 0.0;
    for (int a2 = 0; a2 < ND; ++a2)
      for (int k = 0; k < ND; ++k)
        acc += L.Om[(((size_t)hh * ND + i) * ND + a2) * ND + k] * Etb[(size_t)(ND * L.lfL[ND * js + k] + a2) * ncb + bidx];
    const int e = (L.type[rho] >= 2 && !elim[L.type[rho] - 2][i]) ? 0 : 1;
    if (e)
      for (int kp = 0; kp < ND; ++kp) acc += L.nvec[hh * ND + kp] * L.Pb[(size_t)(ND * i + kp) * ncb + bidx];
    Esb[x] = t_dbl(acc);
  }
  if (arg_Et2) {
    // ---- reconstruction_eta (mpsa.py:757-761, 1187-1266): trace at x' = x_f + hf_eta (x_v - x_f) from the sub-cell
    // gradients, averaged over the sides of the sub-face:  u(x') = u_j + sum_k w_k (Lambda_{lf(j,k)} - u_j),
    // w = (x' - x_cj) D_j^-1  (w = e_k of the face itself when x' is the continuity point: then u(x') = Lambda_s)
    w.sync();  // Et / Etb complete; the Pi | AG | PLA region is dead
    T* W = L.Pi;  // [s][side][k]
    PFV_LANES(x, nsf * 2) {
      const int s = x >> 1, sd = x & 1;
      const int hh = L.sideh[2 * s + sd];
      for (int k = 0; k < ND; ++k) W[(size_t)x * ND + k] = 0.0;
      if (hh >= 0) {
        const int j = hh / ND;
        const int f = L.fid[s];
        const int cell = a.h_cell[h0 + ND * j];
        const T et = a.hf_eta_sub ? a.hf_eta_sub[a.node_sf[f0 + s]] : ((a.nsides[f] == 1) ? 0.0 : a.hf_eta);
        T d[3];
        for (int i = 0; i < ND; ++i) {
          const T xf = a.fcen[i * nf + f];
          d[i] = xf + et * (a.nodes[i * nn + v] - xf) - a.ccen[i * nc + cell];
        }
        for (int k = 0; k < ND; ++k) {
          T t = 0.0;
          for (int i = 0; i < ND; ++i) t += d[i] * L.Dinv[(size_t)j * N2 + i * ND + k];
          W[(size_t)x * ND + k] = t;
        }
      }
    }
    w.sync();
    double* Et2 = arg_Et2 + a.eptr[v];
    double* Etb2 = arg_Etb2 + a.ebptr[v];
    PFV_LANES(x, n * (ncu + ncb)) {
      const int rho = x / (ncu + ncb), col = x - rho * (ncu + ncb);
      const int s = rho / ND, aa = rho - s * ND;
      T acc = 0.0;
      int ns = 0;
      for (int sd = 0; sd < 2; ++sd) {
        const int hh = L.sideh[2 * s + sd];
        if (hh < 0) continue;
        ++ns;
        const int j = hh / ND;
        T wsum = 0.0;
        for (int k = 0; k < ND; ++k) {
          const T wk = W[(size_t)(2 * s + sd) * ND + k];
          wsum += wk;
          const size_t row = (size_t)(ND * L.lfL[ND * j + k] + aa);
          acc += wk * (col < ncu ? Et[row * ncu + col] : Etb[row * ncb + (col - ncu)]);
        }
        if (col == ND * j + aa) acc += 1.0 - wsum;
      }
      acc /= T((double)(ns > 0 ? ns : 1));
      if (col < ncu) Et2[(size_t)rho * ncu + col] = t_dbl(acc);
      else Etb2[(size_t)rho * ncb + (col - ncu)] = t_dbl(acc);
    }
  }
  if (arg_nalpha == 0) return;

  // ---- Biot coupling terms, per coupling tensor alpha (biot.py:714-878, 880-1135).  Pressure enters
  // the traction balance as -alpha p n: rhs of the non-Dirichlet rows; the fluid equation sees
  // alpha : grad u of every sub-cell weighted by its volume V_c / #nodes(c).
  w.sync();  // Etb of this node is read back below
  const int64_t p0 = a.eptr[v] / ND;  // n x deg blocks
  for (int ka = 0; ka < arg_nalpha; ++ka) {
    const double* al = a.alpha + (int64_t)ka * 9 * nc;
    // Lambda response to unit cell pressures: Lp = Ainv Rp, Rp[(s,i)][j] = sum_h sgn (n_h^T alpha_j)_i
    PFV_LANES(x, n * deg) {
      const int rho = x / deg, j = x - rho * deg;
      const int cell = a.h_cell[h0 + ND * j];
      T acc = 0.0;
      for (int kh = 0; kh < ND; ++kh) {
        const int hh = ND * j + kh;
        const int s = L.lfL[hh];
        const T sg = T((double)L.sgL[hh]);
        for (int kr = 0; kr < ND; ++kr) {
          if (L.type[ND * s + kr] == 1) continue;
          T an = 0.0;
          for (int i = BASIS ? 0 : kr; i < (BASIS ? ND : kr + 1); ++i) {
            const T wgt = BASIS ? L.basisL[((size_t)s * ND + kr) * ND + i] : 1.0;
            if (BASIS && wgt == 0.0) continue;
            for (int k = 0; k < ND; ++k) an += wgt * L.nvec[hh * ND + k] * al[(int64_t)(3 * k + i) * nc + cell];
          }
          acc += L.A[rho * ld + ND * s + kr] * sg * an;
        }
      }
      L.Lp[x] = acc;
    }
    w.sync();
    if (refine_steps > 0) {  // as for the displacement columns: every pressure column against its own right-hand side
      for (int j = 0; j < deg; ++j) {
        const int cell = a.h_cell[h0 + ND * j];
        PFV_LANES(r, n) {
          xv[r] = L.Lp[r * deg + j];
          bv[r] = 0.0;
        }
        w.sync();
        PFV_LANES(m, N2) {
          const int kh = m / ND, kr = m - kh * ND;
          const int hh = ND * j + kh;
          const int s = L.lfL[hh];
          if (L.type[ND * s + kr] != 1) {
            T an = 0.0;
            for (int i = BASIS ? 0 : kr; i < (BASIS ? ND : kr + 1); ++i) {
              const T wgt = BASIS ? L.basisL[((size_t)s * ND + kr) * ND + i] : 1.0;
              if (BASIS && wgt == 0.0) continue;
              for (int k = 0; k < ND; ++k) an += wgt * L.nvec[hh * ND + k] * al[(int64_t)(3 * k + i) * nc + cell];
            }
            bv[ND * s + kr] = T((double)L.sgL[hh]) * an;
          }
        }
        w.sync();
        refine_vector(xv, bv, rv, yv, refine_steps);
        PFV_LANES(r, n) L.Lp[r * deg + j] = xv[r];
        w.sync();
      }
    }
    PFV_LANES(x, N2 * deg) {
      const int q = x / deg, j = x - q * deg;
      T acc = 0.0;
      for (int rho = 0; rho < n; ++rho) acc += L.PL[(size_t)q * n + rho] * L.Lp[rho * deg + j];
      L.Pp[x] = acc;
    }
    w.sync();
    double* Esp = a.Esp + (int64_t)ka * a.tot_p + p0;
    double* Etp = a.Etp + (int64_t)ka * a.tot_p + p0;
    PFV_LANES(x, n * deg) {
      const int rho = x / deg, j = x - rho * deg;
      const int s = rho / ND, i = rho - s * ND;
      const int hh = L.firsth[s];
      const int js = hh / ND;
      T acc = 0.0;
      for (int a2 = 0; a2 < ND; ++a2)
        for (int k = 0; k < ND; ++k)
          acc += L.Om[(((size_t)hh * ND + i) * ND + a2) * ND + k] * L.Lp[(ND * L.lfL[ND * js + k] + a2) * deg + j];
      const int e = (L.type[rho] >= 2 && !elim[L.type[rho] - 2][i]) ? 0 : 1;
      if (e)
        for (int kp = 0; kp < ND; ++kp) acc += L.nvec[hh * ND + kp] * L.Pp[(ND * i + kp) * deg + j];
      if (j == js) {
        const int cell = a.h_cell[h0 + ND * js];
        T an = 0.0;
        for (int k = 0; k < ND; ++k) an += L.nvec[hh * ND + k] * al[(int64_t)(3 * k + i) * nc + cell];
        acc -= an;
      }
      Esp[x] = t_dbl(acc);
      Etp[x] = t_dbl(L.Lp[x]);
    }
    // alpha : grad u of sub-cell j = sum_{a,k} dl[a][k] (Lambda_{lf(j,k),a} - u_{j,a}),
    // dl[a][k] = w_j sum_l alpha[a][l] Dinv_j[l][k]
    double* DD = a.DD + (int64_t)ka * a.tot_d + a.dptr[v];
    double* BDD = a.BDD + (int64_t)ka * a.tot_db + a.dbptr[v];
    double* CONS = a.CONS + (int64_t)ka * a.tot_c + a.cptr[v];
    PFV_LANES(x, deg * (ncu + ncb + deg)) {
      const int j = x / (ncu + ncb + deg), col = x - j * (ncu + ncb + deg);
      const int cell = a.h_cell[h0 + ND * j];
      const T wv = L.wj[j];
      T acc = 0.0;
      for (int aa = 0; aa < ND; ++aa)
        for (int k = 0; k < ND; ++k) {
          T dl = 0.0;
          for (int l = 0; l < ND; ++l) dl += al[(int64_t)(3 * aa + l) * nc + cell] * L.Dinv[(size_t)j * N2 + l * ND + k];
          dl *= wv;
          const int row = ND * L.lfL[ND * j + k] + aa;
          T src;
          if (col < ncu) src = Et[(size_t)row * ncu + col] - ((col == ND * j + aa) ? 1.0 : 0.0);
          else if (col < ncu + ncb) src = Etb[(size_t)row * ncb + (col - ncu)];
          else src = L.Lp[row * deg + (col - ncu - ncb)];
          acc += dl * src;
        }
      if (col < ncu) DD[(size_t)j * ncu + col] = t_dbl(acc);
      else if (col < ncu + ncb) BDD[(size_t)j * ncb + (col - ncu)] = t_dbl(acc);
      else CONS[(size_t)j * deg + (col - ncu - ncb)] = t_dbl(acc);
    }
    w.sync();
  }
}

// block expansion of a scalar pattern: row (x, i) of the vector problem has the entries of row x of the
// scalar problem, each expanded to nd columns
static void mpsa_expand_pattern(pfv_ctx_impl& c, const CsrPattern& S, CsrPattern& V) {
  stream_t s = c.stream;
  const int nd = c.nd;
  const int n2 = nd * nd;

    const int64_t nnz = S.nnz * n2;
    if (nnz >= (int64_t(1) << 31)) throw Error(PFV_ERR_UNSUPPORTED, "MPSA matrix with more than 2^31 entries");
    V.nrows = S.nrows * nd;
    V.ncols = S.ncols * nd;
    V.nnz = nnz;
    V.max_row = S.max_row * nd;
    V.indptr.ensure(V.nrows + 1);
    V.indices.ensure(nnz);
    const int32_t* ip = S.indptr;
    const int32_t* ix = S.indices;
    int32_t* vp = V.indptr;
    int32_t* vx = V.indices;
    const int64_t srows = S.nrows;
    parallel_for(s, srows * nd + 1, PFV_LAMBDA(int64_t r) {
      if (r == srows * nd) { vp[r] = ip[srows] * n2; return; }
      const int64_t x = r / nd;
      const int i = (int)(r - x * nd);
      vp[r] = ip[x] * n2 + i * nd * (ip[x + 1] - ip[x]);
    });
    // one lane group per scalar row, consecutive lanes write consecutive entries (a thread per row
    // wrote 9 x len entries with a stride: ~0.3 TB/s)
    wave_for<16>(s, srows, 0, PFV_LAMBDA(const WaveCtx& w) {
      const int64_t x = w.item;
      const int p0 = ip[x], len = ip[x + 1] - p0;
      int32_t* dst = vx + (int64_t)p0 * n2;
      PFV_LANES(o, len * n2) {
        const int i = o / (nd * len);
        const int rem = o - i * nd * len;
        const int k = rem / nd, aa = rem - k * nd;
        (void)i;
        dst[o] = ix[p0 + k] * nd + aa;
      }
    });
}

// ------------------------------------------------------------------------------------------
static void mpsa_symbolic(pfv_ctx_impl& c) {
  ++c.symbolic_epoch;
  stream_t s = c.stream;
  const int nd = c.nd;
  const int64_t nc = c.nc, nf = c.nf, nn = c.nn;
  const int n2 = nd * nd;
  // distinct nodes per cell
  c.cell_nnodes.ensure(nc);
  {
    const int32_t* cf_ptr = c.cf_ptr;
    const int32_t* cf_idx = c.cf_idx;
    const int32_t* fn_ptr = c.fn_ptr;
    const int32_t* fn_idx = c.fn_idx;
    int32_t* out = c.cell_nnodes;
    parallel_for(s, nc, PFV_LAMBDA(int64_t cell) {
      int cnt = 0;
      for (int e = cf_ptr[cell]; e < cf_ptr[cell + 1]; ++e) {
        const int f = cf_idx[e];
        for (int t = fn_ptr[f]; t < fn_ptr[f + 1]; ++t) {
          const int v = fn_idx[t];
          bool seen = false;  // node already met in an earlier (face, position)?
          for (int e2 = cf_ptr[cell]; e2 <= e && !seen; ++e2) {
            const int f2 = cf_idx[e2];
            const int hi = (e2 == e) ? t : fn_ptr[f2 + 1];
            for (int t2 = fn_ptr[f2]; t2 < hi; ++t2)
              if (fn_idx[t2] == v) { seen = true; break; }
          }
          cnt += seen ? 0 : 1;
        }
      }
      out[cell] = cnt;
    });
  }
  // per-node offsets of the expanded rows
  c.node_eptr.ensure(nn + 1);
  c.node_ebptr.ensure(nn + 1);
  {
    Buf<int64_t> sz1, sz2;
    sz1.ensure(nn + 1);
    sz2.ensure(nn + 1);
    const int32_t* hp = c.node_hptr;
    const int32_t* fp = c.node_fptr;
    const int32_t* bp = c.node_bptr;
    int64_t* a1 = sz1;
    int64_t* a2 = sz2;
    parallel_for(s, nn, PFV_LAMBDA(int64_t v) {
      const int64_t n = (int64_t)nd * (fp[v + 1] - fp[v]);
      a1[v] = n * (hp[v + 1] - hp[v]);  // n * nd * deg   (hp counts nd entries per cell)
      a2[v] = n * nd * (bp[v + 1] - bp[v]);
    });
    exclusive_scan<int64_t, int64_t>(s, c.scratch, sz1.p, c.node_eptr.p, (size_t)nn);
    exclusive_scan<int64_t, int64_t>(s, c.scratch, sz2.p, c.node_ebptr.p, (size_t)nn);
    const int64_t te = read_scalar<int64_t>(s, c.node_eptr.p + nn);
    const int64_t tb = read_scalar<int64_t>(s, c.node_ebptr.p + nn);
    c.Es.ensure(te + 1);
    c.Et.ensure(te + 1);
    c.Esb.ensure(tb + 1);
    c.Etb.ensure(tb + 1);
  }
  auto expand = [&](const CsrPattern& S, CsrPattern& V) { mpsa_expand_pattern(c, S, V); };
  // LDS need of the largest node of every block-size class (class maxima of nsf, deg and #boundary
  // faces never occur together, so sizing by them separately would overshoot the 160 KB budget)
  {
    Buf<int32_t> need;
    need.ensure(kNumClasses + 1);
    be_memset(need.p, 0, sizeof(int32_t) * (kNumClasses + 1), s);
    Buf<int32_t> bnd_dev;
    bnd_dev.ensure(kNumClasses);
    be_h2d(bnd_dev.p, kClassBounds, sizeof(int) * kNumClasses, s);
    const int32_t* hp = c.node_hptr;
    const int32_t* fp = c.node_fptr;
    const int32_t* bp = c.node_bptr;
    const int32_t* bd = bnd_dev;
    int32_t* nd_ = need;
    const int nclass = kNumClasses;
    const bool biot = c.biot_nalpha > 0;
    parallel_for(s, nn, PFV_LAMBDA(int64_t v) {
      const int nsf = fp[v + 1] - fp[v];
      if (nsf == 0) return;
      int cls = 0;
      while (cls < nclass - 1 && nsf > bd[cls]) ++cls;
      const size_t b = mpsa_lds_bytes(nsf, (hp[v + 1] - hp[v]) / nd, bp[v + 1] - bp[v], nd, biot);
      track_max_i32(nd_ + cls, (int)(b > 0x7fffffff ? 0x7fffffff : b));
      const size_t bw = mpsa_lds_bytes(nsf, (hp[v + 1] - hp[v]) / nd, bp[v + 1] - bp[v], nd, biot, sizeof(dd));
      track_max_i32(nd_ + nclass, (int)(bw > 0x7fffffff ? 0x7fffffff : bw));  // (any class: the wide body's scratch)
    });
    c.mpsa_class_lds.resize(kNumClasses + 1);
    be_d2h(c.mpsa_class_lds.data(), need.p, sizeof(int32_t) * (kNumClasses + 1), s);
  }
  expand(c.pat_flux, c.pat_stress);
  expand(c.pat_bound, c.pat_bstress);
  expand(c.pat_A, c.pat_Am);
  c.have_mpsa_symbolic = true;
}

// ---- stiffness contrast of every interaction region (VERDICT r5 item 1).  The condensed system adds the tractions of
// all sub-cells around a node into the same entries; when a stiff sub-cell sits between soft ones its own part is rank
// deficient (rigid rotation) and the rotation is fixed by the soft part, eps * contrast below the entry: FP64 keeps 1e-10
// of the reference up to a contrast of ~1e6 and degrades as eps * contrast beyond (DESIGN 8).  Scale of a cell = binary
// exponent of the largest diagonal entry of its stiffness matrix (lambda + 2 mu / mu in the isotropic case); a region is
// flagged when the exponents of its sub-cells differ by more than log2(PFV_MPSA_CONTRAST_LIMIT, default 1e6).  Flagged
// regions go to mpsa_wide_list (assembled and eliminated in double-double, mpsa_node_body<..., dd>); the count and the
// largest ratio go to pfv_stats (mpsa_contrast_regions, mpsa_max_contrast) whether or not the wide body is enabled.
// Ref: the columns the reference keeps apart, numerics/fv/mpsa.py:784-930.
static int64_t mpsa_contrast_scan(pfv_ctx_impl& c, const uint8_t* active) {
  stream_t s = c.stream;
  const int nd = c.nd;
  const int64_t nc = c.nc, nn = c.nn;
  const double* stiff = c.stiff;
  int32_t* ce = c.mpsa_cell_exp.ensure(std::max<int64_t>(nc, 1));
  parallel_for(s, nc, PFV_LAMBDA(int64_t cell) {
    double m = 0.0;
    for (int q = 0; q < 9; ++q) {
      const double x = fabs(stiff[((int64_t)q * 9 + q) * nc + cell]);
      m = (x > m && x < 1.0e300) ? x : m;
    }
    ce[cell] = m > 0.0 ? (int32_t)ilogb(m) : -100000;
  });
  const int limit_exp = std::max(1, (int)std::floor((double)env_int("PFV_MPSA_CONTRAST_LIMIT_LOG10", 6) * 3.321928094887362));
  uint8_t* flag = c.mpsa_wide_flag.ensure(std::max<int64_t>(nn, 1));
  int32_t* list = c.mpsa_wide_list.ensure(std::max<int64_t>(nn, 1));
  int32_t* stat = c.mpsa_wide_stat.ensure(4);
  be_memset(stat, 0, sizeof(int32_t) * 4, s);
  const int32_t* hp = c.node_hptr;
  const int32_t* hc = c.h_cell;
  parallel_for(s, nn, PFV_LAMBDA(int64_t v) {
    flag[v] = 0;
    if (active && !active[v]) return;
    const int h0 = hp[v], h1 = hp[v + 1];
    int lo = 1 << 30, hi = -(1 << 30);
    for (int h = h0; h < h1; h += nd) {
      const int e = ce[hc[h]];
      if (e <= -100000) continue;  // (a cell without stiffness: nothing to compare)
      lo = e < lo ? e : lo;
      hi = e > hi ? e : hi;
    }
    if (hi < lo) return;
    const int d = hi - lo;
    if (d > 0) atomic_max_i32(stat + 1, d);
    if (d > limit_exp) {
      flag[v] = (uint8_t)(d < 255 ? d : 255);  // (the exponent difference: the wide body scales its pivot threshold by it)
      list[atomic_fetch_add_i32(stat + 0, 1)] = (int32_t)v;
    }
  });
  int32_t sh[2];
  be_d2h(sh, stat, sizeof(sh), s);
  c.stats.mpsa_contrast_regions = sh[0];
  c.stats.mpsa_max_contrast = std::ldexp(1.0, sh[1]);
  return sh[0];
}

constexpr int kMpsaThreads = 512;
constexpr int kMpsaRedoWideDefault = 1;  // PFV_MPSA_REDO_WIDE (sliver fixture: 3.5e-12 -> 6.6e-15 against the reference)
static void mpsa_run_node_kernel(pfv_ctx_impl& c, const uint8_t* active = nullptr) {
  stream_t s = c.stream;
  const int nd = c.nd;
  be_memset(c.status.p, 0, sizeof(int32_t) * 4, s);
  MpsaArgs a;
  a.nd = nd; a.nc = c.nc; a.nf = c.nf; a.nn = c.nn; a.eta = c.mpsa_eta;
  a.order = c.node_order; a.hp = c.node_hptr; a.fp = c.node_fptr; a.node_sf = c.node_sf; a.node_face = c.node_face;
  a.sf_face = c.sf_face; a.fn_ptr = c.fn_ptr; a.nsides = c.face_nsides; a.h_cell = c.h_cell;
  a.bp = c.node_bptr; a.cell_nnodes = c.cell_nnodes; a.h_lf = c.h_lf; a.h_first = c.h_first;
  a.sub_bc = c.mpsa_subface_bc ? 1 : 0;
  a.nbc = c.mpsa_subface_bc ? c.nsf : c.nf;
  if (c.mpsa_subface_bc) {
    a.dirbits = c.bc_dirbits_sub; a.neubits = c.bc_neubits_sub;
    a.robbits = c.have_mpsa_robin_sub ? c.bc_robbits_sub.p : nullptr;
    a.robw = c.have_mpsa_robin_sub ? c.mpsa_robw_sub.p : nullptr;
  } else {
    a.dirbits = c.bc_dirbits; a.neubits = c.bc_neubits;
    a.robbits = c.have_mpsa_robin ? c.bc_robbits.p : nullptr;
    a.robw = c.have_mpsa_robin ? c.mpsa_robw.p : nullptr;
  }
  a.farea = c.farea; a.basis = c.mpsa_subface_bc ? (c.have_mpsa_basis_sub ? c.mpsa_basis_sub.p : nullptr) : (c.have_mpsa_basis ? c.mpsa_basis.p : nullptr); a.bls = c.node_bls; a.h_sgn = c.h_sgn;
  a.fnorm = c.fnorm; a.fcen = c.fcen; a.ccen = c.ccen; a.nodes = c.nodes; a.stiff = c.stiff;
  a.cvol = c.cvol; a.eptr = c.node_eptr; a.ebptr = c.node_ebptr;
  a.Es = c.Es; a.Et = c.Et; a.Esb = c.Esb; a.Etb = c.Etb; a.st = c.status;
  a.ablate = std::getenv("PFV_MPSA_ABLATE") ? std::atoi(std::getenv("PFV_MPSA_ABLATE")) : 0;
  a.active = active;
  a.lds_gj = std::getenv("PFV_MPSA_LDS_GJ") ? 1 : 0;
  a.refine = env_int("PFV_NODE_REFINE", 0);
  a.eta_sub = c.have_mpsa_eta_sub ? c.mpsa_eta_sub.p : nullptr;
  a.hf_eta = c.mpsa_hf_eta;
  a.hf_eta_sub = (c.mpsa_hf_on && c.have_mpsa_hf_eta_sub) ? c.mpsa_hf_eta_sub.p : nullptr;
  a.Et2 = a.Etb2 = nullptr;
  if (c.mpsa_hf_on) {
    if (c.biot_nalpha > 0)
      throw Error(PFV_ERR_UNSUPPORTED, "reconstruction_eta is not covered together with the Biot terms");
    const int64_t te = read_scalar<int64_t>(s, c.node_eptr.p + c.nn);
    const int64_t tb = read_scalar<int64_t>(s, c.node_ebptr.p + c.nn);
    a.Et2 = c.Et2.ensure(te + 1);
    a.Etb2 = c.Etb2.ensure(tb + 1);
  }
  a.nalpha = c.have_biot_symbolic ? c.biot_nalpha : 0;
  a.alpha = c.biot_alpha; a.dptr = c.node_dptr; a.dbptr = c.node_dbptr; a.cptr = c.node_cptr;
  a.tot_p = c.biot_tot_p; a.tot_d = c.biot_tot_d; a.tot_db = c.biot_tot_db; a.tot_c = c.biot_tot_c;
  a.Esp = c.bEsp; a.Etp = c.bEtp; a.DD = c.bDD; a.BDD = c.bBDD; a.CONS = c.bCONS;
  // Lean launches (see mpsa_node_body): whenever none of the special stages is asked for.  Nodes whose kappa wants
  // refinement are collected in a.redo and taken by one launch of the full body afterwards.
  const bool lean = a.eta_sub == nullptr && a.Et2 == nullptr && a.nalpha == 0 && a.refine == 0 &&
                    env_int("PFV_MPSA_LEAN", 1) != 0;
  a.redo = lean ? c.mpsa_redo.ensure(std::max<int64_t>(c.nn, 1)) : nullptr;
  a.nopivot = (lean && a.ablate == 0 && env_int("PFV_MPSA_GJ_NP", kMpsaNoPivotDefault) != 0) ? 1 : 0;
  // (the residual of a stable elimination grows with the size of the system: n = 108 against the 36 of the flow regions)
  a.np_tol = kNoPivotResidual * 3.0 * (double)env_int("PFV_MPSA_NP_TOLX", 1);
  // ---- regions of high stiffness contrast (mpsa_contrast_scan): counted always, handed to the double-double body
  // unless PFV_MPSA_DD=0
  const int64_t n_wide = mpsa_contrast_scan(c, active);
  const bool wide_on = n_wide > 0 && env_int("PFV_MPSA_DD", 1) != 0 && a.ablate == 0;
  a.wide = wide_on ? c.mpsa_wide_flag.p : nullptr;
  a.wide_exp = c.mpsa_wide_flag.p;  // (written for every node by the scan: 0 where the contrast stays below the limit)
  size_t lds_redo = 0;
  bool redo_global = false;
  // one launch per block-size class (LDS sized for the class)
  for (int cls = 0; cls < kNumClasses; ++cls) {
    const int64_t b0 = c.class_begin[cls], b1 = c.class_begin[cls + 1];
    if (b1 <= b0) continue;
    const size_t lds = (size_t)c.mpsa_class_lds[cls] + 64;
    if (lean) {
      const bool in_global_l = lds + 256 > 160 * 1024 || env_int("PFV_MPSA_GLOBAL_SCRATCH", 0) != 0;
      lds_redo = std::max(lds_redo, lds);
      redo_global = redo_global || in_global_l;
      if (in_global_l) {
        if (nd == 2) {
          if (a.basis) block_for_global<kMpsaThreads>(s, b1 - b0, lds, c.mpsa_scratch, PFV_LAMBDA(const WaveCtx& w) { mpsa_node_body<2, true, true>(a, w, b0); });
          else block_for_global<kMpsaThreads>(s, b1 - b0, lds, c.mpsa_scratch, PFV_LAMBDA(const WaveCtx& w) { mpsa_node_body<2, false, true>(a, w, b0); });
        } else {
          if (a.basis) block_for_global<kMpsaThreads>(s, b1 - b0, lds, c.mpsa_scratch, PFV_LAMBDA(const WaveCtx& w) { mpsa_node_body<3, true, true>(a, w, b0); });
          else block_for_global<kMpsaThreads>(s, b1 - b0, lds, c.mpsa_scratch, PFV_LAMBDA(const WaveCtx& w) { mpsa_node_body<3, false, true>(a, w, b0); });
        }
      } else if (nd == 2) {
        if (a.basis) block_for<kMpsaThreads>(s, b1 - b0, lds, PFV_LAMBDA(const WaveCtx& w) { mpsa_node_body<2, true, true>(a, w, b0); });
        else block_for<kMpsaThreads>(s, b1 - b0, lds, PFV_LAMBDA(const WaveCtx& w) { mpsa_node_body<2, false, true>(a, w, b0); });
      } else {
        if (a.basis) block_for<kMpsaThreads>(s, b1 - b0, lds, PFV_LAMBDA(const WaveCtx& w) { mpsa_node_body<3, true, true>(a, w, b0); });
        else block_for<kMpsaThreads>(s, b1 - b0, lds, PFV_LAMBDA(const WaveCtx& w) { mpsa_node_body<3, false, true>(a, w, b0); });
      }
      continue;
    }
    // interaction regions too large for the LDS (more than ~36 faces meet in a node of a 3-D grid: common in
    // unstructured tetrahedral meshes) work in global-memory scratch instead
    const bool in_global = lds + 256 > 160 * 1024 || env_int("PFV_MPSA_GLOBAL_SCRATCH", 0) != 0;
    if (in_global) {
      if (nd == 2) {
        if (a.basis) block_for_global<kMpsaThreads>(s, b1 - b0, lds, c.mpsa_scratch, PFV_LAMBDA(const WaveCtx& w) { mpsa_node_body<2, true>(a, w, b0); });
        else block_for_global<kMpsaThreads>(s, b1 - b0, lds, c.mpsa_scratch, PFV_LAMBDA(const WaveCtx& w) { mpsa_node_body<2, false>(a, w, b0); });
      } else {
        if (a.basis) block_for_global<kMpsaThreads>(s, b1 - b0, lds, c.mpsa_scratch, PFV_LAMBDA(const WaveCtx& w) { mpsa_node_body<3, true>(a, w, b0); });
        else block_for_global<kMpsaThreads>(s, b1 - b0, lds, c.mpsa_scratch, PFV_LAMBDA(const WaveCtx& w) { mpsa_node_body<3, false>(a, w, b0); });
      }
      continue;
    }
    if (nd == 2) {
      if (a.basis) block_for<kMpsaThreads>(s, b1 - b0, lds, PFV_LAMBDA(const WaveCtx& w) { mpsa_node_body<2, true>(a, w, b0); });
      else block_for<kMpsaThreads>(s, b1 - b0, lds, PFV_LAMBDA(const WaveCtx& w) { mpsa_node_body<2, false>(a, w, b0); });
    } else {
      if (a.basis) block_for<kMpsaThreads>(s, b1 - b0, lds, PFV_LAMBDA(const WaveCtx& w) { mpsa_node_body<3, true>(a, w, b0); });
      else block_for<kMpsaThreads>(s, b1 - b0, lds, PFV_LAMBDA(const WaveCtx& w) { mpsa_node_body<3, false>(a, w, b0); });
    }
  }
  int32_t sth[4];
  be_d2h(sth, c.status.p, sizeof(sth), s);
  // Regions the lean launches left (kappa asks for refinement: slivers; or the unpivoted elimination failed its check):
  // PFV_MPSA_REDO_WIDE=1 hands them to the double-double body instead of the FP64 body with iterative refinement -- 106
  // bits make a condition number of 1e7 harmless, and D^-1 / Omega are then exact to 31 digits where the FP64 body's
  // own rounding of them is what the refinement cannot repair (DESIGN 1.4).
  // (a launch that leaves more than a few per cent of its regions -- an input on which the unpivoted elimination fails its
  // check everywhere -- keeps the FP64 body: 1 us per region there against 6 us in the wide arithmetic)
  const bool redo_wide = lean && sth[2] > 0 && env_int("PFV_MPSA_REDO_WIDE", kMpsaRedoWideDefault) != 0 && a.ablate == 0 &&
                         env_int("PFV_MPSA_DD", 1) != 0 && (int64_t)sth[2] <= std::max<int64_t>(2000, c.nn / 50);
  if (redo_wide) {
    MpsaArgs a3 = a;
    a3.order = a.redo;
    a3.redo = nullptr;
    a3.nopivot = 0;
    a3.wide = nullptr;
    const int64_t nredo = sth[2];
    const int64_t z0 = 0;
    c.stats_mpsa_redo = nredo;
    c.stats.node_redo = nredo;
    const size_t lds_wide = (size_t)c.mpsa_class_lds[kNumClasses] + 64;
    if (nd == 2) block_for_global<kMpsaThreads>(s, nredo, lds_wide, c.mpsa_scratch, PFV_LAMBDA(const WaveCtx& w) { mpsa_node_body<2, true, false, dd>(a3, w, z0); });
    else block_for_global<kMpsaThreads>(s, nredo, lds_wide, c.mpsa_scratch, PFV_LAMBDA(const WaveCtx& w) { mpsa_node_body<3, true, false, dd>(a3, w, z0); });
    int32_t st2[4];
    be_d2h(st2, c.status.p, sizeof(st2), s);
    sth[0] = std::max(sth[0], st2[0]);
    sth[1] = std::max(sth[1], st2[1]);
  } else if (lean && sth[2] > 0) {
    // the nodes the lean launches left: the full body, in the scratch of the largest class
    MpsaArgs a2 = a;
    a2.order = a.redo;
    a2.redo = nullptr;
    const int64_t nredo = sth[2];
    const int64_t z0 = 0;
    c.stats_mpsa_redo = nredo;
    c.stats.node_redo = nredo;
    if (redo_global) {
      if (nd == 2) {
        if (a.basis) block_for_global<kMpsaThreads>(s, nredo, lds_redo, c.mpsa_scratch, PFV_LAMBDA(const WaveCtx& w) { mpsa_node_body<2, true>(a2, w, z0); });
        else block_for_global<kMpsaThreads>(s, nredo, lds_redo, c.mpsa_scratch, PFV_LAMBDA(const WaveCtx& w) { mpsa_node_body<2, false>(a2, w, z0); });
      } else {
        if (a.basis) block_for_global<kMpsaThreads>(s, nredo, lds_redo, c.mpsa_scratch, PFV_LAMBDA(const WaveCtx& w) { mpsa_node_body<3, true>(a2, w, z0); });
        else block_for_global<kMpsaThreads>(s, nredo, lds_redo, c.mpsa_scratch, PFV_LAMBDA(const WaveCtx& w) { mpsa_node_body<3, false>(a2, w, z0); });
      }
    } else if (nd == 2) {
      if (a.basis) block_for<kMpsaThreads>(s, nredo, lds_redo, PFV_LAMBDA(const WaveCtx& w) { mpsa_node_body<2, true>(a2, w, z0); });
      else block_for<kMpsaThreads>(s, nredo, lds_redo, PFV_LAMBDA(const WaveCtx& w) { mpsa_node_body<2, false>(a2, w, z0); });
    } else {
      if (a.basis) block_for<kMpsaThreads>(s, nredo, lds_redo, PFV_LAMBDA(const WaveCtx& w) { mpsa_node_body<3, true>(a2, w, z0); });
      else block_for<kMpsaThreads>(s, nredo, lds_redo, PFV_LAMBDA(const WaveCtx& w) { mpsa_node_body<3, false>(a2, w, z0); });
    }
    int32_t st2[4];
    be_d2h(st2, c.status.p, sizeof(st2), s);
    sth[0] = std::max(sth[0], st2[0]);
    sth[1] = std::max(sth[1], st2[1]);
  } else {
    c.stats_mpsa_redo = 0;
    c.stats.node_redo = 0;
  }
  if (wide_on) {
    // the flagged regions: full body in double-double arithmetic, one workgroup per region in global-memory scratch
    // (twice the bytes of the FP64 body + its own copies of the trace responses: beyond the LDS from n ~ 60 on)
    MpsaArgs a3 = a;
    a3.order = c.mpsa_wide_list.p;
    a3.redo = nullptr;
    a3.nopivot = 0;
    a3.wide = nullptr;
    const int64_t z0 = 0;
    const size_t lds_wide = (size_t)c.mpsa_class_lds[kNumClasses] + 64;
    if (nd == 2) block_for_global<kMpsaThreads>(s, n_wide, lds_wide, c.mpsa_scratch, PFV_LAMBDA(const WaveCtx& w) { mpsa_node_body<2, true, false, dd>(a3, w, z0); });
    else block_for_global<kMpsaThreads>(s, n_wide, lds_wide, c.mpsa_scratch, PFV_LAMBDA(const WaveCtx& w) { mpsa_node_body<3, true, false, dd>(a3, w, z0); });
    int32_t st3[4];
    be_d2h(st3, c.status.p, sizeof(st3), s);
    sth[0] = std::max(sth[0], st3[0]);
    sth[1] = std::max(sth[1], st3[1]);
  }
  if (a.ablate) return;
  if (sth[1]) throw Error(PFV_ERR_ARGUMENT, "every boundary component needs a Dirichlet or Neumann condition");
  if (sth[0])
    throw Error(PFV_ERR_SINGULAR, "Error in inversion of local linear systems (node " + std::to_string(sth[0] - 1) + ")");
}

// CSR values: every entry adds the expanded rows of the <= nodes(f) sub-faces of its face
// subset != nullptr: only the n_subset listed faces (partial discretization)
static void mpsa_run_face_kernel(pfv_ctx_impl& c, const int32_t* subset = nullptr, int64_t n_subset = 0) {
  stream_t s = c.stream;
  const int nd = c.nd;
  const int n2 = nd * nd;
  double* vs_ = c.val[PFV_MAT_STRESS].ensure(c.pat_stress.nnz);
  double* vt_ = c.val[PFV_MAT_BOUND_DISPLACEMENT_CELL].ensure(c.pat_stress.nnz);
  double* vsb = c.val[PFV_MAT_BOUND_STRESS].ensure(c.pat_bstress.nnz);
  double* vtb = c.val[PFV_MAT_BOUND_DISPLACEMENT_FACE].ensure(c.pat_bstress.nnz);
  const int32_t* fn_ptr = c.fn_ptr;
  const int32_t* fn_idx = c.fn_idx;
  const int32_t* ip = c.pat_flux.indptr;
  const int32_t* bip = c.pat_bound.indptr;
  const int32_t* bix = c.pat_bound.indices;
  const int32_t* hp = c.node_hptr;
  const int32_t* fp = c.node_fptr;
  const int32_t* bp = c.node_bptr;
  const int32_t* bfc = c.node_bfaces;
  const uint8_t* sf_ls = c.sf_ls;
  const uint8_t* colpairs = c.flux_colpairs;
  const int64_t cp_stride = c.cp_stride;
  const int64_t* eptr = c.node_eptr;
  const int64_t* ebptr = c.node_ebptr;
  const double* Es = c.Es;
  const double* Et = c.mpsa_hf_on ? c.Et2.p : c.Et.p;    // (reconstruction_eta: traces at the hf_eta points)
  const double* Esb = c.Esb;
  const double* Etb = c.mpsa_hf_on ? c.Etb2.p : c.Etb.p;
  const int32_t* order = subset ? subset : c.face_order.p;
  const int maxfn = std::max(c.max_face_nodes, 1);
  const size_t lds = (size_t)maxfn * 48 + 64;
  wave_for(s, subset ? n_subset : c.nf, lds, PFV_LAMBDA(const WaveCtx& w) {
    const int64_t f = order[w.item];
    const int a0 = fn_ptr[f], nnf = fn_ptr[f + 1] - a0;
    const int p0 = ip[f], len = ip[f + 1] - p0;
    const int q0 = bip[f], blen = bip[f + 1] - q0;
    const double inn = 1.0 / nnf;
    int64_t* baseE = reinterpret_cast<int64_t*>(w.lds);            // start of the node's expanded rows
    int64_t* baseB = baseE + maxfn;
    int32_t* meta = reinterpret_cast<int32_t*>(baseB + maxfn);     // [node]: ls, ncu, ncb, pair offset
    PFV_LANES(i, nnf) {
      const int v = fn_idx[a0 + i];
      baseE[i] = eptr[v];
      baseB[i] = ebptr[v];
      meta[4 * i + 0] = sf_ls[a0 + i];
      meta[4 * i + 1] = hp[v + 1] - hp[v];            // nd * deg
      meta[4 * i + 2] = nd * (bp[v + 1] - bp[v]);
    }
    w.sync();
    if (w.lane0()) {
      int m = 0;
      for (int i = 0; i < nnf; ++i) { meta[4 * i + 3] = m; m += meta[4 * i + 1] / nd; }
    }
    w.sync();
    const uint8_t* cp = colpairs + (cp_stride ? (int64_t)f * cp_stride : (int64_t)p0 * maxfn);
    for (int i = 0; i < nd; ++i) {
      const int64_t rowbase = (int64_t)p0 * n2 + (int64_t)i * nd * len;
      PFV_LANES(x, len * nd) {
        const int k = x / nd, aa = x - k * nd;
        double sv = 0.0, tv = 0.0;
        for (int t = 0; t < nnf; ++t) {
          const int e = cp[k * maxfn + t];
          if (e != 0xff) {
            const int j = e - meta[4 * t + 3];
            const int64_t off = baseE[t] + (int64_t)(nd * meta[4 * t] + i) * meta[4 * t + 1] + nd * j + aa;
            sv += Es[off];
            tv += Et[off];
          }
        }
        vs_[rowbase + x] = sv;
        vt_[rowbase + x] = tv * inn;
      }
      const int64_t browbase = (int64_t)q0 * n2 + (int64_t)i * nd * blen;
      PFV_LANES(x, blen * nd) {
        const int k = x / nd, aa = x - k * nd;
        const int fb = bix[q0 + k];
        double sv = 0.0, tv = 0.0;
        for (int t = 0; t < nnf; ++t) {
          const int v = fn_idx[a0 + t];
          const int b0 = bp[v], nb = bp[v + 1] - b0;
          const int bi = lower_bound_idx<int32_t>(bfc + b0, nb, fb);
          if (bi < nb && bfc[b0 + bi] == fb) {
            const int64_t off = baseB[t] + (int64_t)(nd * meta[4 * t] + i) * meta[4 * t + 2] + nd * bi + aa;
            sv += Esb[off];
            tv += Etb[off];
          }
        }
        vsb[browbase + x] = sv;
        vtb[browbase + x] = tv * inn;
      }
    }
  });
  c.filled[PFV_MAT_STRESS] = c.filled[PFV_MAT_BOUND_DISPLACEMENT_CELL] = true;
  c.filled[PFV_MAT_BOUND_STRESS] = c.filled[PFV_MAT_BOUND_DISPLACEMENT_FACE] = true;
}

// A_m = div_nd @ stress; row (cell, a) = sum over the faces of the cell of sgn * stress row (f, a)
// ---- conditions per sub-face (mpsa.py:712-720, 752-754, 780-781): stress and bound_stress keep one row
// block per sub-face (expansions of the MPFA sub-face patterns), bound_displacement_face keeps its face rows
// but gets one column block per boundary sub-face
static void mpsa_subface_symbolic(pfv_ctx_impl& c) {
  stream_t s = c.stream;
  const int64_t nf = c.nf, nsf = c.nsf;
  if (!c.have_sub_symbolic) build_subface_symbolic(c);
  mpsa_expand_pattern(c, c.pat_sflux, c.pat_sstress);
  mpsa_expand_pattern(c, c.pat_sbound, c.pat_sbstress);
  // (Nf x Nsf): row f = the boundary sub-faces of the nodes of f, ascending
  const int32_t* fn_ptr = c.fn_ptr;
  const int32_t* fn_idx = c.fn_idx;
  const int32_t* fp = c.node_fptr;
  const int32_t* bp = c.node_bptr;
  const int32_t* nsfid = c.node_sf;
  const uint8_t* bls = c.node_bls;
  Buf<int32_t> len;
  Buf<int64_t> ptr;
  int32_t* ln = len.ensure(nf + 1);
  ptr.ensure(nf + 1);
  parallel_for(s, nf, PFV_LAMBDA(int64_t f) {
    int m = 0;
    for (int e = fn_ptr[f]; e < fn_ptr[f + 1]; ++e) m += bp[fn_idx[e] + 1] - bp[fn_idx[e]];
    ln[f] = m;
  });
  exclusive_scan<int32_t, int64_t>(s, c.scratch, ln, ptr.p, (size_t)nf);
  finish_pattern(c, c.pat_bdf_s, ptr, nf, nsf);
  const int32_t* ip = c.pat_bdf_s.indptr;
  int32_t* ix = c.pat_bdf_s.indices;
  uint8_t* src = c.bdf_src.ensure(2 * std::max<int64_t>(c.pat_bdf_s.nnz, 1));
  int32_t* st = c.status.ensure(16);
  be_memset(st + 12, 0, sizeof(int32_t), s);
  parallel_for(s, nf, PFV_LAMBDA(int64_t f) {
    const int p0 = ip[f];
    int m = 0;
    for (int e = fn_ptr[f]; e < fn_ptr[f + 1]; ++e) {
      const int v = fn_idx[e];
      for (int i = 0; i < bp[v + 1] - bp[v]; ++i) {
        // insertion by global sub-face id (a handful of entries per row)
        const int id = nsfid[fp[v] + bls[bp[v] + i]];
        int q = m++;
        while (q > 0 && ix[p0 + q - 1] > id) {
          ix[p0 + q] = ix[p0 + q - 1];
          src[2 * (p0 + q)] = src[2 * (p0 + q - 1)];
          src[2 * (p0 + q) + 1] = src[2 * (p0 + q - 1) + 1];
          --q;
        }
        ix[p0 + q] = id;
        src[2 * (p0 + q)] = (uint8_t)(e - fn_ptr[f]);
        src[2 * (p0 + q) + 1] = (uint8_t)i;
      }
    }
    track_max_i32(st + 12, m);
  });
  c.pat_bdf_s.max_row = std::max(read_scalar<int32_t>(s, st + 12), 1);
  mpsa_expand_pattern(c, c.pat_bdf_s, c.pat_sbdface);
  c.have_mpsa_sub_symbolic = true;
}

// values of the three matrices that change shape (bound_displacement_cell keeps its face rows: the face kernel's)
static void mpsa_run_subface_kernel(pfv_ctx_impl& c) {
  stream_t s = c.stream;
  const int nd = c.nd, n2 = nd * nd;
  double* vs_ = c.val[PFV_MAT_STRESS].ensure(std::max<int64_t>(c.pat_sstress.nnz, 1));
  double* vsb = c.val[PFV_MAT_BOUND_STRESS].ensure(std::max<int64_t>(c.pat_sbstress.nnz, 1));
  double* vtb = c.val[PFV_MAT_BOUND_DISPLACEMENT_FACE].ensure(std::max<int64_t>(c.pat_sbdface.nnz, 1));
  const int32_t* fn_ptr = c.fn_ptr;
  const int32_t* fn_idx = c.fn_idx;
  const int32_t* hp = c.node_hptr;
  const int32_t* bp = c.node_bptr;
  const uint8_t* sf_ls = c.sf_ls;
  const int64_t* eptr = c.node_eptr;
  const int64_t* ebptr = c.node_ebptr;
  const double* Es = c.Es;
  const double* Esb = c.Esb;
  const double* Etb = c.mpsa_hf_on ? c.Etb2.p : c.Etb.p;  // (reconstruction_eta: traces at the hf_eta points)
  const int32_t* sip = c.pat_sflux.indptr;
  const int32_t* sbip = c.pat_sbound.indptr;
  // rows (sf, i): the node's expanded rows as they are (same column order: the node's cells / boundary sub-faces)
  wave_for<16>(s, c.nsf, 0, PFV_LAMBDA(const WaveCtx& w) {
    const int64_t sf = w.item;
    const int v = fn_idx[sf];
    const int ls = sf_ls[sf];
    const int ncu = hp[v + 1] - hp[v], ncb = nd * (bp[v + 1] - bp[v]);
    const int p0 = sip[sf], q0 = sbip[sf];
    for (int i = 0; i < nd; ++i) {
      const double* es = Es + eptr[v] + (int64_t)(nd * ls + i) * ncu;
      double* dst = vs_ + (int64_t)p0 * n2 + (int64_t)i * ncu;
      PFV_LANES(x, ncu) dst[x] = es[x];
      const double* eb = Esb + ebptr[v] + (int64_t)(nd * ls + i) * ncb;
      double* dstb = vsb + (int64_t)q0 * n2 + (int64_t)i * ncb;
      PFV_LANES(x, ncb) dstb[x] = eb[x];
    }
  });
  // bound_displacement_face: rows (f, i), every entry comes from one node of the face
  const int32_t* fip = c.pat_bdf_s.indptr;
  const uint8_t* src = c.bdf_src;
  wave_for<16>(s, c.nf, 0, PFV_LAMBDA(const WaveCtx& w) {
    const int64_t f = w.item;
    const int a0 = fn_ptr[f], nnf = fn_ptr[f + 1] - a0;
    const int p0 = fip[f], len = fip[f + 1] - p0;
    const double inn = 1.0 / nnf;
    for (int i = 0; i < nd; ++i) {
      double* dst = vtb + (int64_t)p0 * n2 + (int64_t)i * nd * len;
      PFV_LANES(x, len * nd) {
        const int k = x / nd, aa = x - k * nd;
        const int t = src[2 * (p0 + k)], bi = src[2 * (p0 + k) + 1];
        const int v = fn_idx[a0 + t];
        const int ncb = nd * (bp[v + 1] - bp[v]);
        dst[x] = inn * Etb[ebptr[v] + (int64_t)(nd * sf_ls[a0 + t] + i) * ncb + nd * bi + aa];
      }
    }
  });
  c.filled[PFV_MAT_STRESS] = c.filled[PFV_MAT_BOUND_STRESS] = c.filled[PFV_MAT_BOUND_DISPLACEMENT_FACE] = true;
}

static void mpsa_assemble_system(pfv_ctx_impl& c) {
  stream_t s = c.stream;
  const int nd = c.nd;
  const int64_t nc = c.nc;
  double* Aval = c.val[PFV_MAT_MECH_SYSTEM].ensure(c.pat_Am.nnz);
  double* diag = c.diag_m.ensure(nc * nd);
  const int32_t* cf_ptr = c.cf_ptr;
  const int32_t* cf_idx = c.cf_idx;
  const int8_t* cf_sgn = c.cf_sgn;
  const int32_t* sp = c.pat_stress.indptr;
  const int32_t* sx = c.pat_stress.indices;
  const int32_t* ap = c.pat_Am.indptr;
  const int32_t* ax = c.pat_Am.indices;
  const double* vs_ = c.val[PFV_MAT_STRESS];
  const int maxrow = std::max(c.pat_Am.max_row, 1);
#ifndef PFV_EMULATE
  // (as assemble_system in linalg.inc: the stress rows of all faces of the cell requested before any is used -- three
  // dependent round trips instead of three per face; same accumulation order, same bits)
  constexpr int kAsmFaces = 6, kAsmChunks = 4;
  if (c.max_cell_faces <= kAsmFaces && c.pat_stress.max_row <= 64 * kAsmChunks && env_int("PFV_ASM_PREFETCH", 1) != 0) {
    // positions kept under kept patterns, as assemble_system (linalg.inc) does for the flow system: a byte per (row, face,
    // stress entry) recorded by the first assembly under a key, replayed by the following ones -- no column indices of
    // stress (4.1 GB at configs[3]), no indices of A, no searches.  mode 0: search; 1: search and record; 2: replay.
    const int stride_f = 64 * kAsmChunks;
    const int64_t stride_r = (int64_t)std::max(c.max_cell_faces, 1) * stride_f;
    int mode = 0;
    if (env_int("PFV_ASM_POS", 1) != 0 && c.symb_key != 0 && c.pat_Am.max_row <= 255 &&
        (double)nc * nd * (double)stride_r <= 4.0e9) {
      if (c.asm_pos_m_key == c.symb_key && c.asm_pos_m_rows == nc * nd) {
        mode = 2;
      } else {
        c.asm_pos_m.ensure((size_t)(nc * nd * stride_r));
        c.asm_diagpos_m.ensure((size_t)(nc * nd));
        mode = 1;
      }
    }
    uint8_t* posb = c.asm_pos_m.p;
    uint8_t* dpos = c.asm_diagpos_m.p;
    auto body = [=] __device__(const WaveCtx& w, auto mode_c) {
      constexpr int MODE = decltype(mode_c)::value;
      const int64_t row = w.item;
      const int64_t cell = row / nd;
      const int comp = (int)(row - cell * nd);
      const int r0 = ap[row], alen = ap[row + 1] - r0;
      double* acc = reinterpret_cast<double*>(w.lds);
      int32_t* aidx = reinterpret_cast<int32_t*>(acc + maxrow);
      const int e0 = cf_ptr[cell], ne = cf_ptr[cell + 1] - e0;
      int mp0 = 0, mlen = 0;
      double msg = 0.0;
      if (w.lane < ne) {
        const int64_t srow = (int64_t)cf_idx[e0 + w.lane] * nd + comp;
        msg = (double)cf_sgn[e0 + w.lane];
        mp0 = sp[srow];
        mlen = sp[srow + 1] - mp0;
      }
      PFV_LANES(i, alen) {
        if (MODE != 2) aidx[i] = ax[r0 + i];
        acc[i] = 0.0;
      }
      int cj[kAsmFaces][kAsmChunks];
      double v[kAsmFaces][kAsmChunks];
      uint8_t* mypos = posb + row * stride_r;
#pragma unroll
      for (int e = 0; e < kAsmFaces; ++e) {
        const int p0 = __shfl(mp0, e, 64), len = __shfl(mlen, e, 64);
#pragma unroll
        for (int u = 0; u < kAsmChunks; ++u) {
          const int k = u * 64 + w.lane;
          const bool live = k < len;
          if (MODE == 2) cj[e][u] = live ? (int)mypos[e * stride_f + k] : -1;
          else cj[e][u] = live ? sx[p0 + k] : -1;
          v[e][u] = live ? vs_[p0 + k] : 0.0;
        }
      }
      w.lsync();
#pragma unroll
      for (int e = 0; e < kAsmFaces; ++e) {
        const double sg = __shfl(msg, e, 64);
#pragma unroll
        for (int u = 0; u < kAsmChunks; ++u) {
          if (cj[e][u] >= 0) {
            const int pos = MODE == 2 ? cj[e][u] : lower_bound_idx<int32_t>(aidx, alen, cj[e][u]);
            if (MODE == 1) mypos[e * stride_f + u * 64 + w.lane] = (uint8_t)pos;
            acc[pos] += sg * v[e][u];
          }
        }
        w.lsync();
      }
      const int dp = MODE == 2 ? (int)dpos[row] : -1;
      PFV_LANES(i, alen) {
        Aval[r0 + i] = acc[i];
        const bool is_diag = MODE == 2 ? (i == dp) : (aidx[i] == (int32_t)row);
        if (is_diag) {
          diag[row] = acc[i];
          if (MODE == 1) dpos[row] = (uint8_t)i;
        }
      }
      w.lsync();
    };
    using M0 = std::integral_constant<int, 0>;
    using M1 = std::integral_constant<int, 1>;
    using M2 = std::integral_constant<int, 2>;
    const size_t ldsb = (size_t)maxrow * 12 + 32;
    if (mode == 2) wave_for(s, nc * nd, ldsb, [=] __device__(const WaveCtx& w) { body(w, M2{}); });
    else if (mode == 1) wave_for(s, nc * nd, ldsb, [=] __device__(const WaveCtx& w) { body(w, M1{}); });
    else wave_for(s, nc * nd, ldsb, [=] __device__(const WaveCtx& w) { body(w, M0{}); });
    if (mode == 1) {
      c.asm_pos_m_key = c.symb_key;
      c.asm_pos_m_rows = nc * nd;
    }
    c.stats.assemble_positions_kept = mode == 2 ? 1 : 0;
    c.filled[PFV_MAT_MECH_SYSTEM] = true;
    return;
  }
#endif
  wave_for(s, nc * nd, (size_t)maxrow * 12 + 32, PFV_LAMBDA(const WaveCtx& w) {
    const int64_t row = w.item;
    const int64_t cell = row / nd;
    const int comp = (int)(row - cell * nd);
    const int r0 = ap[row], alen = ap[row + 1] - r0;
    double* acc = reinterpret_cast<double*>(w.lds);
    int32_t* aidx = reinterpret_cast<int32_t*>(acc + maxrow);
    PFV_LANES(i, alen) {
      aidx[i] = ax[r0 + i];
      acc[i] = 0.0;
    }
    w.sync();
    for (int e = cf_ptr[cell]; e < cf_ptr[cell + 1]; ++e) {
      const int64_t srow = (int64_t)cf_idx[e] * nd + comp;
      const double sg = (double)cf_sgn[e];
      const int p0 = sp[srow], len = sp[srow + 1] - p0;
      PFV_LANES(i, len) {
        const int pos = lower_bound_idx<int32_t>(aidx, alen, sx[p0 + i]);
        acc[pos] += sg * vs_[p0 + i];
      }
      w.sync();
    }
    PFV_LANES(i, alen) {
      Aval[r0 + i] = acc[i];
      if (aidx[i] == (int32_t)row) diag[row] = acc[i];
    }
  });
  c.filled[PFV_MAT_MECH_SYSTEM] = true;
}

static void mpsa_assemble_rhs(pfv_ctx_impl& c, const double* d_bc, const double* d_src) {
  stream_t s = c.stream;
  const int nd = c.nd;
  const int64_t nc = c.nc, nf = c.nf;
  double* ft = c.face_tmp.ensure(nf * nd);
  spmv(c, c.pat_bstress, c.val[PFV_MAT_BOUND_STRESS], d_bc, ft);
  double* b = c.rhs_m.ensure(nc * nd);
  const int32_t* cf_ptr = c.cf_ptr;
  const int32_t* cf_idx = c.cf_idx;
  const int8_t* cf_sgn = c.cf_sgn;
  parallel_for(s, nc * nd, PFV_LAMBDA(int64_t row) {
    const int64_t cell = row / nd;
    const int comp = (int)(row - cell * nd);
    double acc = d_src ? d_src[row] : 0.0;
    for (int e = cf_ptr[cell]; e < cf_ptr[cell + 1]; ++e)
      acc -= (double)cf_sgn[e] * ft[(int64_t)cf_idx[e] * nd + comp];
    b[row] = acc;
  });
}

}  // namespace pfv
