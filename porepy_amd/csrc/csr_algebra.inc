// csr_algebra.inc — device-resident CSR matrices and the sparse algebra of the step after discretize (SURVEY §8 row N4).
//
// The reference turns discretization matrices into equations on the host: MergedOperator.parse concatenates the
// matrices of the subdomains block-diagonally (numerics/ad/ad_utils.py:597-663 ->
// matrix_operations.csr_matrix_from_sparse_blocks), the operator tree multiplies the result with projections,
// divergences and diagonal scalings and adds the pieces up (scipy csr @ / + in ad/operators.py, assembled by
// EquationSystem.assemble, equation_system.py:1579).  A pfv_csr keeps such a matrix in HBM: created from a
// discretization matrix of a handle (device-to-device, the 21 GB of a 2 M-cell discretization never cross PCIe) or
// uploaded once (projections, divergence), combined by the kernels below, handed to pfv_solve as the active system.
//
// Conventions follow scipy so that results can be compared entry by entry:
//   * rows sorted by column, no duplicates (inputs are required to be in that form: scipy's canonical format);
//   * products and sums accumulate in the order scipy's csr_matmat / csr_binop do (ascending position in the row of the
//     left factor; left operand before right operand) with every product rounded on its own -- same bits;
//   * entries whose computed value is exactly zero are not stored (scipy drops them in both kernels).
// Portable bodies (backend.h): the host emulation runs the same code in the CPU tests.

struct pfv_csr {
  pfv_ctx* h = nullptr;
  pfv::CsrPattern P;
  pfv::Buf<double> val;
};

namespace pfv {

constexpr int kSpgemmMaxRow = 4096;  // products feeding one row of A B that are sorted in LDS (longer rows: global sorts)

static void csr_check_sorted(pfv_ctx_impl& c, const CsrPattern& P, const char* what) {
  stream_t s = c.stream;
  const int32_t* ip = P.indptr;
  const int32_t* ix = P.indices;
  const int64_t ncols = P.ncols;
  int32_t* st = c.status.ensure(16);
  be_memset(st + 12, 0, sizeof(int32_t), s);
  parallel_for(s, P.nrows, PFV_LAMBDA(int64_t r) {
    bool bad = ip[r + 1] < ip[r];
    for (int e = ip[r]; e < ip[r + 1]; ++e) {
      if (ix[e] < 0 || ix[e] >= ncols) bad = true;
      if (e > ip[r] && ix[e] <= ix[e - 1]) bad = true;
    }
    if (bad) atomic_max_i32(st + 12, 1);
  });
  if (read_scalar<int32_t>(s, st + 12))
    throw Error(PFV_ERR_ARGUMENT, std::string(what) + ": rows must be sorted by column without duplicates, indices in range");
}

// C = blockdiag(B_0, ..., B_{n-1})   (MergedOperator.parse)
static void csr_block_diag(pfv_ctx_impl& c, int n, const pfv_csr* const* blocks, pfv_csr& out) {
  stream_t s = c.stream;
  int64_t nr = 0, ncl = 0, nnz = 0;
  int mr = 0;
  for (int b = 0; b < n; ++b) {
    nr += blocks[b]->P.nrows;
    ncl += blocks[b]->P.ncols;
    nnz += blocks[b]->P.nnz;
    mr = std::max(mr, blocks[b]->P.max_row);
  }
  if (nnz >= (int64_t(1) << 31) || ncl >= (int64_t(1) << 31))
    throw Error(PFV_ERR_UNSUPPORTED, "block diagonal: more than 2^31 entries or columns");
  out.P.nrows = nr;
  out.P.ncols = ncl;
  out.P.nnz = nnz;
  out.P.max_row = mr;
  int32_t* op = out.P.indptr.ensure((size_t)nr + 1);
  int32_t* ox = out.P.indices.ensure((size_t)std::max<int64_t>(nnz, 1));
  double* ov = out.val.ensure((size_t)std::max<int64_t>(nnz, 1));
  int64_t r0 = 0, c0 = 0, e0 = 0;
  for (int b = 0; b < n; ++b) {
    const CsrPattern& B = blocks[b]->P;
    const int32_t* bp = B.indptr;
    const int32_t* bx = B.indices;
    const double* bv = blocks[b]->val;
    const int64_t rr = r0, cc = c0, ee = e0;
    parallel_for(s, B.nrows + (b + 1 == n ? 1 : 0), PFV_LAMBDA(int64_t r) { op[rr + r] = (int32_t)(ee + bp[r]); });
    parallel_for(s, B.nnz, PFV_LAMBDA(int64_t e) {
      ox[ee + e] = (int32_t)(cc + bx[e]);
      ov[ee + e] = bv[e];
    });
    r0 += B.nrows;
    c0 += B.ncols;
    e0 += B.nnz;
  }
  if (n == 0) be_memset(op, 0, sizeof(int32_t), s);
}

// C = A B.  One lane group per row of A: the products a_ik b_kj are gathered in the order of scipy's csr_matmat (k in
// the row's storage order, j in the storage order of row k of B), sorted by (column, gather position) with a bitonic
// network in LDS, every run of equal columns summed in gather order; exact zeros are dropped.
static void csr_spgemm(pfv_ctx_impl& c, const pfv_csr& A, const pfv_csr& B, pfv_csr& out) {
  stream_t s = c.stream;
  if (A.P.ncols != B.P.nrows) throw Error(PFV_ERR_ARGUMENT, "matrix product: inner dimensions differ");
  const int64_t n = A.P.nrows;
  const int32_t* ap = A.P.indptr;
  const int32_t* ax = A.P.indices;
  const double* av = A.val;
  const int32_t* bp = B.P.indptr;
  const int32_t* bx = B.P.indices;
  const double* bv = B.val;
  Buf<int32_t> cap_, cnt_, tcol_;
  Buf<int64_t> tptr_, cptr_;
  Buf<double> tval_;
  int32_t* cap = cap_.ensure((size_t)n + 1);
  int32_t* cnt = cnt_.ensure((size_t)n + 1);
  int64_t* tptr = tptr_.ensure((size_t)n + 1);
  int64_t* cptr = cptr_.ensure((size_t)n + 1);
  int32_t* st = c.status.ensure(16);
  be_memset(st + 8, 0, sizeof(int32_t) * 2, s);
  parallel_for(s, n, PFV_LAMBDA(int64_t r) {
    int64_t m = 0;  // (products feeding the row: summed in 64 bits, a row beyond 2^31 - 1 is refused below)
    for (int e = ap[r]; e < ap[r + 1]; ++e) m += bp[ax[e] + 1] - bp[ax[e]];
    const int mc = m > 2147483647LL ? 2147483647 : (int)m;
    cap[r] = mc;
    track_max_i32(st + 8, mc);
  });
  exclusive_scan<int32_t, int64_t>(s, c.scratch, cap, tptr, (size_t)n);
  const int maxcap = read_scalar<int32_t>(s, st + 8);
  if (maxcap == 2147483647) throw Error(PFV_ERR_UNSUPPORTED, "sparse product: a row is fed by 2^31 or more products");
  const int64_t ttot = read_scalar<int64_t>(s, tptr + n);
  // LDS path: keys + values + run masks of the longest row must fit the workgroup's share of the LDS of THIS device
  // (160 KB on gfx950; 64 KB parts take the global-sort path from ~2600 products per row on)
#ifdef PFV_EMULATE
  size_t lds_limit = 160 * 1024;  // (the host emulation stands for gfx950: it selects the path the product takes there)
#else
  size_t lds_limit = 64 * 1024;
  {
    int smem = 0;
    if (hipDeviceGetAttribute(&smem, hipDeviceAttributeMaxSharedMemoryPerBlock, c.device) == hipSuccess && smem > 0)
      lds_limit = (size_t)smem;
  }
#endif
  size_t lds_need = 0;
  {
    int capP_ = 2;
    while (capP_ < std::max<int64_t>(maxcap, 1)) capP_ <<= 1;
    lds_need = 8 * (size_t)capP_ + 8 * (size_t)std::max<int64_t>(maxcap, 1) + 8 * (size_t)(capP_ / 64 + 1) + 64;
  }
  if (maxcap > kSpgemmMaxRow || lds_need + 256 > lds_limit || env_int("PFV_SPGEMM_GENERIC", 0) != 0) {
    c.stats.spgemm_path = 1;
    c.stats.spgemm_lds_bytes = 0;
    // Rows too long for the LDS sort: all products as (row, column, value) triplets in gather order, two stable radix
    // sorts (by column, then by row) leave them grouped by (row, column) with the gather order kept inside every group,
    // every group summed in that order by the thread of its first element -- the same sums, slower.
    if (ttot >= (int64_t(1) << 31)) throw Error(PFV_ERR_UNSUPPORTED, "matrix product: more than 2^31 products");
    Buf<uint32_t> k1_, k2_, ko_;
    Buf<int32_t> v1_, v2_, v3_, keep_;
    Buf<int64_t> pos_;
    Buf<double> pv_, sv_;
    const size_t T = (size_t)std::max<int64_t>(ttot, 1);
    uint32_t* kcol = k1_.ensure(T);
    uint32_t* krow = k2_.ensure(T);
    uint32_t* kout = ko_.ensure(T);
    int32_t* idx = v1_.ensure(T);
    int32_t* p1 = v2_.ensure(T);
    int32_t* p2 = v3_.ensure(T);
    double* pv = pv_.ensure(T);
    wave_for<16>(s, n, 16, PFV_LAMBDA(const WaveCtx& w) {
      const int64_t r = w.item;
      int64_t o = tptr[r];
      for (int e = ap[r]; e < ap[r + 1]; ++e) {
        const int k = ax[e];
        const double a = av[e];
        const int p0 = bp[k], len = bp[k + 1] - p0;
        PFV_LANES(t, len) {
          kcol[o + t] = (uint32_t)bx[p0 + t];
          krow[o + t] = (uint32_t)r;
          pv[o + t] = a * bv[p0 + t];
          idx[o + t] = (int32_t)(o + t);
        }
        o += len;
      }
    });
    int cbits = 1, rbits = 1;
    while ((int64_t(1) << cbits) < B.P.ncols) ++cbits;
    while ((int64_t(1) << rbits) < n) ++rbits;
    sort_pairs(s, c.scratch, kcol, kout, idx, p1, (size_t)ttot, cbits);
    uint32_t* krow_perm = kout;  // (reuse: the sorted column keys are not needed, the columns are read through the permutation)
    parallel_for(s, ttot, PFV_LAMBDA(int64_t q) { krow_perm[q] = krow[p1[q]]; });
    uint32_t* rsorted = krow;    // (its old content has just been copied out)
    sort_pairs(s, c.scratch, krow_perm, rsorted, p1, p2, (size_t)ttot, rbits);
    int32_t* keep = keep_.ensure(T + 1);
    int64_t* pos = pos_.ensure(T + 1);
    double* sv = sv_.ensure(T);
    parallel_for(s, ttot, PFV_LAMBDA(int64_t q) {
      const int e = p2[q];
      const uint32_t row = rsorted[q], col = kcol[e];
      const bool head = q == 0 || rsorted[q - 1] != row || kcol[p2[q - 1]] != col;
      int kp = 0;
      if (head) {
        double sum = pv[e];
        for (int64_t t = q + 1; t < ttot && rsorted[t] == row && kcol[p2[t]] == col; ++t) sum += pv[p2[t]];
        sv[q] = sum;
        kp = sum != 0.0 ? 1 : 0;
      }
      keep[q] = kp;
    });
    exclusive_scan<int32_t, int64_t>(s, c.scratch, keep, pos, (size_t)ttot);
    const int64_t nnz = read_scalar<int64_t>(s, pos + ttot);
    out.P.nrows = n;
    out.P.ncols = B.P.ncols;
    out.P.nnz = nnz;
    int32_t* cp = out.P.indptr.ensure((size_t)n + 1);
    int32_t* cx = out.P.indices.ensure((size_t)std::max<int64_t>(nnz, 1));
    double* cv = out.val.ensure((size_t)std::max<int64_t>(nnz, 1));
    parallel_for(s, n + 1, PFV_LAMBDA(int64_t r) {
      cp[r] = (int32_t)pos[lower_bound_idx<uint32_t>(rsorted, (int)ttot, (uint32_t)r)];
    });
    parallel_for(s, ttot, PFV_LAMBDA(int64_t q) {
      if (keep[q]) {
        cx[pos[q]] = (int32_t)kcol[p2[q]];
        cv[pos[q]] = sv[q];
      }
    });
    be_memset(st + 8, 0, sizeof(int32_t), s);
    parallel_for(s, n, PFV_LAMBDA(int64_t r) { track_max_i32(st + 8, cp[r + 1] - cp[r]); });
    out.P.max_row = read_scalar<int32_t>(s, st + 8);
    be_sync(s);
    return;
  }
  int32_t* tcol = tcol_.ensure((size_t)std::max<int64_t>(ttot, 1));
  double* tval = tval_.ensure((size_t)std::max<int64_t>(ttot, 1));
  const int capL = std::max(maxcap, 1);
  const int G = capL <= 64 ? 16 : (capL <= 160 ? 32 : 64);
  int capP = 2;
  while (capP < capL) capP <<= 1;
  const int nw = capP / 64 + 1;
  const size_t lds = 8 * (size_t)capP + 8 * (size_t)capL + 8 * (size_t)nw + 64;
  c.stats.spgemm_path = G;  // (what the launch below takes: wave_for rounds the row's share up to 16 bytes, 64 / G rows a block)
  c.stats.spgemm_lds_bytes = (int64_t)(((lds + 15) & ~size_t(15)) * (size_t)(64 / G));
  wave_for_g(G, s, n, lds, PFV_LAMBDA(const WaveCtx& w) {
    const int64_t r = w.item;
    unsigned long long* key = reinterpret_cast<unsigned long long*>(w.lds);
    double* v0 = reinterpret_cast<double*>(key + capP);
    unsigned long long* mask = reinterpret_cast<unsigned long long*>(v0 + capL);
    int m = 0;
    for (int e = ap[r]; e < ap[r + 1]; ++e) {
      const int k = ax[e];
      const double a = av[e];
      const int p0 = bp[k], len = bp[k + 1] - p0;
      PFV_LANES(t, len) {
        key[m + t] = ((unsigned long long)(unsigned)bx[p0 + t] << 32) | (unsigned)(m + t);
        v0[m + t] = a * bv[p0 + t];
      }
      m += len;
    }
    int P2 = 2;
    while (P2 < m) P2 <<= 1;
    PFV_LANES(t, P2 - m) key[m + t] = ~0ull;
    PFV_LANES(i, P2 / 64 + 1) mask[i] = 0ull;
    w.sync();
    for (int k = 2; k <= P2; k <<= 1) {
      for (int j = k >> 1; j > 0; j >>= 1) {
        PFV_LANES(t, P2 >> 1) {
          const int lo = ((t & ~(j - 1)) << 1) | (t & (j - 1));
          const int hi = lo | j;
          const bool up = (lo & k) == 0;
          const unsigned long long x = key[lo], y = key[hi];
          if ((x > y) == up) {
            key[lo] = y;
            key[hi] = x;
          }
        }
        w.sync();
      }
    }
    // heads of runs whose sum is not exactly zero
    PFV_LANES(e, m) {
      if (e == 0 || (key[e] >> 32) != (key[e - 1] >> 32)) {
        const unsigned long long kc = key[e] >> 32;
        double sum = v0[(unsigned)key[e]];
        for (int t = e + 1; t < m && (key[t] >> 32) == kc; ++t) sum += v0[(unsigned)key[t]];  // gather order
        if (sum != 0.0) atomic_or_u64(mask + (e >> 6), 1ull << (e & 63));
      }
    }
    w.sync();
    int total = 0;
    for (int i = 0; i < m / 64 + 1; ++i) total += popcount64(mask[i]);
    const int64_t t0 = tptr[r];
    PFV_LANES(e, m) {
      const unsigned long long word = mask[e >> 6];
      if ((word >> (e & 63)) & 1ull) {
        int posn = popcount64(word & ((1ull << (e & 63)) - 1ull));
        for (int i = 0; i < (e >> 6); ++i) posn += popcount64(mask[i]);
        const unsigned long long kc = key[e] >> 32;
        double sum = v0[(unsigned)key[e]];
        for (int t = e + 1; t < m && (key[t] >> 32) == kc; ++t) sum += v0[(unsigned)key[t]];
        tcol[t0 + posn] = (int32_t)kc;
        tval[t0 + posn] = sum;
      }
    }
    if (w.lane0()) cnt[r] = total;
    w.sync();
  });
  exclusive_scan<int32_t, int64_t>(s, c.scratch, cnt, cptr, (size_t)n);
  const int64_t nnz = read_scalar<int64_t>(s, cptr + n);
  if (nnz >= (int64_t(1) << 31)) throw Error(PFV_ERR_UNSUPPORTED, "matrix product: more than 2^31 entries");
  out.P.nrows = n;
  out.P.ncols = B.P.ncols;
  out.P.nnz = nnz;
  out.P.max_row = maxcap;
  int32_t* cp = out.P.indptr.ensure((size_t)n + 1);
  int32_t* cx = out.P.indices.ensure((size_t)std::max<int64_t>(nnz, 1));
  double* cv = out.val.ensure((size_t)std::max<int64_t>(nnz, 1));
  parallel_for(s, n + 1, PFV_LAMBDA(int64_t r) { cp[r] = (int32_t)cptr[r]; });
  wave_for<16>(s, n, 16, PFV_LAMBDA(const WaveCtx& w) {
    const int64_t r = w.item;
    const int64_t t0 = tptr[r], o = cptr[r];
    PFV_LANES(t, cnt[r]) {
      cx[o + t] = tcol[t0 + t];
      cv[o + t] = tval[t0 + t];
    }
  });
  be_sync(s);  // (the scratch buffers above die with this scope)
}

// C = alpha A + beta B, merged row by row; exact zeros are dropped (scipy's csr_binop_csr_canonical)
static void csr_axpby(pfv_ctx_impl& c, double alpha, const pfv_csr& A, double beta, const pfv_csr& B, pfv_csr& out) {
  stream_t s = c.stream;
  if (A.P.nrows != B.P.nrows || A.P.ncols != B.P.ncols) throw Error(PFV_ERR_ARGUMENT, "matrix sum: shapes differ");
  const int64_t n = A.P.nrows;
  const int32_t* ap = A.P.indptr;
  const int32_t* ax = A.P.indices;
  const double* av = A.val;
  const int32_t* bp = B.P.indptr;
  const int32_t* bx = B.P.indices;
  const double* bv = B.val;
  Buf<int32_t> cnt_;
  Buf<int64_t> cptr_;
  int32_t* cnt = cnt_.ensure((size_t)n + 1);
  int64_t* cptr = cptr_.ensure((size_t)n + 1);
  int32_t* st = c.status.ensure(16);
  be_memset(st + 8, 0, sizeof(int32_t) * 2, s);
  for (int pass = 0; pass < 2; ++pass) {
    int32_t* cx = pass ? out.P.indices.p : nullptr;
    double* cv = pass ? out.val.p : nullptr;
    parallel_for(s, n, PFV_LAMBDA(int64_t r) {
#ifdef __clang__
#pragma clang fp contract(off)  // alpha a + beta b as scipy computes it: two rounded products, one rounded sum
#endif
      int i = ap[r], j = bp[r];
      const int ie = ap[r + 1], je = bp[r + 1];
      int m = 0;
      int64_t o = pass ? cptr[r] : 0;
      while (i < ie || j < je) {
        const int ca = i < ie ? ax[i] : 0x7fffffff, cb = j < je ? bx[j] : 0x7fffffff;
        double v;
        int col;
        if (ca == cb) {
          v = alpha * av[i] + beta * bv[j];
          col = ca;
          ++i;
          ++j;
        } else if (ca < cb) {
          v = alpha * av[i];
          col = ca;
          ++i;
        } else {
          v = beta * bv[j];
          col = cb;
          ++j;
        }
        if (v != 0.0) {
          if (pass) {
            cx[o + m] = col;
            cv[o + m] = v;
          }
          ++m;
        }
      }
      if (!pass) {
        cnt[r] = m;
        track_max_i32(st + 8, m);
      }
    });
    if (!pass) {
      exclusive_scan<int32_t, int64_t>(s, c.scratch, cnt, cptr, (size_t)n);
      const int64_t nnz = read_scalar<int64_t>(s, cptr + n);
      if (nnz >= (int64_t(1) << 31)) throw Error(PFV_ERR_UNSUPPORTED, "matrix sum: more than 2^31 entries");
      out.P.nrows = n;
      out.P.ncols = A.P.ncols;
      out.P.nnz = nnz;
      out.P.max_row = read_scalar<int32_t>(s, st + 8);
      int32_t* cp = out.P.indptr.ensure((size_t)n + 1);
      out.P.indices.ensure((size_t)std::max<int64_t>(nnz, 1));
      out.val.ensure((size_t)std::max<int64_t>(nnz, 1));
      parallel_for(s, n + 1, PFV_LAMBDA(int64_t r) { cp[r] = (int32_t)cptr[r]; });
    }
  }
  be_sync(s);
}

// C = A^T: stable radix sort of the entries by column keeps them in row order inside every column, i.e. the rows of
// the transpose come out sorted (what scipy's tocsc / transpose().tocsr() yields)
static void csr_transpose(pfv_ctx_impl& c, const pfv_csr& A, pfv_csr& out) {
  stream_t s = c.stream;
  const int64_t nr = A.P.nrows, ncl = A.P.ncols, nnz = A.P.nnz;
  const int32_t* ap = A.P.indptr;
  const int32_t* ax = A.P.indices;
  const double* av = A.val;
  Buf<uint32_t> kin_, kout_;
  Buf<int32_t> vin_, vout_, rowof_;
  uint32_t* kin = kin_.ensure((size_t)std::max<int64_t>(nnz, 1));
  uint32_t* kout = kout_.ensure((size_t)std::max<int64_t>(nnz, 1));
  int32_t* vin = vin_.ensure((size_t)std::max<int64_t>(nnz, 1));
  int32_t* vout = vout_.ensure((size_t)std::max<int64_t>(nnz, 1));
  int32_t* rowof = rowof_.ensure((size_t)std::max<int64_t>(nnz, 1));
  wave_for<16>(s, nr, 16, PFV_LAMBDA(const WaveCtx& w) {
    const int64_t r = w.item;
    const int p0 = ap[r], len = ap[r + 1] - p0;
    PFV_LANES(t, len) {
      rowof[p0 + t] = (int32_t)r;
      kin[p0 + t] = (uint32_t)ax[p0 + t];
      vin[p0 + t] = p0 + t;
    }
  });
  int bits = 1;
  while ((int64_t(1) << bits) < ncl) ++bits;
  sort_pairs(s, c.scratch, kin, kout, vin, vout, (size_t)nnz, bits);
  out.P.nrows = ncl;
  out.P.ncols = nr;
  out.P.nnz = nnz;
  int32_t* op = out.P.indptr.ensure((size_t)ncl + 1);
  int32_t* ox = out.P.indices.ensure((size_t)std::max<int64_t>(nnz, 1));
  double* ov = out.val.ensure((size_t)std::max<int64_t>(nnz, 1));
  parallel_for(s, ncl + 1, PFV_LAMBDA(int64_t col) { op[col] = (int32_t)lower_bound_idx<uint32_t>(kout, (int)nnz, (uint32_t)col); });
  parallel_for(s, nnz, PFV_LAMBDA(int64_t q) {
    const int e = vout[q];
    ox[q] = rowof[e];
    ov[q] = av[e];
  });
  int32_t* st = c.status.ensure(16);
  be_memset(st + 8, 0, sizeof(int32_t), s);
  parallel_for(s, ncl, PFV_LAMBDA(int64_t col) { track_max_i32(st + 8, op[col + 1] - op[col]); });
  out.P.max_row = read_scalar<int32_t>(s, st + 8);
  be_sync(s);
}

// C = [[B_00, B_01, ...], [B_10, ...], ...]: block matrix from a grid of blocks (scipy.sparse.bmat; what stacking the
// equations of several variables amounts to in EquationSystem.assemble).  Missing blocks are zero; the block rows /
// columns take their sizes from the blocks present (row_sizes / col_sizes given by the caller).
static void csr_bmat(pfv_ctx_impl& c, int nbr, int nbc, const pfv_csr* const* blocks, const int64_t* row_sizes,
                     const int64_t* col_sizes, pfv_csr& out) {
  stream_t s = c.stream;
  std::vector<int64_t> r0((size_t)nbr + 1, 0), c0((size_t)nbc + 1, 0);
  for (int i = 0; i < nbr; ++i) r0[i + 1] = r0[i] + row_sizes[i];
  for (int j = 0; j < nbc; ++j) c0[j + 1] = c0[j] + col_sizes[j];
  const int64_t nr = r0[nbr], ncl = c0[nbc];
  int64_t nnz = 0;
  for (int q = 0; q < nbr * nbc; ++q)
    if (blocks[q]) nnz += blocks[q]->P.nnz;
  if (nnz >= (int64_t(1) << 31) || ncl >= (int64_t(1) << 31))
    throw Error(PFV_ERR_UNSUPPORTED, "block matrix: more than 2^31 entries or columns");
  Buf<int32_t> len_;
  Buf<int64_t> ptr_;
  int32_t* len = len_.ensure((size_t)nr + 1);
  int64_t* ptr = ptr_.ensure((size_t)nr + 1);
  be_memset(len, 0, sizeof(int32_t) * (size_t)(nr + 1), s);
  for (int i = 0; i < nbr; ++i)
    for (int j = 0; j < nbc; ++j) {
      const pfv_csr* B = blocks[i * nbc + j];
      if (!B) continue;
      const int32_t* bp = B->P.indptr;
      const int64_t rr = r0[i];
      parallel_for(s, B->P.nrows, PFV_LAMBDA(int64_t r) { len[rr + r] += bp[r + 1] - bp[r]; });  // (one block per launch)
    }
  exclusive_scan<int32_t, int64_t>(s, c.scratch, len, ptr, (size_t)nr);
  out.P.nrows = nr;
  out.P.ncols = ncl;
  out.P.nnz = nnz;
  int32_t* op = out.P.indptr.ensure((size_t)nr + 1);
  int32_t* ox = out.P.indices.ensure((size_t)std::max<int64_t>(nnz, 1));
  double* ov = out.val.ensure((size_t)std::max<int64_t>(nnz, 1));
  parallel_for(s, nr + 1, PFV_LAMBDA(int64_t r) { op[r] = (int32_t)ptr[r]; });
  // fill block column by block column: the running offset inside each row is the length of the blocks to the left
  be_memset(len, 0, sizeof(int32_t) * (size_t)(nr + 1), s);
  int mr = 0;
  for (int i = 0; i < nbr; ++i) {
    int rowmax = 0;
    for (int j = 0; j < nbc; ++j) {
      const pfv_csr* B = blocks[i * nbc + j];
      if (!B) continue;
      rowmax += B->P.max_row;
      const int32_t* bp = B->P.indptr;
      const int32_t* bx = B->P.indices;
      const double* bv = B->val;
      const int64_t rr = r0[i], cc = c0[j];
      wave_for<16>(s, B->P.nrows, 16, PFV_LAMBDA(const WaveCtx& w) {
        const int64_t r = w.item;
        const int p0 = bp[r], n = bp[r + 1] - p0;
        const int64_t o = ptr[rr + r] + len[rr + r];
        PFV_LANES(t, n) {
          ox[o + t] = (int32_t)(cc + bx[p0 + t]);
          ov[o + t] = bv[p0 + t];
        }
        w.sync();
        if (w.lane0()) len[rr + r] += n;
      });
    }
    mr = std::max(mr, rowmax);
  }
  out.P.max_row = mr;
  be_sync(s);
}

static void csr_copy(pfv_ctx_impl& c, const CsrPattern& P, const double* val, pfv_csr& out) {
  stream_t s = c.stream;
  out.P.nrows = P.nrows;
  out.P.ncols = P.ncols;
  out.P.nnz = P.nnz;
  out.P.max_row = P.max_row;
  be_d2d(out.P.indptr.ensure((size_t)P.nrows + 1), P.indptr.p, sizeof(int32_t) * (size_t)(P.nrows + 1), s);
  be_d2d(out.P.indices.ensure((size_t)std::max<int64_t>(P.nnz, 1)), P.indices.p, sizeof(int32_t) * (size_t)P.nnz, s);
  be_d2d(out.val.ensure((size_t)std::max<int64_t>(P.nnz, 1)), val, sizeof(double) * (size_t)P.nnz, s);
}

}  // namespace pfv

extern "C" {

pfv_status pfv_csr_from_host(pfv_ctx* h, int64_t nrows, int64_t ncols, const int32_t* indptr, const int32_t* indices,
                             const double* values, pfv_csr** out) {
  if (!out) return PFV_ERR_ARGUMENT;
  *out = nullptr;
  return guarded(h, [&] {
    require(nrows >= 0 && ncols >= 0 && indptr && indptr[0] == 0, "bad matrix");
    const int64_t nnz = indptr[nrows];
    require(nnz >= 0 && (nnz == 0 || (indices && values)), "bad matrix");
    auto m = std::make_unique<pfv_csr>();
    m->h = h;
    m->P.nrows = nrows;
    m->P.ncols = ncols;
    m->P.nnz = nnz;
    // (the kernels that follow, csr_check_sorted first, walk [indptr[r], indptr[r + 1]) of the uploaded arrays: an indptr
    // that decreases or leaves [0, nnz] is refused here, on the host, before anything is uploaded or launched)
    int mr = 0;
    for (int64_t r = 0; r < nrows; ++r) {
      require(indptr[r + 1] >= indptr[r] && indptr[r + 1] <= nnz, "indptr must be non-decreasing and within [0, nnz]");
      mr = std::max(mr, indptr[r + 1] - indptr[r]);
    }
    m->P.max_row = mr;
    auto s = h->stream;
    be_h2d(m->P.indptr.ensure((size_t)nrows + 1), indptr, sizeof(int32_t) * (size_t)(nrows + 1), s);
    be_h2d(m->P.indices.ensure((size_t)std::max<int64_t>(nnz, 1)), indices, sizeof(int32_t) * (size_t)nnz, s);
    be_h2d(m->val.ensure((size_t)std::max<int64_t>(nnz, 1)), values, sizeof(double) * (size_t)nnz, s);
    pfv::csr_check_sorted(*h, m->P, "pfv_csr_from_host");
    *out = m.release();
  });
}

// device-to-device copy of a discretization matrix of `src` (which: pfv_matrix_id), owned by `h` (same device)
pfv_status pfv_csr_from_matrix(pfv_ctx* h, pfv_ctx* src, int which, pfv_csr** out) {
  if (!out || !src) return PFV_ERR_ARGUMENT;
  *out = nullptr;
  return guarded(h, [&] {
    require(which >= 0 && which < PFV_NUM_MATS, "bad matrix selector");
    require(src->device == h->device, "the handles live on different devices");
    require(pattern_ready(src, which) && src->filled[which], "discretize first");
    {
      pfv::PoolScope src_pool(&src->pool);  // (the index array of vector_source is written on demand, into src's buffers)
      materialize_pattern(src, which);
    }
    pfv::be_sync(src->stream);
    auto m = std::make_unique<pfv_csr>();
    m->h = h;
    pfv::csr_copy(*h, src->pattern_of(which), src->val[which].p, *m);
    pfv::be_sync(h->stream);
    *out = m.release();
  });
}

pfv_status pfv_csr_block_diag(pfv_ctx* h, int n, const pfv_csr* const* blocks, pfv_csr** out) {
  if (!out) return PFV_ERR_ARGUMENT;
  *out = nullptr;
  return guarded(h, [&] {
    require(n >= 0 && (n == 0 || blocks), "bad block list");
    for (int b = 0; b < n; ++b) require(blocks[b] && blocks[b]->h && blocks[b]->h->device == h->device, "bad block");
    auto m = std::make_unique<pfv_csr>();
    m->h = h;
    pfv::csr_block_diag(*h, n, blocks, *m);
    pfv::be_sync(h->stream);
    *out = m.release();
  });
}

pfv_status pfv_csr_matmul(pfv_ctx* h, const pfv_csr* A, const pfv_csr* B, pfv_csr** out) {
  if (!out) return PFV_ERR_ARGUMENT;
  *out = nullptr;
  return guarded(h, [&] {
    require(A && B, "null matrix");
    auto m = std::make_unique<pfv_csr>();
    m->h = h;
    pfv::csr_spgemm(*h, *A, *B, *m);
    *out = m.release();
  });
}

pfv_status pfv_csr_axpby(pfv_ctx* h, double alpha, const pfv_csr* A, double beta, const pfv_csr* B, pfv_csr** out) {
  if (!out) return PFV_ERR_ARGUMENT;
  *out = nullptr;
  return guarded(h, [&] {
    require(A && B, "null matrix");
    auto m = std::make_unique<pfv_csr>();
    m->h = h;
    pfv::csr_axpby(*h, alpha, *A, beta, *B, *m);
    *out = m.release();
  });
}

pfv_status pfv_csr_transpose(pfv_ctx* h, const pfv_csr* A, pfv_csr** out) {
  if (!out) return PFV_ERR_ARGUMENT;
  *out = nullptr;
  return guarded(h, [&] {
    require(A != nullptr, "null matrix");
    auto m = std::make_unique<pfv_csr>();
    m->h = h;
    pfv::csr_transpose(*h, *A, *m);
    *out = m.release();
  });
}

// blocks: nbr x nbc pointers, row-major, NULL = zero block; row_sizes[nbr], col_sizes[nbc]
pfv_status pfv_csr_bmat(pfv_ctx* h, int nbr, int nbc, const pfv_csr* const* blocks, const int64_t* row_sizes,
                        const int64_t* col_sizes, pfv_csr** out) {
  if (!out) return PFV_ERR_ARGUMENT;
  *out = nullptr;
  return guarded(h, [&] {
    require(nbr >= 1 && nbc >= 1 && blocks && row_sizes && col_sizes, "bad block grid");
    for (int i = 0; i < nbr; ++i)
      for (int j = 0; j < nbc; ++j) {
        const pfv_csr* B = blocks[i * nbc + j];
        require(row_sizes[i] >= 0 && col_sizes[j] >= 0, "negative block size");
        if (B) {
          require(B->h && B->h->device == h->device, "bad block");
          require(B->P.nrows == row_sizes[i] && B->P.ncols == col_sizes[j], "block matrix: a block does not fit its row / column");
        }
      }
    auto m = std::make_unique<pfv_csr>();
    m->h = h;
    pfv::csr_bmat(*h, nbr, nbc, blocks, row_sizes, col_sizes, *m);
    *out = m.release();
  });
}

// in place: A <- diag(row) A diag(col); either vector may be NULL (host arrays)
pfv_status pfv_csr_scale(pfv_csr* A, const double* row_scale, const double* col_scale) {
  if (!A) return PFV_ERR_ARGUMENT;
  return guarded(A->h, [&] {
    auto s = A->h->stream;
    pfv::Buf<double> rs, cs;
    double* r = nullptr;
    double* cc = nullptr;
    if (row_scale) {
      r = rs.ensure((size_t)std::max<int64_t>(A->P.nrows, 1));
      be_h2d(r, row_scale, sizeof(double) * (size_t)A->P.nrows, s);
    }
    if (col_scale) {
      cc = cs.ensure((size_t)std::max<int64_t>(A->P.ncols, 1));
      be_h2d(cc, col_scale, sizeof(double) * (size_t)A->P.ncols, s);
    }
    const int32_t* ip = A->P.indptr;
    const int32_t* ix = A->P.indices;
    double* v = A->val;
    pfv::wave_for<16>(s, A->P.nrows, 16, PFV_LAMBDA(const pfv::WaveCtx& w) {
      const int64_t row = w.item;
      const int p0 = ip[row], len = ip[row + 1] - p0;
      const double f = r ? r[row] : 1.0;
      PFV_LANES(t, len) v[p0 + t] = f * v[p0 + t] * (cc ? cc[ix[p0 + t]] : 1.0);
    });
    pfv::be_sync(s);
  });
}

// in place: A <- A / s as scipy computes it: ``_divide`` is ``_mul_scalar(1. / s)``, every value multiplied by the rounded
// reciprocal -- not a true division, from which it differs in the last bit for most s
pfv_status pfv_csr_divide(pfv_csr* A, double s_) {
  if (!A) return PFV_ERR_ARGUMENT;
  return guarded(A->h, [&] {
    auto s = A->h->stream;
    double* v = A->val;
    const double inv = 1.0 / s_;
    pfv::parallel_for(s, A->P.nnz, PFV_LAMBDA(int64_t e) { v[e] = v[e] * inv; });
    pfv::be_sync(s);
  });
}

// y = A x on device vectors (A.ncols / A.nrows doubles), on the stream of the handle that owns A
pfv_status pfv_csr_spmv_device(const pfv_csr* A, const double* d_x, double* d_y) {
  if (!A) return PFV_ERR_ARGUMENT;
  return guarded(A->h, [&] {
    require(d_x && d_y, "null vector");
    pfv::amg_spmv_t<double, 0>(*A->h, A->P, A->val.p, d_x, d_y, nullptr, nullptr, 0.0);
  });
}

// y = A x with host vectors
pfv_status pfv_csr_spmv(const pfv_csr* A, const double* x, double* y) {
  if (!A) return PFV_ERR_ARGUMENT;
  return guarded(A->h, [&] {
    require(x && y, "null vector");
    auto s = A->h->stream;
    pfv::Buf<double> dx, dy;
    double* px = dx.ensure((size_t)std::max<int64_t>(A->P.ncols, 1));
    double* py = dy.ensure((size_t)std::max<int64_t>(A->P.nrows, 1));
    be_h2d(px, x, sizeof(double) * (size_t)A->P.ncols, s);
    pfv::amg_spmv_t<double, 0>(*A->h, A->P, A->val.p, px, py, nullptr, nullptr, 0.0);
    be_d2h(y, py, sizeof(double) * (size_t)A->P.nrows, s);
    pfv::be_sync(s);
  });
}

pfv_status pfv_csr_info(const pfv_csr* A, int64_t* nrows, int64_t* ncols, int64_t* nnz) {
  if (!A) return PFV_ERR_ARGUMENT;
  if (nrows) *nrows = A->P.nrows;
  if (ncols) *ncols = A->P.ncols;
  if (nnz) *nnz = A->P.nnz;
  return PFV_OK;
}

pfv_status pfv_csr_get(const pfv_csr* A, int32_t* indptr, int32_t* indices, double* values) {
  if (!A) return PFV_ERR_ARGUMENT;
  return guarded(A->h, [&] {
    auto s = A->h->stream;
    if (indptr) be_d2h(indptr, A->P.indptr.p, sizeof(int32_t) * (size_t)(A->P.nrows + 1), s);
    if (indices) be_d2h(indices, A->P.indices.p, sizeof(int32_t) * (size_t)A->P.nnz, s);
    if (values) be_d2h(values, A->val.p, sizeof(double) * (size_t)A->P.nnz, s);
    pfv::be_sync(s);
  });
}

// (A, rhs) become the active system of h (what pfv_solve / pfv_solve_sharded / pfv_amg_setup work on): device-to-device,
// rhs is a host array unless rhs_on_device.  Same requirements as pfv_set_system (square, non-zero diagonal).
pfv_status pfv_csr_set_system(pfv_ctx* h, const pfv_csr* A, const double* rhs, int rhs_on_device) {
  return guarded(h, [&] {
    require(A && rhs, "bad system");
    require(A->P.nrows == A->P.ncols && A->P.nrows > 0, "the system matrix must be square");
    require(A->h->device == h->device, "the matrix lives on another device");
    const int64_t n = A->P.nrows, nnz = A->P.nnz;
    auto s = h->stream;
    pfv::be_sync(A->h->stream);
    pfv::CsrPattern& P = h->pat_user;
    P.nrows = P.ncols = n;
    P.nnz = nnz;
    P.max_row = A->P.max_row;
    int32_t* ip = P.indptr.ensure((size_t)n + 1);
    int32_t* ix = P.indices.ensure((size_t)std::max<int64_t>(nnz, 1));
    double* v = h->val[PFV_MAT_USER_SYSTEM].ensure((size_t)std::max<int64_t>(nnz, 1));
    double* b = h->rhs_u.ensure((size_t)n);
    pfv::be_d2d(ip, A->P.indptr.p, sizeof(int32_t) * (size_t)(n + 1), s);
    pfv::be_d2d(ix, A->P.indices.p, sizeof(int32_t) * (size_t)nnz, s);
    pfv::be_d2d(v, A->val.p, sizeof(double) * (size_t)nnz, s);
    if (rhs_on_device) pfv::be_d2d(b, rhs, sizeof(double) * (size_t)n, s);
    else be_h2d(b, rhs, sizeof(double) * (size_t)n, s);
    user_system_ready(h);
  });
}

void pfv_csr_free(pfv_csr* A) {
  if (!A) return;
  pfv_ctx* h = A->h;
#ifndef PFV_EMULATE
  if (h) {
    (void)hipSetDevice(h->device);
    (void)hipStreamSynchronize(h->stream);
  }
#endif
  pfv::PoolScope pool_scope(h ? &h->pool : nullptr);
  delete A;
}

}  // extern "C"
