// spmv_win.inc — "windowed" CSR SpMV for the solve (SURVEY §8 a21, the dominant kernel).
//
// Measured on MI355X (2 M tets, 70 entries per row): the plain CSR kernel is not limited by HBM but by
// the per-entry gather x[col] — one divergent 8-byte global load per entry costs more address
// cycles than the two coalesced streams together (replacing the f64 values by f32 took 31 % of the
// bytes but only 10 % of the time away).  FV matrices are local: the 64 rows of a block touch
// ~650 distinct columns for 4 500 entries.  So, once per matrix pattern, every block of 64 rows gets
// the sorted list of its distinct columns ("window"), and every entry the 16-bit position of its
// column in that list.  The kernel stages the window's x values in LDS with coalesced loads (7x
// fewer global gathers, runs of consecutive addresses) and the per-entry gather becomes an LDS
// read; the index stream shrinks from 4 to 2 bytes per entry.  0.37 -> 0.26 ms per product with f64
// values, 0.31 -> 0.18 ms with the f32 copy the AMG smoother reads.
//
// A block whose window exceeds kWinMax columns (a matrix without locality) makes the whole matrix
// fall back to the plain CSR kernels.  Device only: the host emulation build has no windows.

namespace pfv {

constexpr int kWinRows = 64;     // rows per block (= per workgroup)
constexpr int kWinMax = 4096;    // largest window (32 KB of LDS)
constexpr int kWinHash = 8192;   // open-addressing table of the build kernel

// operands of the fused cycle products (MODE 4 / 5 of k_spmv_win and of amg.inc's k_amg_spmv)
struct SpmvFuse {
  const double* xc = nullptr;   // MODE 4: coarse correction(s): t[c] = x[c] + alpha (xc[agg(c)] + xc2[agg(c)])
  const double* xc2 = nullptr;  //         (optional)
  const int32_t* agg = nullptr;
  int bs = 1;
  double alpha = 0.0;
  double* y2 = nullptr;         // MODE 5: second output
};
PFV_HD inline double spmv_prolonged(const SpmvFuse& F, const double* x, int64_t c) {
  const int64_t ci = c / F.bs;
  const int64_t a = (int64_t)F.agg[ci] * F.bs + (c - ci * F.bs);
  double v = F.xc[a];
  if (F.xc2) v += F.xc2[a];
  return x[c] + F.alpha * v;
}

#ifndef PFV_EMULATE
// pass 1 (FILL = false): distinct columns per block -> cnt, max -> st[0], overflow -> st[1]
// pass 2 (FILL = true):  window (ascending) -> wcol[wptr[b]..], local index of every entry -> lidx
// one pass (ONE = true, FILL = true): the window of block b goes to wcol[b * stride ..) and its length to cnt[b] --
// no counting pass, no scan; a block with more than `stride` distinct columns raises st[1] (the host then falls back
// to the two-pass form).  Hashing every entry into the LDS table is the cost of a pass (2.4 ms for the 138 M entries
// of the 2 M-cell system): doing it once instead of twice is what this saves.
template <bool FILL, bool ONE = false>
__global__ void __launch_bounds__(256) k_win_build(int64_t nrows, const int32_t* __restrict__ indptr,
                                                   const int32_t* __restrict__ indices, int32_t* __restrict__ cnt,
                                                   int64_t* __restrict__ wptr, int32_t* __restrict__ wcol,
                                                   uint16_t* __restrict__ lidx, int32_t* __restrict__ st,
                                                   int64_t stride = 0) {
  __shared__ int32_t table[kWinHash];
  __shared__ int32_t keys[FILL ? kWinMax : 1];
  __shared__ int32_t nuniq, nkeys;
  const int tid = threadIdx.x;
  const int64_t row0 = (int64_t)blockIdx.x * kWinRows;
  const int64_t row1 = row0 + kWinRows < nrows ? row0 + kWinRows : nrows;
  const int e0 = indptr[row0], e1 = indptr[row1];
  for (int i = tid; i < kWinHash; i += 256) table[i] = -1;
  if (tid == 0) nuniq = nkeys = 0;
  __syncthreads();
  for (int e = e0 + tid; e < e1; e += 256) {
    const int32_t col = indices[e];
    unsigned h = ((unsigned)col * 2654435761u) >> 19;  // 13 bits
    while (true) {
      const int32_t prev = atomicCAS(&table[h], -1, col);
      if (prev == -1) { atomicAdd(&nuniq, 1); break; }
      if (prev == col) break;
      h = (h + 1) & (kWinHash - 1);
    }
    // stop filling a hopeless table (keeps the probe loop finite: <= kWinMax + 256 slots in use)
    if (*(volatile int32_t*)&nuniq > kWinMax) break;
  }
  __syncthreads();
  const int nu = nuniq;
  if (!FILL) {
    if (tid == 0) {
      if (nu > kWinMax) { cnt[blockIdx.x] = 0; atomicMax(st + 1, 1); }
      else { cnt[blockIdx.x] = nu; atomicMax(st, nu); }
    }
    return;
  } else {
    if (ONE) {
      if (tid == 0) {
        cnt[blockIdx.x] = nu;
        wptr[blockIdx.x] = (int64_t)blockIdx.x * stride;
        if (nu > kWinMax || nu > stride) atomicMax(st + 1, 1);
        else atomicMax(st, nu);
      }
      if (nu > kWinMax || nu > stride) return;
    }
    if (nu > kWinMax) return;  // (pass 1 has flagged it; the host does not launch pass 2 then)
    for (int i = tid; i < kWinHash; i += 256) {
      const int32_t k = table[i];
      if (k >= 0) keys[atomicAdd(&nkeys, 1)] = k;
    }
    int np2 = 1;
    while (np2 < nu) np2 <<= 1;
    __syncthreads();
    for (int i = nu + tid; i < np2; i += 256) keys[i] = 0x7fffffff;
    __syncthreads();
    for (int k = 2; k <= np2; k <<= 1) {
      for (int j = k >> 1; j > 0; j >>= 1) {
        for (int i = tid; i < np2; i += 256) {
          const int l = i ^ j;
          if (l > i) {
            const int32_t a = keys[i], b = keys[l];
            const bool up = (i & k) == 0;
            if ((a > b) == up) { keys[i] = b; keys[l] = a; }
          }
        }
        __syncthreads();
      }
    }
    const int64_t w0 = ONE ? (int64_t)blockIdx.x * stride : wptr[blockIdx.x];
    for (int i = tid; i < nu; i += 256) wcol[w0 + i] = keys[i];
    for (int e = e0 + tid; e < e1; e += 256) {
      const int32_t col = indices[e];
      int lo = 0, hi = nu - 1;
      while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (keys[mid] < col) lo = mid + 1; else hi = mid;
      }
      lidx[e] = (uint16_t)lo;
    }
  }
}

// Windows of a matrix whose rows are SUBSETS of the rows of a matrix that already has windows (the strength-filtered
// copy of A the AMG cycle smooths with: amg.inc).  The parent's window of a block is a sorted superset of the block's
// columns, so hashing and sorting -- what k_win_build spends its time on -- are not needed: the parent's window goes
// to LDS, every entry finds its column there by binary search and flags it, a scan of the flags ranks the columns that
// are in use, and the entry's position is the rank.  One-pass layout (fixed stride, lengths in cnt).
__global__ void __launch_bounds__(256) k_win_derive(int64_t nrows, const int32_t* __restrict__ indptr,
                                                    const int32_t* __restrict__ indices, const int64_t* __restrict__ pwptr,
                                                    const int32_t* __restrict__ pwlen, const int32_t* __restrict__ pwcol,
                                                    int32_t* __restrict__ cnt, int64_t* __restrict__ wptr,
                                                    int32_t* __restrict__ wcol, uint16_t* __restrict__ lidx,
                                                    int32_t* __restrict__ st, int64_t stride) {
  __shared__ int32_t keys[kWinMax];
  __shared__ int32_t rank[kWinMax];
  __shared__ int32_t wsum[256];
  const int tid = threadIdx.x;
  const int64_t row0 = (int64_t)blockIdx.x * kWinRows;
  const int64_t row1 = row0 + kWinRows < nrows ? row0 + kWinRows : nrows;
  const int e0 = indptr[row0], e1 = indptr[row1];
  const int64_t pw0 = pwptr[blockIdx.x];
  const int pn = pwlen ? pwlen[blockIdx.x] : (int)(pwptr[blockIdx.x + 1] - pw0);
  for (int i = tid; i < pn; i += 256) {
    keys[i] = pwcol[pw0 + i];
    rank[i] = 0;
  }
  __syncthreads();
  bool missing = false;
  for (int e = e0 + tid; e < e1; e += 256) {
    const int32_t col = indices[e];
    int lo = 0, hi = pn - 1;
    while (lo < hi) {
      const int mid = (lo + hi) >> 1;
      if (keys[mid] < col) lo = mid + 1; else hi = mid;
    }
    if (pn > 0 && keys[lo] == col) rank[lo] = 1;  // (all writers store the same value)
    else missing = true;
  }
  if (missing) atomicMax(st + 1, 1);  // not a subset of the parent's columns: the caller falls back to k_win_build
  __syncthreads();
  // exclusive scan of the flags: every thread owns a contiguous chunk
  const int chunk = (pn + 255) / 256;
  const int i0 = tid * chunk, i1 = i0 + chunk < pn ? i0 + chunk : pn;
  int loc = 0;
  for (int i = i0; i < i1; ++i) loc += rank[i];
  wsum[tid] = loc;
  __syncthreads();
  for (int off = 1; off < 256; off <<= 1) {
    const int v = tid >= off ? wsum[tid - off] : 0;
    __syncthreads();
    wsum[tid] += v;
    __syncthreads();
  }
  const int total = wsum[255];
  int run = wsum[tid] - loc;
  const int64_t w0 = (int64_t)blockIdx.x * stride;
  // (a parent built by the two-pass layout may hold more than `stride` columns in a block: a filtered block that keeps
  // more of them than its fixed-stride slice takes is flagged and writes NOTHING beyond the slice -- the caller falls
  // back to k_win_build, as k_win_build<true, true> itself returns before it writes)
  const bool fits = total <= stride;
  for (int i = i0; i < i1; ++i) {
    const int f = rank[i];
    rank[i] = run;
    if (f && fits) wcol[w0 + run] = keys[i];
    run += f;
  }
  if (tid == 0) {
    cnt[blockIdx.x] = total;
    wptr[blockIdx.x] = w0;
    if (!fits) atomicMax(st + 1, 1);
    else atomicMax(st, total);
  }
  if (!fits) return;  // (block-uniform: `total` comes out of shared memory after a barrier)
  __syncthreads();
  for (int e = e0 + tid; e < e1; e += 256) {
    const int32_t col = indices[e];
    int lo = 0, hi = pn - 1;
    while (lo < hi) {
      const int mid = (lo + hi) >> 1;
      if (keys[mid] < col) lo = mid + 1; else hi = mid;
    }
    lidx[e] = (uint16_t)rank[lo];
  }
}

// MODE 0: y = A x;  1: y = x + omega dinv (w - A x);  2: y = A x, a = (w, y);  3: y = A x, a = (y, w), b = (y, y)
// Fused forms of the AMG cycle (amg.inc: amg_cycle), operands in SpmvFuse:
// MODE 4: y = t + omega dinv (w - A t) with t = x + alpha P (xc + xc2) formed while the window is staged (t is never stored:
//         the prolongation kernel and its round trip through memory are gone);
// MODE 5: y = w - A x and y2 = omega dinv y (the residual a second coarse visit works on, and that visit's first
//         smoothing step from a zero guess, in the launch of the product)
// MODE 6: y = w - A x alone (level 0 of the cycle: the restriction and the post-smoothing through AP read only b - A_s x0)
template <int L, int U, class VT, int MODE>
__global__ void __launch_bounds__(256) k_spmv_win(int64_t nrows, const int32_t* __restrict__ indptr,
                                                  const int64_t* __restrict__ wptr, const int32_t* __restrict__ wcol,
                                                  const uint16_t* __restrict__ lidx, const VT* __restrict__ val,
                                                  const double* __restrict__ x, double* __restrict__ y,
                                                  const double* __restrict__ w, const double* __restrict__ dinv,
                                                  double omega, Reduce R, const int32_t* __restrict__ wlen,
                                                  const int32_t* __restrict__ blist, const SpmvFuse F) {
  extern __shared__ double xs[];
  // blist: the launch covers only the listed row blocks (sharded solves: blocks without halo columns first, the others
  // once the halo exchange has landed); every block keeps its own slot of the reduction partials
  const unsigned blk = blist ? (unsigned)blist[blockIdx.x] : blockIdx.x;
  const int64_t w0 = wptr[blk];
  const int wn = wlen ? wlen[blk] : (int)(wptr[blk + 1] - w0);  // (fixed-stride windows carry their length)
  for (int i = threadIdx.x; i < wn; i += 256) {
    const int cw = wcol[w0 + i];
    xs[i] = MODE == 4 ? spmv_prolonged(F, x, cw) : x[cw];
  }
  __syncthreads();
  const int lane = threadIdx.x % L;
  const int64_t row0 = (int64_t)blk * kWinRows;
  double acc1 = 0.0, acc2 = 0.0;
#pragma unroll 1
  for (int k = 0; k < kWinRows / (256 / L); ++k) {
    const int64_t row = row0 + k * (256 / L) + threadIdx.x / L;
    const bool live = row < nrows;
    const int a = live ? indptr[row] : 0, b = live ? indptr[row + 1] : 0;
    double wrow = 0.0, xrow = 0.0, drow = 0.0;
    if (MODE != 0 && live && lane == 0) {
      wrow = w[row];
      if (MODE == 1) { xrow = x[row]; drow = dinv[row]; }
      if (MODE == 4) { xrow = spmv_prolonged(F, x, row); drow = dinv[row]; }
      if (MODE == 5) drow = dinv[row];
    }
    double sum = 0.0;
    for (int p = a + lane; p < b; p += L * U) {
      int col[U];
      double v[U];
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const int pp = p + u * L;
        const bool ok = pp < b;
        const int pc = ok ? pp : a;
        col[u] = lidx[pc];
        const double vv = (double)val[pc];
        v[u] = ok ? vv : 0.0;
      }
#pragma unroll
      for (int u = 0; u < U; ++u) sum += v[u] * xs[col[u]];
    }
#pragma unroll
    for (int o = L / 2; o > 0; o >>= 1) sum += __shfl_down(sum, o, L);
    if (live && lane == 0) {
      if (MODE == 1 || MODE == 4) y[row] = xrow + omega * drow * (wrow - sum);
      else if (MODE == 5) {
        const double res = wrow - sum;
        y[row] = res;
        F.y2[row] = omega * drow * res;
      } else if (MODE == 6) y[row] = wrow - sum;
      else y[row] = sum;
      if (MODE == 2) acc1 += wrow * sum;
      if (MODE == 3) { acc1 += sum * wrow; acc2 += sum * sum; }
    }
  }
  if (MODE == 2 || MODE == 3) reduce_finalize_slot(acc1, acc2, R, blk);
}

// k_spmv_win with every load that does not depend on the staged window issued BEFORE the barrier that publishes it:
// the row bounds of all the block's passes, the first U-chunk of every row (for rows of up to L * U entries: the whole
// row) and the row scalars travel while the window's two-step gather (column list -> x) is in flight.  The plain kernel
// serialises the two chains: window gather, barrier, then per pass row bounds -> entries.  Same products in the same
// order: same bits.  (L <= 16: 2 or 4 passes of 256 / L rows; registers: passes x U x 3.)
template <int L, int U, class VT, int MODE>
__global__ void __launch_bounds__(256) k_spmv_win_pre(int64_t nrows, const int32_t* __restrict__ indptr,
                                                      const int64_t* __restrict__ wptr, const int32_t* __restrict__ wcol,
                                                      const uint16_t* __restrict__ lidx, const VT* __restrict__ val,
                                                      const double* __restrict__ x, double* __restrict__ y,
                                                      const double* __restrict__ w, const double* __restrict__ dinv,
                                                      double omega, Reduce R, const int32_t* __restrict__ wlen,
                                                      const int32_t* __restrict__ blist) {
  extern __shared__ double xs[];
  constexpr int RP = 256 / L, NP = kWinRows / RP, WU = 4;
  const unsigned blk = blist ? (unsigned)blist[blockIdx.x] : blockIdx.x;
  const int64_t w0 = wptr[blk];
  const int wn = wlen ? wlen[blk] : (int)(wptr[blk + 1] - w0);
  const int lane = threadIdx.x % L;
  const int64_t row0 = (int64_t)blk * kWinRows;
  int wc[WU];
#pragma unroll
  for (int j = 0; j < WU; ++j) {
    const int i = threadIdx.x + 256 * j;
    wc[j] = i < wn ? wcol[w0 + i] : -1;
  }
  int a[NP], b[NP];
#pragma unroll
  for (int k = 0; k < NP; ++k) {
    const int64_t row = row0 + k * RP + threadIdx.x / L;
    const bool live = row < nrows;
    a[k] = live ? indptr[row] : 0;
    b[k] = live ? indptr[row + 1] : 0;
  }
  double xv[WU];
#pragma unroll
  for (int j = 0; j < WU; ++j) xv[j] = wc[j] >= 0 ? x[wc[j]] : 0.0;
  int col[NP][U];
  double v[NP][U];
#pragma unroll
  for (int k = 0; k < NP; ++k) {
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int pp = a[k] + lane + u * L;
      const bool ok = pp < b[k];
      col[k][u] = ok ? (int)lidx[pp] : -1;
      v[k][u] = ok ? (double)val[pp] : 0.0;
    }
  }
  double wrow[NP], xrow[NP], drow[NP];
#pragma unroll
  for (int k = 0; k < NP; ++k) {
    wrow[k] = xrow[k] = drow[k] = 0.0;
    const int64_t row = row0 + k * RP + threadIdx.x / L;
    if (MODE != 0 && row < nrows && lane == 0) {
      wrow[k] = w[row];
      if (MODE == 1) { xrow[k] = x[row]; drow[k] = dinv[row]; }
    }
  }
#pragma unroll
  for (int j = 0; j < WU; ++j) {
    const int i = threadIdx.x + 256 * j;
    if (i < wn) xs[i] = xv[j];
  }
  for (int i = threadIdx.x + 256 * WU; i < wn; i += 256) xs[i] = x[wcol[w0 + i]];
  __syncthreads();
  double acc1 = 0.0, acc2 = 0.0;
#pragma unroll
  for (int k = 0; k < NP; ++k) {
    const int64_t row = row0 + k * RP + threadIdx.x / L;
    const bool live = row < nrows;
    double sum = 0.0;
#pragma unroll
    for (int u = 0; u < U; ++u) sum += v[k][u] * (col[k][u] >= 0 ? xs[col[k][u]] : 0.0);
    for (int p = a[k] + lane + L * U; p < b[k]; p += L * U) {
      int c2[U];
      double v2[U];
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const int pp = p + u * L;
        const bool ok = pp < b[k];
        const int pc = ok ? pp : a[k];
        c2[u] = lidx[pc];
        const double vv = (double)val[pc];
        v2[u] = ok ? vv : 0.0;
      }
#pragma unroll
      for (int u = 0; u < U; ++u) sum += v2[u] * xs[c2[u]];
    }
#pragma unroll
    for (int o = L / 2; o > 0; o >>= 1) sum += __shfl_down(sum, o, L);
    if (live && lane == 0) {
      if (MODE == 1) y[row] = xrow[k] + omega * drow[k] * (wrow[k] - sum);
      else y[row] = sum;
      if (MODE == 2) acc1 += wrow[k] * sum;
      if (MODE == 3) { acc1 += sum * wrow[k]; acc2 += sum * sum; }
    }
  }
  if (MODE >= 2) reduce_finalize_slot(acc1, acc2, R, blk);
}

template <int L, class VT, int MODE>
static void launch_spmv_win_u(stream_t s, int U, const WinCsr& W, const int32_t* ip, const VT* val, const double* x,
                              double* y, const double* w, const double* dinv, double omega, const Reduce& R,
                              const int32_t* blist = nullptr, int64_t nlist = 0, const SpmvFuse& F = SpmvFuse{}) {
  if (blist && nlist <= 0) return;
  const dim3 grid((unsigned)(blist ? nlist : W.nblk)), block(256);
  const size_t lds = (size_t)W.wmax * sizeof(double);
  if constexpr (L <= 16 && sizeof(VT) == 8 && MODE < 4) {
    // PFV_SPMV_PRELOAD=0: the plain kernel.  Only the f64 Krylov products preload -- measured
    // (profiles/r04_ab_runs.txt, call O): the f64 product of the 2 M-cell flow system (L 16, U 5) gains 0.6 ms per
    // solve; the f32 products of the cycle gain nothing at L 8 and LOSE 20 % at L 16, U 6 (MPSA: 127 registers held
    // across the barrier, 4 wavefronts per SIMD), so they are not even instantiated
    static const bool pre = env_int("PFV_SPMV_PRELOAD", 1) != 0;
    if (pre && U <= 5) {  // (6 chunks: the register budget of the case that lost)
#define PFV_WINPRE_CASE(UU)                                                                                         \
  PFV_LAUNCH(HIP_KERNEL_NAME(k_spmv_win_pre<L, UU, VT, MODE>), grid, block, lds, s, W.nrows, ip, W.wptr64, \
                     W.wcol.p, W.lidx.p, val, x, y, w, dinv, omega, R, W.wlen, blist)
      switch (U) {
        case 1: case 2: PFV_WINPRE_CASE(2); break;
        case 3: PFV_WINPRE_CASE(3); break;
        case 4: PFV_WINPRE_CASE(4); break;
        default: PFV_WINPRE_CASE(5); break;
      }
#undef PFV_WINPRE_CASE
      return;
    }
  }
#define PFV_WIN_CASE(UU)                                                                                        \
  PFV_LAUNCH(HIP_KERNEL_NAME(k_spmv_win<L, UU, VT, MODE>), grid, block, lds, s, W.nrows, ip, W.wptr64, \
                     W.wcol.p, W.lidx.p, val, x, y, w, dinv, omega, R, W.wlen, blist, F)
  switch (U) {
    case 1: case 2: PFV_WIN_CASE(2); break;
    case 3: PFV_WIN_CASE(3); break;
    case 4: PFV_WIN_CASE(4); break;
    case 5: PFV_WIN_CASE(5); break;
    default: PFV_WIN_CASE(6); break;
  }
#undef PFV_WIN_CASE
}
#endif  // !PFV_EMULATE

// Build the window structure of P (W.ok tells whether the windowed kernels may be used).
static void win_build(pfv_ctx_impl& c, const CsrPattern& P, WinCsr& W) {
  W.ok = false;
#ifdef PFV_EMULATE
  (void)c; (void)P;
#else
  if (env_int("PFV_SPMV_WINDOW", 1) == 0 || P.nrows < 1 || P.nnz < 1) return;
  stream_t s = c.stream;
  const int64_t nblk = (P.nrows + kWinRows - 1) / kWinRows;
  int32_t* cnt = W.cnt.ensure(nblk + 1);
  int64_t* wptr = W.wptr64buf.ensure(nblk + 1);
  int32_t* st = c.status.ensure(16);
  int32_t hst[2];
  W.wlen = nullptr;
  // one pass at a fixed stride per block (PFV_WIN_ONEPASS=0: the two-pass compact form only)
  const int64_t stride = env_int("PFV_WIN_STRIDE", 1024);
  bool built = false;
  if (env_int("PFV_WIN_ONEPASS", 1) != 0 && stride > 0 && stride <= kWinMax && (double)nblk * (double)stride * 4.0 <= 2.0e9) {
    be_memset(st + 12, 0, 2 * sizeof(int32_t), s);
    int32_t* wcol = W.wcol.ensure(std::max<int64_t>(nblk * stride, 1));
    uint16_t* lidx = W.lidx.ensure(P.nnz);
    PFV_LAUNCH(HIP_KERNEL_NAME(k_win_build<true, true>), dim3((unsigned)nblk), dim3(256), 0, s, P.nrows,
                       P.indptr.p, P.indices.p, cnt, wptr, wcol, lidx, st + 12, stride);
    PFV_HIP_CHECK(hipGetLastError());
    be_d2h(hst, st + 12, sizeof(hst), s);
    if (hst[1] == 0) {
      built = true;
      W.wlen = cnt;
    }
  }
  if (!built) {
    be_memset(st + 12, 0, 2 * sizeof(int32_t), s);
    be_memset(cnt + nblk, 0, sizeof(int32_t), s);
    PFV_LAUNCH(HIP_KERNEL_NAME(k_win_build<false>), dim3((unsigned)nblk), dim3(256), 0, s, P.nrows,
                       P.indptr.p, P.indices.p, cnt, nullptr, nullptr, nullptr, st + 12, (int64_t)0);
    exclusive_scan<int32_t, int64_t>(s, c.scratch, cnt, wptr, (size_t)nblk);
    be_d2h(hst, st + 12, sizeof(hst), s);
    if (env_int("PFV_DEBUG_WIN", 0))
      std::fprintf(stderr, "win_build: rows %lld nnz %lld blocks %lld wmax %d overflow %d\n", (long long)P.nrows,
                   (long long)P.nnz, (long long)nblk, hst[0], hst[1]);
    if (hst[1] != 0) return;  // a block without locality: plain CSR kernels
    const int64_t total = read_scalar<int64_t>(s, wptr + nblk);
    int32_t* wcol = W.wcol.ensure(std::max<int64_t>(total, 1));
    uint16_t* lidx = W.lidx.ensure(P.nnz);
    PFV_LAUNCH(HIP_KERNEL_NAME(k_win_build<true>), dim3((unsigned)nblk), dim3(256), 0, s, P.nrows,
                       P.indptr.p, P.indices.p, cnt, wptr, wcol, lidx, st + 12, (int64_t)0);
    PFV_HIP_CHECK(hipGetLastError());
  } else if (env_int("PFV_DEBUG_WIN", 0)) {
    std::fprintf(stderr, "win_build (one pass, stride %lld): rows %lld nnz %lld blocks %lld wmax %d\n", (long long)stride,
                 (long long)P.nrows, (long long)P.nnz, (long long)nblk, hst[0]);
  }
  W.wptr64 = wptr;
  W.nblk = nblk;
  W.nrows = P.nrows;
  W.nnz = P.nnz;
  W.wmax = hst[0];
  W.ok = true;
#endif
}

// Windows of P from the windows `parent` of a matrix with the same rows whose columns include P's (k_win_derive);
// false: not applicable / a column was missing -- the caller builds them from scratch.
static bool win_derive(pfv_ctx_impl& c, const CsrPattern& P, const WinCsr& parent, WinCsr& W) {
#ifdef PFV_EMULATE
  (void)c; (void)P; (void)parent; (void)W;
  return false;
#else
  if (!parent.ok || parent.nrows != P.nrows || P.nnz < 1 || env_int("PFV_WIN_DERIVE", 1) == 0) return false;
  const int64_t stride = env_int("PFV_WIN_STRIDE", 1024);
  if (parent.wmax > kWinMax || stride <= 0 || stride > kWinMax) return false;
  stream_t s = c.stream;
  const int64_t nblk = (P.nrows + kWinRows - 1) / kWinRows;
  if (nblk != parent.nblk || (double)nblk * (double)stride * 4.0 > 2.0e9) return false;
  W.ok = false;
  int32_t* cnt = W.cnt.ensure(nblk + 1);
  int64_t* wptr = W.wptr64buf.ensure(nblk + 1);
  int32_t* st = c.status.ensure(16);
  be_memset(st + 12, 0, 2 * sizeof(int32_t), s);
  int32_t* wcol = W.wcol.ensure(std::max<int64_t>(nblk * stride, 1));
  uint16_t* lidx = W.lidx.ensure(P.nnz);
  PFV_LAUNCH(k_win_derive, dim3((unsigned)nblk), dim3(256), 0, s, P.nrows, P.indptr.p, P.indices.p, parent.wptr64,
             parent.wlen, parent.wcol.p, cnt, wptr, wcol, lidx, st + 12, stride);
  PFV_HIP_CHECK(hipGetLastError());
  int32_t hst[2];
  be_d2h(hst, st + 12, sizeof(hst), s);
  if (hst[1] != 0) return false;
  W.wlen = cnt;
  W.wptr64 = wptr;
  W.nblk = nblk;
  W.nrows = P.nrows;
  W.nnz = P.nnz;
  W.wmax = hst[0];
  W.ok = true;
  return true;
#endif
}

#ifndef PFV_EMULATE
// the windowed product in one of the four modes (see k_spmv_win); caller has checked W.ok
template <class VT, int MODE>
static void spmv_win(pfv_ctx_impl& c, const CsrPattern& P, const WinCsr& W, const VT* val, const double* x, double* y,
                     const double* w, const double* dinv, double omega, const Reduce& R,
                     const int32_t* blist = nullptr, int64_t nlist = 0, const SpmvFuse& F = SpmvFuse{}) {
  stream_t s = c.stream;
  const double avg = (double)P.nnz / (double)P.nrows;
  // lanes per row.  The f32 products of the AMG cycle take 8 lanes up to 40 entries per row (the coarse levels of a flow
  // hierarchy: 27-30): their 4 000 / 500 row blocks are two rounds of workgroups at most, so what a launch waits for is a
  // block's chain of dependent loads, and 8 lanes make that 2 passes of 32 rows instead of 4 of 16 -- measured on the
  // 250 k / 31 k-row levels of the 2 M-cell system (profiles/r06_ab_runs.txt call J): residual product 12.9 -> 10.3 us,
  // prolong + smooth 15.8 -> 13.1, residual + first step 16.7 -> 13.0.  PFV_SPMV_L8_MAX_F32 overrides.
  static const int l8max_f32 = env_int("PFV_SPMV_L8_MAX_F32", 40);
  const int L = avg <= (sizeof(VT) == 4 ? (double)l8max_f32 : 20.0) ? 8 : (avg <= 160 ? 16 : 32);
  const int envU = env_int("PFV_SPMV_U", 0);
  const int U = envU ? envU : std::max(1, std::min(6, (int)std::ceil(1.1 * avg / L)));
  if (L == 8) launch_spmv_win_u<8, VT, MODE>(s, U, W, P.indptr.p, val, x, y, w, dinv, omega, R, blist, nlist, F);
  else if (L == 16) launch_spmv_win_u<16, VT, MODE>(s, U, W, P.indptr.p, val, x, y, w, dinv, omega, R, blist, nlist, F);
  else launch_spmv_win_u<32, VT, MODE>(s, U, W, P.indptr.p, val, x, y, w, dinv, omega, R, blist, nlist, F);
  PFV_HIP_CHECK(hipGetLastError());
}
#endif

}  // namespace pfv
