// linalg.inc — A = div @ flux, right-hand side, CSR SpMV and Jacobi-preconditioned Krylov.
//
// fv_elliptic.py:67-112 of the reference forms A and b with scipy SpGEMM / SpMV on the
// host; its solve is a sparse direct solver (models/solution_strategy.py:830-884).  Here
// A's rows are gathered from the signed flux rows of the cell's faces (pattern from the
// symbolic phase), and the solve is CG / BiCGStab with all vectors and scalars resident
// in HBM: no host round trip per iteration except a residual check every few steps.

namespace pfv {

static void assemble_system(pfv_ctx_impl& c) {
  stream_t s = c.stream;
  const int64_t nc = c.nc;
  double* Aval = c.val[PFV_MAT_SYSTEM].ensure(c.pat_A.nnz);
  double* diag = c.diag.ensure(nc);
  const int32_t* cf_ptr = c.cf_ptr;
  const int32_t* cf_idx = c.cf_idx;
  const int8_t* cf_sgn = c.cf_sgn;
  const int32_t* ip = c.pat_flux.indptr;
  const int32_t* ix = c.pat_flux.indices;
  const int32_t* ap = c.pat_A.indptr;
  const int32_t* ax = c.pat_A.indices;
  const double* vq = c.val[PFV_MAT_FLUX];
  const int maxrow = std::max(c.pat_A.max_row, 1);
  const size_t lds = (size_t)std::max(maxrow, 64) * 12 + 32;  // (the row's accumulators double as the reduction scratch)
  // the largest off-diagonal magnitude of every row rides along: the strength filter of the AMG setup (amg_filter)
  // starts from it, and here the row is in LDS anyway (saves its first pass over A: 0.6 ms at 2 M cells)
  double* rowmax = c.sys_rowmax.ensure(nc);
  c.sys_rowmax_for = Aval;
#ifndef PFV_EMULATE
  // Cells with at most 6 faces whose flux rows have at most 64 entries (simplices, hexahedra): the rows of ALL faces
  // of a cell are requested before any of them is used.  The generic body below takes the faces one after the other,
  // each a chain face id -> row bounds -> entries (12 dependent round trips per tetrahedron, 2.2 ms at 2 M cells);
  // here it is three.  Same accumulation order (faces in order, a barrier between them): same bits.
  constexpr int kAsmFaces = 6, kAsmChunks = 4;
  if (c.max_cell_faces <= kAsmFaces && c.pat_flux.max_row <= 16 * kAsmChunks && env_int("PFV_ASM_G", 16) == 16 &&
      env_int("PFV_ASM_PREFETCH", 1) != 0) {
    // Positions kept (round 6): where entry k of the flux row of face e of a cell lands in the cell's row of A is a
    // function of the two patterns alone.  While the patterns on the handle are the ones a key was taken for
    // (c.symb_key: kept across rebuilt topologies that are proved unchanged), the positions of the first assembly are
    // replayed from a byte array -- no column indices of flux (0.9 GB at 2 M cells), no indices of A, no searches in LDS.
    // Same accumulation order: same bits.  mode 0: search; 1: search and record; 2: replay.
    const int stride_f = 16 * kAsmChunks;                       // bytes per (cell, face)
    const int64_t stride_c = (int64_t)std::max(c.max_cell_faces, 1) * stride_f;
    int mode = 0;
    if (env_int("PFV_ASM_POS", 1) != 0 && c.symb_key != 0 && c.pat_A.max_row <= 255) {
      if (c.asm_pos_key == c.symb_key && c.asm_pos_cells == nc) {
        mode = 2;
      } else {
        c.asm_pos.ensure((size_t)(nc * stride_c));
        c.asm_diagpos.ensure((size_t)nc);
        mode = 1;
      }
    }
    uint8_t* posb = c.asm_pos.p;
    uint8_t* dpos = c.asm_diagpos.p;
    auto body = [=] __device__(const WaveCtx& w, auto mode_c) {
      constexpr int MODE = decltype(mode_c)::value;
      const int64_t cell = w.item;
      const int a0 = ap[cell], alen = ap[cell + 1] - a0;
      Carver cv(w.lds);
      double* acc = cv.take<double>(std::max(maxrow, 64));
      int32_t* aidx = cv.take<int32_t>(std::max(maxrow, 64));
      const int e0 = cf_ptr[cell], ne = cf_ptr[cell + 1] - e0;
      int mf = 0, mp0 = 0, mlen = 0;
      double msg = 0.0;
      if (w.lane < ne) {
        mf = cf_idx[e0 + w.lane];
        msg = (double)cf_sgn[e0 + w.lane];
      }
      PFV_LANES(i, alen) {
        if (MODE != 2) aidx[i] = ax[a0 + i];
        acc[i] = 0.0;
      }
      if (w.lane < ne) {
        mp0 = ip[mf];
        mlen = ip[mf + 1] - mp0;
      }
      int cj[kAsmFaces][kAsmChunks];
      double v[kAsmFaces][kAsmChunks];
      uint8_t* mypos = posb + cell * stride_c;
#pragma unroll
      for (int e = 0; e < kAsmFaces; ++e) {
        const int p0 = __shfl(mp0, e, 16), len = __shfl(mlen, e, 16);  // (lanes >= ne hold len 0)
#pragma unroll
        for (int u = 0; u < kAsmChunks; ++u) {
          const int k = u * 16 + w.lane;
          const bool live = k < len;
          if (MODE == 2) cj[e][u] = live ? (int)mypos[e * stride_f + k] : -1;
          else cj[e][u] = live ? ix[p0 + k] : -1;
          v[e][u] = live ? vq[p0 + k] : 0.0;
        }
      }
      w.lsync();
#pragma unroll
      for (int e = 0; e < kAsmFaces; ++e) {
        const double sg = __shfl(msg, e, 16);
#pragma unroll
        for (int u = 0; u < kAsmChunks; ++u) {
          if (cj[e][u] >= 0) {
            const int pos = MODE == 2 ? cj[e][u] : lower_bound_idx<int32_t>(aidx, alen, cj[e][u]);
            if (MODE == 1) mypos[e * stride_f + u * 16 + w.lane] = (uint8_t)pos;
            acc[pos] += sg * v[e][u];
          }
        }
        w.lsync();
      }
      double mx = 0.0;
      const int dp = MODE == 2 ? (int)dpos[cell] : -1;
      PFV_LANES(i, alen) {
        Aval[a0 + i] = acc[i];
        const bool is_diag = MODE == 2 ? (i == dp) : (aidx[i] == (int32_t)cell);
        if (is_diag) {
          diag[cell] = acc[i];
          if (MODE == 1) dpos[cell] = (uint8_t)i;
        } else {
          mx = fmax(mx, fabs(acc[i]));
        }
      }
      mx = fmax(mx, __shfl_xor(mx, 8, 16));
      mx = fmax(mx, __shfl_xor(mx, 4, 16));
      mx = fmax(mx, __shfl_xor(mx, 2, 16));
      mx = fmax(mx, __shfl_xor(mx, 1, 16));
      if (w.lane0()) rowmax[cell] = mx;
      w.lsync();
    };
    using M0 = std::integral_constant<int, 0>;
    using M1 = std::integral_constant<int, 1>;
    using M2 = std::integral_constant<int, 2>;
    if (mode == 2) wave_for<16>(s, nc, lds, [=] __device__(const WaveCtx& w) { body(w, M2{}); });
    else if (mode == 1) wave_for<16>(s, nc, lds, [=] __device__(const WaveCtx& w) { body(w, M1{}); });
    else wave_for<16>(s, nc, lds, [=] __device__(const WaveCtx& w) { body(w, M0{}); });
    if (mode == 1) {
      c.asm_pos_key = c.symb_key;
      c.asm_pos_cells = nc;
    }
    c.stats.assemble_positions_kept = mode == 2 ? 1 : 0;
    c.filled[PFV_MAT_SYSTEM] = true;
    return;
  }
#endif
  wave_for_g(env_int("PFV_ASM_G", 16), s, nc, lds, PFV_LAMBDA(const WaveCtx& w) {
    const int64_t cell = w.item;
    const int a0 = ap[cell], alen = ap[cell + 1] - a0;
    Carver cv(w.lds);
    double* acc = cv.take<double>(std::max(maxrow, 64));
    int32_t* aidx = cv.take<int32_t>(std::max(maxrow, 64));
    PFV_LANES(i, alen) {
      aidx[i] = ax[a0 + i];
      acc[i] = 0.0;
    }
    w.sync();
    for (int e = cf_ptr[cell]; e < cf_ptr[cell + 1]; ++e) {
      const int f = cf_idx[e];
      const double sg = (double)cf_sgn[e];
      const int p0 = ip[f], len = ip[f + 1] - p0;
      PFV_LANES(i, len) {
        const int pos = lower_bound_idx<int32_t>(aidx, alen, ix[p0 + i]);
        acc[pos] += sg * vq[p0 + i];
      }
      w.sync();
    }
    double mx = 0.0;
    PFV_LANES(i, alen) {
      Aval[a0 + i] = acc[i];
      if (aidx[i] == (int32_t)cell) diag[cell] = acc[i];
      else mx = fmax(mx, fabs(acc[i]));
    }
    w.lsync();           // every lane has read its accumulators: they become the scratch of the reduction
    double* red = acc;
    red[w.lane] = mx;
    w.lsync();
    if (w.lane0()) {
      double mm = 0.0;
      for (int l = 0; l < w.width; ++l) mm = fmax(mm, red[l]);
      rowmax[cell] = mm;
    }
    w.lsync();
  });
  c.filled[PFV_MAT_SYSTEM] = true;
}

// y = M x; one CSR row per group of L lanes on the device.  NT: matrix values / indices are
// streamed with non-temporal loads so that they do not evict x from the XCD's L2.
#ifndef PFV_EMULATE
// U: independent (index, value) loads a lane keeps in flight per trip.  The kernel is
// latency-bound on HBM unless every lane has several loads outstanding (Little's law:
// 2048 lanes/CU x 12 B x U in flight against ~2 us loaded latency).
template <int L, bool NT, int U>
__global__ void __launch_bounds__(256) k_spmv(int64_t nrows, const int32_t* __restrict__ indptr,
                                              const int32_t* __restrict__ indices,
                                              const double* __restrict__ val,
                                              const double* __restrict__ x, double* __restrict__ y) {
  const int lane = threadIdx.x % L;
  const int64_t rows_per_grid = (int64_t)gridDim.x * (256 / L);
  for (int64_t row = (int64_t)blockIdx.x * (256 / L) + threadIdx.x / L; row < nrows; row += rows_per_grid) {
    const int a = indptr[row], b = indptr[row + 1];
    double sum = 0.0;
    for (int p = a + lane; p < b; p += L * U) {
      int col[U];
      double v[U];
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const int pp = p + u * L;
        const bool ok = pp < b;
        const int pc = ok ? pp : a;  // clamp: always a valid address, contribution masked below
        col[u] = NT ? __builtin_nontemporal_load(indices + pc) : indices[pc];
        const double vv = NT ? __builtin_nontemporal_load(val + pc) : val[pc];
        v[u] = ok ? vv : 0.0;
      }
#pragma unroll
      for (int u = 0; u < U; ++u) sum += v[u] * x[col[u]];
    }
#pragma unroll
    for (int o = L / 2; o > 0; o >>= 1) sum += __shfl_down(sum, o, L);
    if (lane == 0) y[row] = sum;
  }
}
template <int L, bool NT>
static void launch_spmv(stream_t s, int64_t blocks, int64_t nrows, const int32_t* ip, const int32_t* ix,
                        const double* val, const double* x, double* y, int U) {
  switch (U) {
    case 1: PFV_LAUNCH(HIP_KERNEL_NAME(k_spmv<L, NT, 1>), dim3((unsigned)blocks), dim3(256), 0, s, nrows, ip, ix, val, x, y); break;
    case 2: PFV_LAUNCH(HIP_KERNEL_NAME(k_spmv<L, NT, 2>), dim3((unsigned)blocks), dim3(256), 0, s, nrows, ip, ix, val, x, y); break;
    case 3: PFV_LAUNCH(HIP_KERNEL_NAME(k_spmv<L, NT, 3>), dim3((unsigned)blocks), dim3(256), 0, s, nrows, ip, ix, val, x, y); break;
    case 5: PFV_LAUNCH(HIP_KERNEL_NAME(k_spmv<L, NT, 5>), dim3((unsigned)blocks), dim3(256), 0, s, nrows, ip, ix, val, x, y); break;
    case 6: PFV_LAUNCH(HIP_KERNEL_NAME(k_spmv<L, NT, 6>), dim3((unsigned)blocks), dim3(256), 0, s, nrows, ip, ix, val, x, y); break;
    default: PFV_LAUNCH(HIP_KERNEL_NAME(k_spmv<L, NT, 4>), dim3((unsigned)blocks), dim3(256), 0, s, nrows, ip, ix, val, x, y); break;
  }
}
#endif

static void spmv(pfv_ctx_impl& c, const CsrPattern& P, const double* val, const double* x, double* y) {
  stream_t s = c.stream;
  const int64_t nrows = P.nrows;
  if (nrows == 0) return;
  const int32_t* ip = P.indptr;
  const int32_t* ix = P.indices;
#ifdef PFV_EMULATE
  parallel_for(s, nrows, PFV_LAMBDA(int64_t r) {
    double sum = 0.0;
    for (int p = ip[r]; p < ip[r + 1]; ++p) sum += val[p] * x[ix[p]];
    y[r] = sum;
  });
#else
  const double avg = (double)P.nnz / (double)nrows;
  int L = 64;
  // measured on MI355X (tools/tune_spmv.py, 70 nnz/row): 16 lanes/row 3.74 TB/s, 32: 3.29, 8: 3.09
  if (avg <= 6) L = 4; else if (avg <= 20) L = 8; else if (avg <= 160) L = 16; else if (avg <= 512) L = 32;
  // tuning hooks (tools/tune_spmv.py): lanes per row, non-temporal matrix loads, grid cap
  const int envL = env_int("PFV_SPMV_L", 0), envNT = env_int("PFV_SPMV_NT", 0),
                   envCap = env_int("PFV_SPMV_BLOCKS", 0), envU = env_int("PFV_SPMV_U", 0);
  if (envL) L = envL;
  // loads in flight per lane: enough to cover a typical row in one trip (measured: U=1 3.7 TB/s,
  // U=5 4.6 TB/s at 70 nnz/row, 16 lanes/row)
  int U = envU ? envU : (int)std::ceil(1.1 * avg / L);
  U = std::max(1, std::min(6, U));
  const int rows_per_block = 256 / L;
  int64_t blocks = (nrows + rows_per_block - 1) / rows_per_block;
  if (envCap > 0 && blocks > envCap) blocks = envCap;
  if (envNT) {
    switch (L) {
      case 4: launch_spmv<4, true>(s, blocks, nrows, ip, ix, val, x, y, U); break;
      case 8: launch_spmv<8, true>(s, blocks, nrows, ip, ix, val, x, y, U); break;
      case 16: launch_spmv<16, true>(s, blocks, nrows, ip, ix, val, x, y, U); break;
      case 32: launch_spmv<32, true>(s, blocks, nrows, ip, ix, val, x, y, U); break;
      default: launch_spmv<64, true>(s, blocks, nrows, ip, ix, val, x, y, U); break;
    }
  } else {
    switch (L) {
      case 4: launch_spmv<4, false>(s, blocks, nrows, ip, ix, val, x, y, U); break;
      case 8: launch_spmv<8, false>(s, blocks, nrows, ip, ix, val, x, y, U); break;
      case 16: launch_spmv<16, false>(s, blocks, nrows, ip, ix, val, x, y, U); break;
      case 32: launch_spmv<32, false>(s, blocks, nrows, ip, ix, val, x, y, U); break;
      default: launch_spmv<64, false>(s, blocks, nrows, ip, ix, val, x, y, U); break;
    }
  }
  PFV_HIP_CHECK(hipGetLastError());
#endif
}

// y = V x for V = vector_source / bound_pressure_vector_source addressed THROUGH the flux pattern (c.vs_implicit: the
// matrices have >= 2^31 entries, their own CSR arrays do not exist): entry p of flux row f, component k, is value nd p + k
// in column nd c_p + k.  One wavefront-quarter per row, products summed in the order of the explicit CSR row.
static void spmv_vs_implicit(pfv_ctx_impl& c, const double* val, const double* x, double* y) {
  stream_t s = c.stream;
  const int nd = c.nd;
  const int32_t* ip = c.pat_flux.indptr;
  const int32_t* ix = c.pat_flux.indices;
  wave_for<16>(s, c.nf, 16 * sizeof(double) + 16, PFV_LAMBDA(const WaveCtx& w) {
    const int64_t f = w.item;
    const int p0 = ip[f], len = ip[f + 1] - p0;
    double acc = 0.0;
    PFV_LANES(q, len * nd) {
      const int p = q / nd, k = q - p * nd;
      acc += val[(int64_t)(p0 + p) * nd + k] * x[(int64_t)ix[p0 + p] * nd + k];
    }
    double* sh = reinterpret_cast<double*>(w.lds);
    sh[w.lane] = acc;
    w.sync();
    if (w.lane0()) {
      double sum = 0.0;
      for (int j = 0; j < w.width; ++j) sum += sh[j];
      y[f] = sum;
    }
    w.sync();
  });
}
// the product with one of the two vector-source matrices, explicit or implicit pattern
static void spmv_vs(pfv_ctx_impl& c, int which, const double* x, double* y) {
  if (c.vs_implicit) {
    spmv_vs_implicit(c, c.val[which], x, y);
  } else {
    ensure_vs_indices(c);
    spmv(c, c.pat_vs, c.val[which], x, y);
  }
}

// b = source - div (bound_flux bc + vector_source g)
static void assemble_rhs(pfv_ctx_impl& c, const double* d_bc, const double* d_vs, const double* d_src) {
  stream_t s = c.stream;
  const int64_t nc = c.nc, nf = c.nf;
  double* ft = c.face_tmp.ensure(nf);
  double* ft2 = nullptr;
  spmv(c, c.pat_bound, c.val[PFV_MAT_BOUND_FLUX], d_bc, ft);
  Buf<double> tmp2;
  if (d_vs) {
    ft2 = tmp2.ensure(nf);
    spmv_vs(c, PFV_MAT_VECTOR_SOURCE, d_vs, ft2);
  }
  double* b = c.rhs.ensure(nc);
  const int32_t* cf_ptr = c.cf_ptr;
  const int32_t* cf_idx = c.cf_idx;
  const int8_t* cf_sgn = c.cf_sgn;
  parallel_for(s, nc, PFV_LAMBDA(int64_t cell) {
    double acc = d_src ? d_src[cell] : 0.0;
    for (int e = cf_ptr[cell]; e < cf_ptr[cell + 1]; ++e) {
      const int f = cf_idx[e];
      double t = ft[f];
      if (ft2) t += ft2[f];
      acc -= (double)cf_sgn[e] * t;
    }
    b[cell] = acc;
  });
  be_sync(s);  // tmp2 is freed on return
}


// ---------------------------------------------------------------------------- Krylov
// All Krylov scalars live in HBM (array S); every reduction ends with a small scalar update
// ("mode") so the host never touches them inside the iteration.
enum { S_RHO = 0, S_RHO_OLD, S_ALPHA, S_OMEGA, S_BETA, S_RV, S_TS, S_TT, S_RR, S_BB, S_RAW0, S_RAW1, S_COUNT = 16 };
enum { M_BB = 0, M_START = 1, M_ALPHA = 2, M_OMEGA = 3, M_RHO_BETA = 4, M_CG_ALPHA = 5, M_CG_BETA = 6,
       M_RAW = 7 /* sharded solve: keep this rank's sums; the update follows the all-reduce */ };

PFV_HD inline void apply_scalar_mode(double* S, double a, double b, int mode) {
  switch (mode) {
    case M_BB:  // a = (b,b)
      S[S_BB] = a;
      break;
    case M_START:  // a = (r,r), b = (rhat,r) [BiCGStab] or (r,z) [CG]
      S[S_RR] = a;
      S[S_RHO] = b;
      S[S_RHO_OLD] = 1.0;
      S[S_ALPHA] = 1.0;
      S[S_OMEGA] = 1.0;
      S[S_BETA] = 0.0;
      break;
    case M_ALPHA:  // a = (rhat, v): alpha = rho / (rhat,v)
      S[S_RV] = a;
      S[S_ALPHA] = S[S_RHO] / a;
      break;
    case M_OMEGA:  // a = (t,s), b = (t,t)
      S[S_TS] = a;
      S[S_TT] = b;
      S[S_OMEGA] = (b != 0.0) ? a / b : 0.0;
      break;
    case M_RHO_BETA:  // a = (r,r), b = (rhat, r): next rho and beta
      S[S_RR] = a;
      S[S_RHO_OLD] = S[S_RHO];
      S[S_RHO] = b;
      S[S_BETA] = (b / S[S_RHO_OLD]) * (S[S_ALPHA] / S[S_OMEGA]);
      break;
    case M_CG_ALPHA:  // a = (p, Ap)
      S[S_ALPHA] = S[S_RHO] / a;
      break;
    case M_CG_BETA:  // a = (r,r), b = (r,z)
      S[S_RR] = a;
      S[S_BETA] = b / S[S_RHO];
      S[S_RHO] = b;
      break;
    case M_RAW:
      S[S_RAW0] = a;
      S[S_RAW1] = b;
      break;
    default:
      break;
  }
}

constexpr int kRedBlocks = 2048;  // partial sums per accumulator (fixed -> deterministic order)

struct Reduce {
  double* partial;  // [2 * stride]: one partial per producing block and accumulator
  int64_t stride;
  double* S;
};

#ifdef PFV_EMULATE
// portable two-stage form (what the host emulation runs)
static void dot_partials(pfv_ctx_impl& c, int64_t n, const double* x, const double* y, const double* x2,
                         const double* y2, double* partial, int64_t stride) {
  wave_for(c.stream, kRedBlocks, 64 * 16 + 16, PFV_LAMBDA(const WaveCtx& w) {
    double* p1 = reinterpret_cast<double*>(w.lds);
    double* p2 = p1 + 64;
    PFV_LANES(l, 64) {
      double a = 0.0, b = 0.0;
      for (int64_t i = w.item * 64 + l; i < n; i += (int64_t)kRedBlocks * 64) {
        a += x[i] * y[i];
        if (x2) b += x2[i] * y2[i];
      }
      p1[l] = a;
      p2[l] = b;
    }
    w.sync();
    if (w.lane0()) {
      double a = 0.0, b = 0.0;
      for (int l = 0; l < 64; ++l) { a += p1[l]; b += p2[l]; }
      partial[w.item] = a;
      partial[stride + w.item] = b;
    }
  });
}
static void finalize_scalars(pfv_ctx_impl& c, const double* partial, int64_t stride, double* S, int mode) {
  parallel_for(c.stream, 1, PFV_LAMBDA(int64_t) {
    double a = 0.0, b = 0.0;
    for (int i = 0; i < kRedBlocks; ++i) { a += partial[i]; b += partial[stride + i]; }
    apply_scalar_mode(S, a, b, mode);
  });
}
#else
// ---- device: reductions fused into the producing kernel; the last block to arrive (agent-scope
// release / ticket / acquire, MI355X guide G16) sums the partials in a fixed order and applies
// the scalar update, so no separate reduction launches exist.
__device__ __forceinline__ double block_sum(double v, double* sm) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) sm[threadIdx.x >> 6] = v;
  __syncthreads();
  double t = 0.0;
  if (threadIdx.x == 0)
    for (int i = 0; i < (int)(blockDim.x >> 6); ++i) t += sm[i];
  return t;
}
// Every block leaves its two partial sums; a one-block kernel then adds them in a fixed order and
// applies the scalar update.  (A fused "last block finalizes" variant with agent-scope
// release/ticket/acquire was measured at +160 us per SpMV on MI355X - 2048 L2 write-back fences
// and same-address tickets - versus ~8 us for this extra launch.)
__device__ __forceinline__ void reduce_finalize(double a, double b, const Reduce& R, int mode) {
  __shared__ double sm[16];
  (void)mode;
  const double sa = block_sum(a, sm);
  const double sb = block_sum(b, sm);
  if (threadIdx.x == 0) {
    R.partial[blockIdx.x] = sa;
    R.partial[R.stride + blockIdx.x] = sb;
  }
}
__device__ __forceinline__ void reduce_finalize_slot(double a, double b, const Reduce& R, unsigned slot) {
  __shared__ double sm[16];
  const double sa = block_sum(a, sm);
  const double sb = block_sum(b, sm);
  if (threadIdx.x == 0) {
    R.partial[slot] = sa;
    R.partial[R.stride + slot] = sb;
  }
}
__global__ void __launch_bounds__(1024) k_finalize(int nblocks, Reduce R, int mode) {
  __shared__ double sm[16];
  double x = 0.0, y = 0.0;
  for (int i = threadIdx.x; i < nblocks; i += blockDim.x) {
    x += R.partial[i];
    y += R.partial[R.stride + i];
  }
  x = block_sum(x, sm);
  y = block_sum(y, sm);
  if (threadIdx.x == 0) apply_scalar_mode(R.S, x, y, mode);
}
// first stage for long partial arrays (one partial per SpMV block): 128 blocks, contiguous chunks
__global__ void __launch_bounds__(256) k_reduce_stage(int nblocks, Reduce R, Reduce R2) {
  __shared__ double sm[16];
  const int chunk = (nblocks + (int)gridDim.x - 1) / (int)gridDim.x;
  const int lo = blockIdx.x * chunk, hi = min(nblocks, lo + chunk);
  double x = 0.0, y = 0.0;
  for (int i = lo + threadIdx.x; i < hi; i += blockDim.x) {
    x += R.partial[i];
    y += R.partial[R.stride + i];
  }
  x = block_sum(x, sm);
  y = block_sum(y, sm);
  if (threadIdx.x == 0) {
    R2.partial[blockIdx.x] = x;
    R2.partial[R2.stride + blockIdx.x] = y;
  }
}
static void launch_finalize(stream_t s, int nblocks, const Reduce& R, int mode) {
  if (nblocks > 4096) {
    Reduce R2 = R;
    R2.partial = R.partial + 2 * R.stride + S_COUNT;  // 2 x 128 doubles behind the scalars
    R2.stride = 128;
    PFV_LAUNCH(k_reduce_stage, dim3(128), dim3(256), 0, s, nblocks, R, R2);
    PFV_LAUNCH(k_finalize, dim3(1), dim3(128), 0, s, 128, R2, mode);
  } else {
    PFV_LAUNCH(k_finalize, dim3(1), dim3(1024), 0, s, nblocks, R, mode);
  }
}

// y = A x with optional fused dots: DOT 1: a = (w, y); DOT 2: a = (y, w), b = (y, y)
template <int L, int U, int DOT>
__global__ void __launch_bounds__(256) k_spmv_dot(int64_t nrows, const int32_t* __restrict__ indptr,
                                                  const int32_t* __restrict__ indices,
                                                  const double* __restrict__ val, const double* __restrict__ x,
                                                  double* __restrict__ y, const double* __restrict__ w,
                                                  Reduce R, int mode) {
  const int lane = threadIdx.x % L;
  const int64_t rows_per_grid = (int64_t)gridDim.x * (256 / L);
  double acc1 = 0.0, acc2 = 0.0;
  for (int64_t row = (int64_t)blockIdx.x * (256 / L) + threadIdx.x / L; row < nrows; row += rows_per_grid) {
    const int a = indptr[row], b = indptr[row + 1];
    const double wrow = (lane == 0) ? w[row] : 0.0;  // issued with the matrix loads, not after them
    double sum = 0.0;
    for (int p = a + lane; p < b; p += L * U) {
      int col[U];
      double v[U];
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const int pp = p + u * L;
        const bool ok = pp < b;
        const int pc = ok ? pp : a;
        col[u] = indices[pc];
        const double vv = val[pc];
        v[u] = ok ? vv : 0.0;
      }
#pragma unroll
      for (int u = 0; u < U; ++u) sum += v[u] * x[col[u]];
    }
#pragma unroll
    for (int o = L / 2; o > 0; o >>= 1) sum += __shfl_down(sum, o, L);
    if (lane == 0) {
      y[row] = sum;
      if (DOT == 1) acc1 += wrow * sum;
      if (DOT == 2) { acc1 += sum * wrow; acc2 += sum * sum; }
    }
  }
  reduce_finalize(acc1, acc2, R, mode);
}

// a = sum x1*y1, b = sum x2*y2 (x2 may be null)
__global__ void __launch_bounds__(256) k_dot2(int64_t n, const double* __restrict__ x1, const double* __restrict__ y1,
                                              const double* __restrict__ x2, const double* __restrict__ y2,
                                              Reduce R, int mode) {
  double a = 0.0, b = 0.0;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
    a += x1[i] * y1[i];
    if (x2) b += x2[i] * y2[i];
  }
  reduce_finalize(a, b, R, mode);
}

// BiCGStab tail: x += alpha y + omega z; r = s - omega t; a = (r,r), b = (rhat,r)
__global__ void __launch_bounds__(256) k_bicg_tail(int64_t n, double* __restrict__ x, double* __restrict__ r,
                                                   const double* __restrict__ y, const double* __restrict__ z,
                                                   const double* __restrict__ t, const double* __restrict__ rhat,
                                                   Reduce R, int mode) {
  const double alpha = R.S[S_ALPHA], omega = R.S[S_OMEGA];
  double a = 0.0, b = 0.0;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
    x[i] += alpha * y[i] + omega * z[i];
    const double ri = r[i] - omega * t[i];
    r[i] = ri;
    a += ri * ri;
    b += rhat[i] * ri;
  }
  reduce_finalize(a, b, R, mode);
}

// CG tail: x += alpha p; r -= alpha v; z = r / diag; a = (r,r), b = (r,z)
__global__ void __launch_bounds__(256) k_cg_tail(int64_t n, double* __restrict__ x, double* __restrict__ r,
                                                 double* __restrict__ z, const double* __restrict__ p,
                                                 const double* __restrict__ v, const double* __restrict__ diag,
                                                 Reduce R, int mode) {
  const double alpha = R.S[S_ALPHA];
  double a = 0.0, b = 0.0;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
    x[i] += alpha * p[i];
    const double ri = r[i] - alpha * v[i];
    const double zi = ri / diag[i];
    r[i] = ri;
    z[i] = zi;
    a += ri * ri;
    b += ri * zi;
  }
  reduce_finalize(a, b, R, mode);
}

template <int L, int DOT>
static void launch_spmv_dot_u(stream_t s, int blocks, int U, int64_t nrows, const int32_t* ip, const int32_t* ix,
                              const double* val, const double* x, double* y, const double* w, Reduce R, int mode) {
#define PFV_SPMV_DOT_CASE(UU)                                                                                \
  case UU:                                                                                                   \
    PFV_LAUNCH(HIP_KERNEL_NAME(k_spmv_dot<L, UU, DOT>), dim3(blocks), dim3(256), 0, s, nrows, ip, ix, \
                       val, x, y, w, R, mode);                                                               \
    break;
  switch (U) {
    PFV_SPMV_DOT_CASE(1)
    PFV_SPMV_DOT_CASE(2)
    PFV_SPMV_DOT_CASE(3)
    PFV_SPMV_DOT_CASE(4)
    PFV_SPMV_DOT_CASE(5)
    default:
      PFV_LAUNCH(HIP_KERNEL_NAME(k_spmv_dot<L, 6, DOT>), dim3(blocks), dim3(256), 0, s, nrows, ip, ix, val,
                         x, y, w, R, mode);
      break;
  }
#undef PFV_SPMV_DOT_CASE
}
#endif

}  // namespace pfv
#include "spmv_win.inc"
#include "amg.inc"
#include "amg_nns.inc"
namespace pfv {

// ---- sharded BiCGStab with merged reductions.  The textbook iteration has three global synchronisation points,
// (rhat, v) | (t, s), (t, t) | (r, r), (rhat, r) -- at 250 k cells per GPU each of them is a latency-bound all-reduce
// as long as the iteration's SpMV.  The third follows from sums that can be formed together with the second
// (r_new = s - omega t):   (rhat, r_new) = (rhat, s) - omega (rhat, t),   (r_new, r_new) = (s, s) - 2 omega (t, s)
// + omega^2 (t, t).  So the sharded loop reduces FIVE sums in its second all-reduce and none after the vector update:
// two all-reduces per iteration instead of three (SURVEY 8(e): "fuse into one reduction"; the remaining one, (rhat, v),
// needs v = A M^-1 p first).  The five partial sums: one pass over t, s, rhat in fixed blocks, partials added in
// block order (deterministic).
constexpr int kDot5Blocks = 512;
static void shard_dot5(pfv_ctx_impl& c, int64_t n, const double* t, const double* sv, const double* rhat,
                       double* partial /* [5 * kDot5Blocks] */, double* out5) {
  stream_t s = c.stream;
  const int nb = (int)std::min<int64_t>(kDot5Blocks, (n + 1023) / 1024);
  block_for<256>(s, nb, 256 * sizeof(double), PFV_LAMBDA(const WaveCtx& wc) {
    double* sh = reinterpret_cast<double*>(wc.lds);
    const int64_t b = wc.item;
    const int64_t lo = n * b / nb, hi = n * (b + 1) / nb;
    double acc[5] = {0.0, 0.0, 0.0, 0.0, 0.0};
    for (int64_t i = lo + wc.lane; i < hi; i += wc.width) {
      const double ti = t[i], si = sv[i], hi_ = rhat[i];
      acc[0] += ti * si;
      acc[1] += ti * ti;
      acc[2] += si * si;
      acc[3] += hi_ * si;
      acc[4] += hi_ * ti;
    }
    for (int k = 0; k < 5; ++k) {
      sh[wc.lane] = acc[k];
      wc.sync();
      for (int o = wc.width >> 1; o > 0; o >>= 1) {
        if (wc.lane < o) sh[wc.lane] += sh[wc.lane + o];
        wc.sync();
      }
      if (wc.lane0()) partial[(int64_t)k * nb + b] = sh[0];
      wc.sync();
    }
  });
  parallel_for(s, 5, PFV_LAMBDA(int64_t k) {
    double a = 0.0;
    for (int i = 0; i < nb; ++i) a += partial[k * nb + i];
    out5[k] = a;
  });
}
// omega, the next rho / beta and the recursive residual norm from the five global sums
PFV_HD inline void apply_merged_omega(double* S, const double* g) {
  const double ts = g[0], tt = g[1], ss = g[2], hs = g[3], ht = g[4];
  const double om = (tt != 0.0) ? ts / tt : 0.0;
  S[S_TS] = ts;
  S[S_TT] = tt;
  S[S_OMEGA] = om;
  const double rr = ss - 2.0 * om * ts + om * om * tt;
  S[S_RR] = rr > 0.0 ? rr : 0.0;  // (cancellation near convergence can leave a tiny negative value)
  const double rho_new = hs - om * ht;
  S[S_RHO_OLD] = S[S_RHO];
  S[S_RHO] = rho_new;
  S[S_BETA] = (rho_new / S[S_RHO_OLD]) * (S[S_ALPHA] / om);
}

// ---- sharded solve (pfv_solve_sharded): the caller's hooks
static void shard_halo(pfv_ctx_impl& c, double* x) {
  if (!c.shard) return;
  if (c.shard->exchange_halo(c.shard->user, x, (void*)(intptr_t)c.stream))
    throw Error(PFV_ERR_ARGUMENT, "exchange_halo hook failed");
}

static void finish_reduction(pfv_ctx_impl& c, int nblocks, const Reduce& R, int mode);
static void spmv_dot(pfv_ctx_impl& c, const CsrPattern& P, const double* val, const double* x, double* y,
                     const double* w, int dot, const Reduce& R, int mode, const WinCsr* W = nullptr);

// y = A x of a sharded solve, the halo entries of x fetched on the way.  Default: exchange, then the product.
// PFV_SHARD_OVERLAP (native RCCL transport only): the exchange runs on the handle's second stream while the row blocks
// whose windows hold no halo column are multiplied; the others follow once it has landed -- at 250 k cells per GPU the
// exchange (~15-20 us over xGMI) is as long as half the product (SURVEY 8(e): "overlap with interior SpMV").  Every row
// block keeps its slot of the reduction partials, so the sums do not depend on the split.
static void shard_spmv(pfv_ctx_impl& c, const CsrPattern& P, const double* val, double* x, double* y, const double* w,
                       int dot, const Reduce& R, int mode, const WinCsr* W) {
#ifndef PFV_EMULATE
  if (c.shard && c.shard_overlap && W && W->ok && c.aux_stream) {
    {
      StreamFork fork(c.stream, c.aux_stream);  // the exchange waits for everything that wrote x
      if (c.shard->exchange_halo(c.shard->user, x, (void*)(intptr_t)c.aux_stream))
        throw Error(PFV_ERR_ARGUMENT, "exchange_halo hook failed");
      const int32_t* li = c.shard_blocks.p;
      if (dot == 0) spmv_win<double, 0>(c, P, *W, val, x, y, nullptr, nullptr, 0.0, R, li, c.shard_n_interior);
      else if (dot == 1) spmv_win<double, 2>(c, P, *W, val, x, y, w, nullptr, 0.0, R, li, c.shard_n_interior);
      else spmv_win<double, 3>(c, P, *W, val, x, y, w, nullptr, 0.0, R, li, c.shard_n_interior);
      fork.join();                               // the boundary blocks wait for the halo entries
    }
    const int32_t* lb = c.shard_blocks.p + c.shard_n_interior;
    if (dot == 0) spmv_win<double, 0>(c, P, *W, val, x, y, nullptr, nullptr, 0.0, R, lb, c.shard_n_boundary);
    else if (dot == 1) spmv_win<double, 2>(c, P, *W, val, x, y, w, nullptr, 0.0, R, lb, c.shard_n_boundary);
    else spmv_win<double, 3>(c, P, *W, val, x, y, w, nullptr, 0.0, R, lb, c.shard_n_boundary);
    if (dot) finish_reduction(c, (int)W->nblk, R, mode);
    return;
  }
#endif
  shard_halo(c, x);
  spmv_dot(c, P, val, x, y, w, dot, R, mode, W);
}

// Second stage of every two-accumulator reduction: the block partials are summed in a fixed order and
// the scalar update `mode` is applied on the device.  In a sharded solve the rank's sums first go
// through the caller's all-reduce (one call for the pair), then the update runs on the global sums.
static void finish_reduction(pfv_ctx_impl& c, int nblocks, const Reduce& R, int mode) {
  const int m1 = c.shard ? (int)M_RAW : mode;
#ifdef PFV_EMULATE
  (void)nblocks;
  finalize_scalars(c, R.partial, R.stride, R.S, m1);
#else
  launch_finalize(c.stream, nblocks, R, m1);
#endif
  if (c.shard) {
    double* raw = c.shard_work + 2 * c.shard_nloc;
    double* S = R.S;
    be_d2d(raw, S + S_RAW0, 2 * sizeof(double), c.stream);
    if (c.shard->allreduce_sum(c.shard->user, raw, 2, (void*)(intptr_t)c.stream))
      throw Error(PFV_ERR_ARGUMENT, "allreduce_sum hook failed");
    parallel_for(c.stream, 1, PFV_LAMBDA(int64_t) { apply_scalar_mode(S, raw[0], raw[1], mode); });
  }
}

// y = A x, then (optionally) a fused reduction and scalar update.  dot: 0 none, 1 (w,y), 2 (y,w),(y,y)
static void spmv_dot(pfv_ctx_impl& c, const CsrPattern& P, const double* val, const double* x, double* y,
                     const double* w, int dot, const Reduce& R, int mode, const WinCsr* W) {
#ifdef PFV_EMULATE
  (void)W;
  spmv(c, P, val, x, y);
  if (dot == 1) dot_partials(c, P.nrows, w, y, nullptr, nullptr, R.partial, R.stride);
  if (dot == 2) dot_partials(c, P.nrows, y, w, y, y, R.partial, R.stride);
  if (dot) finish_reduction(c, 0, R, mode);
#else
  if (W && W->ok) {
    if (dot == 0) spmv_win<double, 0>(c, P, *W, val, x, y, nullptr, nullptr, 0.0, R);
    else if (dot == 1) spmv_win<double, 2>(c, P, *W, val, x, y, w, nullptr, 0.0, R);
    else spmv_win<double, 3>(c, P, *W, val, x, y, w, nullptr, 0.0, R);
    if (dot) finish_reduction(c, (int)W->nblk, R, mode);
    return;
  }
  if (dot == 0) {
    spmv(c, P, val, x, y);
    return;
  }
  stream_t s = c.stream;
  const int64_t nrows = P.nrows;
  const double avg = (double)P.nnz / (double)nrows;
  const int L = avg <= 20 ? 8 : (avg <= 160 ? 16 : 32);
  int U = (int)std::ceil(1.1 * avg / L);
  U = std::max(1, std::min(6, U));
  const int64_t groups = (nrows + 256 / L - 1) / (256 / L);
  const int blocks = (int)groups;  // one row group per block: the hardware overlaps blocks, a grid-stride loop does not
  if (L == 8) {
    if (dot == 1) launch_spmv_dot_u<8, 1>(s, blocks, U, nrows, P.indptr, P.indices, val, x, y, w, R, mode);
    else launch_spmv_dot_u<8, 2>(s, blocks, U, nrows, P.indptr, P.indices, val, x, y, w, R, mode);
  } else if (L == 16) {
    if (dot == 1) launch_spmv_dot_u<16, 1>(s, blocks, U, nrows, P.indptr, P.indices, val, x, y, w, R, mode);
    else launch_spmv_dot_u<16, 2>(s, blocks, U, nrows, P.indptr, P.indices, val, x, y, w, R, mode);
  } else {
    if (dot == 1) launch_spmv_dot_u<32, 1>(s, blocks, U, nrows, P.indptr, P.indices, val, x, y, w, R, mode);
    else launch_spmv_dot_u<32, 2>(s, blocks, U, nrows, P.indptr, P.indices, val, x, y, w, R, mode);
  }
  finish_reduction(c, blocks, R, mode);
  PFV_HIP_CHECK(hipGetLastError());
#endif
}

// y = A x for a system (windowed kernel when pfv_solve has built the window)
static void sys_spmv(pfv_ctx_impl& c, const LinSys& sys, const double* x, double* y) {
#ifndef PFV_EMULATE
  if (sys.win && sys.win->ok) {
    Reduce R{};
    spmv_win<double, 0>(c, *sys.P, *sys.win, sys.val, x, y, nullptr, nullptr, 0.0, R);
    return;
  }
#endif
  spmv(c, *sys.P, sys.val, x, y);
}

static void dot2(pfv_ctx_impl& c, int64_t n, const double* x1, const double* y1, const double* x2,
                 const double* y2, const Reduce& R, int mode) {
#ifdef PFV_EMULATE
  dot_partials(c, n, x1, y1, x2, y2, R.partial, R.stride);
  finish_reduction(c, 0, R, mode);
#else
  const int blocks = (int)std::min<int64_t>((n + 255) / 256, kRedBlocks);
  PFV_LAUNCH(k_dot2, dim3(blocks), dim3(256), 0, c.stream, n, x1, y1, x2, y2, R, mode);
  finish_reduction(c, blocks, R, mode);
  PFV_HIP_CHECK(hipGetLastError());
#endif
}

struct SolveResult {
  int iterations = 0;
  bool converged = false;
  double relres = 0.0;
};

// M == nullptr: Jacobi, fused into the vector kernels; otherwise the preconditioner is applied
// between them (its cost dwarfs the un-fused vector updates)
static SolveResult krylov_solve(pfv_ctx_impl& c, const LinSys& sys, int method, double rtol, int maxit,
                                double* d_x, bool x_is_zero, const Precond* M = nullptr) {
  stream_t s = c.stream;
  const int64_t n = sys.n;
  const CsrPattern& P = *sys.P;
  const double* Aval = sys.val;
  const double* diag = sys.diag;
  const double* d_b = sys.rhs;
  double* r = c.kry[0].ensure(n);
  double* rhat = c.kry[1].ensure(n);
  // sharded solve: the SpMV inputs carry the halo entries behind the owned ones and live in the
  // caller's work space (BiCGStab: y and z; CG: p), so that the exchange hook can address them
  const bool sharded = c.shard != nullptr;
  const bool sh_cg = sharded && method == PFV_SOLVE_CG;
  double* p = sh_cg ? c.shard_work : c.kry[2].ensure(n);
  double* v = c.kry[3].ensure(n);
  double* y = (sharded && !sh_cg) ? c.shard_work : c.kry[4].ensure(n);
  double* z = sharded ? c.shard_work + c.shard_nloc : c.kry[5].ensure(n);
  double* t = c.kry[6].ensure(n);
  Reduce R;
  R.stride = std::max<int64_t>(kRedBlocks, n / 8 + 2);  // >= row groups of the widest SpMV grid
  double* red = c.red.ensure(2 * R.stride + S_COUNT + 2 * 128);
  R.partial = red;
  R.S = red + 2 * R.stride;
  double* S = R.S;
  // (sharded: every rank must take the same branches, and n is the rank's own size -- test every iteration)
  // Sharded: the test reads the all-reduced residual, the same number on every rank, so every rank takes the same
  // branch whatever the interval; reading it every iteration would drain the stream once per iteration -- at 250 k
  // cells per GPU the ~60 launches of an iteration then run at host launch rate instead of queueing behind each other.
  const int merged = (sharded && method == PFV_SOLVE_BICGSTAB && env_int("PFV_SHARD_MERGED_DOTS", 1) != 0) ? 1 : 0;
  const int check_every = sharded ? std::max(1, env_int("PFV_SHARD_CHECK_EVERY", 4)) : ((M || n < 200000) ? 1 : 10);
  SolveResult res;

  // r = b - A x
  if (x_is_zero) {
    be_d2d(r, d_b, sizeof(double) * n, s);
  } else {
    if (sharded) throw Error(PFV_ERR_ARGUMENT, "a sharded solve starts from zero");
    sys_spmv(c, sys, d_x, t);
    parallel_for(s, n, PFV_LAMBDA(int64_t i) { r[i] = d_b[i] - t[i]; });
  }
  dot2(c, n, d_b, d_b, nullptr, nullptr, R, M_BB);
  const double bb = read_scalar<double>(s, S + S_BB);
  if (!(bb > 0.0)) {  // b = 0 -> x = 0
    be_memset(d_x, 0, sizeof(double) * n, s);
    res.converged = true;
    return res;
  }
  const double tol2 = rtol * rtol * bb;

  if (method == PFV_SOLVE_CG) {
    if (M) {
      precond_apply(c, *M, n, r, z);
      be_d2d(p, z, sizeof(double) * n, s);
    } else {
      parallel_for(s, n, PFV_LAMBDA(int64_t i) {
        const double zi = r[i] / diag[i];
        z[i] = zi;
        p[i] = zi;
      });
    }
    dot2(c, n, r, r, r, z, R, M_START);
    for (int it = 1; it <= maxit; ++it) {
      shard_halo(c, p);
      spmv_dot(c, P, Aval, p, v, p, 1, R, M_CG_ALPHA, sys.win);  // (p, Ap)
      if (M) {
        parallel_for(s, n, PFV_LAMBDA(int64_t i) {
          const double al = S[S_ALPHA];
          d_x[i] += al * p[i];
          r[i] -= al * v[i];
        });
        precond_apply(c, *M, n, r, z);
        dot2(c, n, r, r, r, z, R, M_CG_BETA);
      } else {
#ifdef PFV_EMULATE
      parallel_for(s, n, PFV_LAMBDA(int64_t i) {
        const double al = S[S_ALPHA];
        d_x[i] += al * p[i];
        const double ri = r[i] - al * v[i];
        r[i] = ri;
        z[i] = ri / diag[i];
      });
      dot2(c, n, r, r, r, z, R, M_CG_BETA);
#else
      {
        const int blocks = (int)std::min<int64_t>((n + 255) / 256, kRedBlocks);
        PFV_LAUNCH(k_cg_tail, dim3(blocks), dim3(256), 0, s, n, d_x, r, z, p, v, diag, R, (int)M_CG_BETA);
        finish_reduction(c, blocks, R, M_CG_BETA);
      }
#endif
      }
      parallel_for(s, n, PFV_LAMBDA(int64_t i) { p[i] = z[i] + S[S_BETA] * p[i]; });
      res.iterations = it;
      if (it % check_every == 0 || it == maxit) {
        const double rr = read_scalar<double>(s, S + S_RR);
        res.relres = std::sqrt(rr / bb);
        if (rr <= tol2) { res.converged = true; break; }
        if (!(rr == rr)) break;  // NaN: breakdown
      }
    }
    return res;
  }

  // BiCGStab, right-preconditioned.  The loop stops on the RECURSIVE residual; at tolerances near
  // 1e-13 that one keeps falling after the true residual b - A x has stalled at the rounding level of
  // the updates.  So, outside sharded solves: once the recursive residual has converged, the true
  // residual is computed and, if it misses the tolerance, the iteration restarts from the current x
  // with r = b - A x (at most kTrueResidualRestarts times) -- the reported residual is the true one.
  constexpr int kTrueResidualRestarts = 3;
  int restarts = 0;
  int it = 1;
  // plain AMG on its AP path: the first smoothing step of the cycle's finest level, x0 = omega_0 D_0^-1 in, is written
  // by the update that forms `in` (the vector is in registers there; the cycle's own launch read it back), the same
  // expression on the same numbers
  const double* dinv0 = nullptr;
  double omega0 = 0.0;
  const bool presmooth = M && !sharded && precond_presmooth(*M, dinv0, omega0);
restart_bicgstab:
  be_d2d(rhat, r, sizeof(double) * n, s);
  be_memset(p, 0, sizeof(double) * n, s);
  be_memset(v, 0, sizeof(double) * n, s);
  dot2(c, n, r, r, rhat, r, R, M_START);
  for (; it <= maxit; ++it) {
    // p = r + beta (p - omega v); y = M^-1 p
    if (presmooth) {
      parallel_for(s, n, PFV_LAMBDA(int64_t i) {
        const double pi = r[i] + S[S_BETA] * (p[i] - S[S_OMEGA] * v[i]);
        p[i] = pi;
        y[i] = omega0 * dinv0[i] * pi;
      });
      amg_cycle(c, *M->amg, 0, p, y, true);
    } else if (M) {
      parallel_for(s, n, PFV_LAMBDA(int64_t i) { p[i] = r[i] + S[S_BETA] * (p[i] - S[S_OMEGA] * v[i]); });
      precond_apply(c, *M, n, p, y);
    } else {
      parallel_for(s, n, PFV_LAMBDA(int64_t i) {
        const double pi = r[i] + S[S_BETA] * (p[i] - S[S_OMEGA] * v[i]);
        p[i] = pi;
        y[i] = pi / diag[i];
      });
    }
    shard_spmv(c, P, Aval, y, v, rhat, 1, R, M_ALPHA, sys.win);  // v = A y, alpha = rho / (rhat, v)
    // s = r - alpha v (stored in r); z = M^-1 s
    if (presmooth) {
      parallel_for(s, n, PFV_LAMBDA(int64_t i) {
        const double si = r[i] - S[S_ALPHA] * v[i];
        r[i] = si;
        z[i] = omega0 * dinv0[i] * si;
      });
      amg_cycle(c, *M->amg, 0, r, z, true);
    } else if (M) {
      parallel_for(s, n, PFV_LAMBDA(int64_t i) { r[i] -= S[S_ALPHA] * v[i]; });
      precond_apply(c, *M, n, r, z);
    } else {
      parallel_for(s, n, PFV_LAMBDA(int64_t i) {
        const double si = r[i] - S[S_ALPHA] * v[i];
        r[i] = si;
        z[i] = si / diag[i];
      });
    }
    if (merged) {
      // t = A z; the five sums in one all-reduce; omega, rho, beta, (r,r) on the device; the vector update needs no
      // reduction of its own
      shard_spmv(c, P, Aval, z, t, r, 0, R, M_OMEGA, sys.win);
      double* raw = c.shard_work + 2 * c.shard_nloc;
      shard_dot5(c, n, t, r, rhat, c.red5.ensure(5 * kDot5Blocks), raw);
      if (c.shard->allreduce_sum(c.shard->user, raw, 5, (void*)(intptr_t)c.stream))
        throw Error(PFV_ERR_ARGUMENT, "allreduce_sum hook failed");
      parallel_for(s, 1, PFV_LAMBDA(int64_t) { apply_merged_omega(S, raw); });
      parallel_for(s, n, PFV_LAMBDA(int64_t i) {
        const double om = S[S_OMEGA];
        d_x[i] += S[S_ALPHA] * y[i] + om * z[i];
        r[i] -= om * t[i];
      });
    } else {
    shard_halo(c, z);
    spmv_dot(c, P, Aval, z, t, r, 2, R, M_OMEGA, sys.win);  // t = A z, omega = (t,s)/(t,t)
#ifdef PFV_EMULATE
    parallel_for(s, n, PFV_LAMBDA(int64_t i) {
      const double om = S[S_OMEGA];
      d_x[i] += S[S_ALPHA] * y[i] + om * z[i];
      r[i] -= om * t[i];
    });
    dot2(c, n, r, r, rhat, r, R, M_RHO_BETA);
#else
    {
      const int blocks = (int)std::min<int64_t>((n + 255) / 256, kRedBlocks);
      PFV_LAUNCH(k_bicg_tail, dim3(blocks), dim3(256), 0, s, n, d_x, r, y, z, t, rhat, R, (int)M_RHO_BETA);
      finish_reduction(c, blocks, R, M_RHO_BETA);
    }
#endif
    }
    res.iterations = it;
    if (it % check_every == 0 || it == maxit) {
      const double rr = read_scalar<double>(s, S + S_RR);
      res.relres = std::sqrt(rr / bb);
      if (rr <= tol2) { res.converged = true; break; }
      if (!(rr == rr)) break;
    }
  }
  if (res.converged && !sharded && env_int("PFV_TRUE_RESIDUAL", 1) != 0) {
    sys_spmv(c, sys, d_x, t);
    parallel_for(s, n, PFV_LAMBDA(int64_t i) { r[i] = d_b[i] - t[i]; });
    dot2(c, n, r, r, nullptr, nullptr, R, M_RAW);
    const double rr_true = read_scalar<double>(s, S + S_RAW0);
    res.relres = std::sqrt(rr_true / bb);
    if (!(rr_true <= tol2)) {
      res.converged = false;
      if (restarts < kTrueResidualRestarts && it < maxit && rr_true == rr_true) {
        ++restarts;
        ++it;
        goto restart_bicgstab;
      }
    }
  }
  return res;
}

// ------------------------------------------------------------------------------------
// Restarted GMRES(m), right-preconditioned with Jacobi.  Arnoldi by classical Gram-Schmidt
// applied twice (CGS2): per pass one multi-dot kernel (reads w once and the basis once) and
// one multi-axpy kernel, both deterministic (fixed block partition, fixed reduction order).
// The Hessenberg column, the Givens rotations and the triangular solve live on the device in a
// one-thread kernel, so the host only reads the residual estimate to decide when to stop.
constexpr int kGmresBlocks = 1024;
constexpr int kGmresGroup = 8;  // basis vectors handled per pass over w

// out[k] (+)= (V_k, w) for k in [0, nv); V_k = V + k * ld
static void gmres_multi_dot(pfv_ctx_impl& c, int64_t n, const double* V, int64_t ld, int nv, const double* w,
                            double* partial, double* out, bool accumulate) {
  stream_t s = c.stream;
  const int nb = (int)std::min<int64_t>(kGmresBlocks, (n + 2047) / 2048);
  block_for<256>(s, nb, 256 * sizeof(double), PFV_LAMBDA(const WaveCtx& wc) {
    double* sh = reinterpret_cast<double*>(wc.lds);
    const int64_t b = wc.item;
    const int64_t lo = n * b / nb, hi = n * (b + 1) / nb;
    for (int k0 = 0; k0 < nv; k0 += kGmresGroup) {
      const int kc = (nv - k0) < kGmresGroup ? (nv - k0) : kGmresGroup;
      double acc[kGmresGroup];
      for (int k = 0; k < kGmresGroup; ++k) acc[k] = 0.0;
      for (int64_t i = lo + wc.lane; i < hi; i += wc.width) {
        const double wi = w[i];
        for (int k = 0; k < kGmresGroup; ++k)
          if (k < kc) acc[k] += V[(int64_t)(k0 + k) * ld + i] * wi;
      }
      for (int k = 0; k < kc; ++k) {
        sh[wc.lane] = acc[k];
        wc.sync();
        for (int o = wc.width >> 1; o > 0; o >>= 1) {
          if (wc.lane < o) sh[wc.lane] += sh[wc.lane + o];
          wc.sync();
        }
        if (wc.lane0()) partial[(int64_t)(k0 + k) * nb + b] = sh[0];
        wc.sync();
      }
    }
  });
  block_for<256>(s, nv, 256 * sizeof(double), PFV_LAMBDA(const WaveCtx& wc) {
    double* sh = reinterpret_cast<double*>(wc.lds);
    const int64_t k = wc.item;
    double a = 0.0;
    for (int i = wc.lane; i < nb; i += wc.width) a += partial[k * nb + i];
    sh[wc.lane] = a;
    wc.sync();
    for (int o = wc.width >> 1; o > 0; o >>= 1) {
      if (wc.lane < o) sh[wc.lane] += sh[wc.lane + o];
      wc.sync();
    }
    if (wc.lane0()) out[k] = accumulate ? out[k] + sh[0] : sh[0];
    wc.sync();
  });
}

// w -= sum_k coef[k] V_k
static void gmres_multi_axpy(pfv_ctx_impl& c, int64_t n, const double* V, int64_t ld, int nv, const double* coef,
                             double* w) {
  parallel_for(c.stream, n, PFV_LAMBDA(int64_t i) {
    double wi = w[i];
    for (int k = 0; k < nv; ++k) wi -= coef[k] * V[(int64_t)k * ld + i];
    w[i] = wi;
  });
}

static SolveResult gmres_solve(pfv_ctx_impl& c, const LinSys& sys, double rtol, int maxit, int restart,
                               double* d_x, bool x_is_zero, const Precond* Mp = nullptr) {
  Precond Mj;
  Mj.diag = sys.diag;
  const Precond& M = Mp ? *Mp : Mj;
  stream_t s = c.stream;
  const int64_t n = sys.n;
  const CsrPattern& P = *sys.P;
  const double* Aval = sys.val;
  const double* diag = sys.diag;
  const double* d_b = sys.rhs;
  int m = restart > 0 ? std::min(restart, 200) : 30;
  m = std::min(m, std::max(1, maxit));
  double* V = c.gmres_basis.ensure((int64_t)(m + 1) * n);
  double* w = c.kry[0].ensure(n);
  double* y = c.kry[1].ensure(n);
  // small state: R (upper triangular, column-major, ld = m + 1) | cs | sn | g | hcol | h2 | scal
  const int ldh = m + 1;
  double* st = c.gmres_small.ensure((int64_t)ldh * m + 6 * (m + 2) + 8);
  double* Rm = st;
  double* cs = Rm + (int64_t)ldh * m;
  double* sn = cs + m + 2;
  double* g = sn + m + 2;
  double* hcol = g + m + 2;
  double* ysol = hcol + m + 2;
  double* scal = ysol + m + 2;  // [0] beta^2 / ||w||^2, [1] 1 / norm, [2] residual estimate^2, [3] (b,b)
  double* partial = c.red.ensure((int64_t)(m + 2) * kGmresBlocks + 64);
  SolveResult res;

  gmres_multi_dot(c, n, d_b, n, 1, d_b, partial, scal + 3, false);
  const double bb = read_scalar<double>(s, scal + 3);
  if (!(bb > 0.0)) {
    be_memset(d_x, 0, sizeof(double) * n, s);
    res.converged = true;
    return res;
  }
  if (x_is_zero) be_memset(d_x, 0, sizeof(double) * n, s);
  const double tol2 = rtol * rtol * bb;
  const int check_every = (n < 200000) ? 1 : 5;
  bool first = true;
  while (res.iterations < maxit) {
    // r = b - A x -> V_0 = r / beta
    double* v0 = V;
    if (first && x_is_zero) {
      be_d2d(v0, d_b, sizeof(double) * n, s);
    } else {
      sys_spmv(c, sys, d_x, w);
      parallel_for(s, n, PFV_LAMBDA(int64_t i) { v0[i] = d_b[i] - w[i]; });
    }
    first = false;
    gmres_multi_dot(c, n, v0, n, 1, v0, partial, scal, false);
    const double rr0 = read_scalar<double>(s, scal);
    res.relres = std::sqrt(rr0 / bb);
    if (rr0 <= tol2) { res.converged = true; break; }
    if (!(rr0 == rr0)) break;
    parallel_for(s, 1, PFV_LAMBDA(int64_t) {
      const double beta = sqrt(scal[0]);
      scal[1] = 1.0 / beta;
      for (int i = 0; i < m + 2; ++i) g[i] = 0.0;
      g[0] = beta;
    });
    parallel_for(s, n, PFV_LAMBDA(int64_t i) { v0[i] *= scal[1]; });
    int j = 0;
    bool stop = false;
    for (; j < m && res.iterations < maxit && !stop; ++j) {
      const double* vj = V + (int64_t)j * n;
      precond_apply(c, M, n, vj, y);
      sys_spmv(c, sys, y, w);
      // CGS2: h = V^T w, w -= V h, twice; hcol accumulates both passes
      gmres_multi_dot(c, n, V, n, j + 1, w, partial, hcol, false);
      gmres_multi_axpy(c, n, V, n, j + 1, hcol, w);
      gmres_multi_dot(c, n, V, n, j + 1, w, partial, ysol, false);
      gmres_multi_axpy(c, n, V, n, j + 1, ysol, w);
      gmres_multi_dot(c, n, w, n, 1, w, partial, scal, false);
      parallel_for(s, 1, PFV_LAMBDA(int64_t) {
        for (int i = 0; i <= j; ++i) hcol[i] += ysol[i];
        const double hn = sqrt(scal[0]);
        scal[1] = hn > 0.0 ? 1.0 / hn : 0.0;
        for (int i = 0; i < j; ++i) {  // earlier rotations
          const double a = hcol[i], b = hcol[i + 1];
          hcol[i] = cs[i] * a + sn[i] * b;
          hcol[i + 1] = -sn[i] * a + cs[i] * b;
        }
        const double a = hcol[j], r = sqrt(a * a + hn * hn);
        const double cj = r > 0.0 ? a / r : 1.0, sj = r > 0.0 ? hn / r : 0.0;
        cs[j] = cj;
        sn[j] = sj;
        hcol[j] = r;
        g[j + 1] = -sj * g[j];
        g[j] = cj * g[j];
        for (int i = 0; i <= j; ++i) Rm[(int64_t)j * ldh + i] = hcol[i];
        scal[2] = g[j + 1] * g[j + 1];
      });
      double* vn = V + (int64_t)(j + 1) * n;
      parallel_for(s, n, PFV_LAMBDA(int64_t i) { vn[i] = w[i] * scal[1]; });
      ++res.iterations;
      if (res.iterations % check_every == 0 || res.iterations == maxit || j + 1 == m) {
        const double est = read_scalar<double>(s, scal + 2);
        res.relres = std::sqrt(est / bb);
        if (est <= tol2 || !(est == est)) stop = true;
      }
    }
    // x += M^-1 V y,  R y = g
    const int k = j;
    parallel_for(s, 1, PFV_LAMBDA(int64_t) {
      for (int i = k - 1; i >= 0; --i) {
        double t = g[i];
        for (int q = i + 1; q < k; ++q) t -= Rm[(int64_t)q * ldh + i] * ysol[q];
        const double d = Rm[(int64_t)i * ldh + i];
        ysol[i] = d != 0.0 ? t / d : 0.0;
      }
    });
    parallel_for(s, n, PFV_LAMBDA(int64_t i) {
      double a = 0.0;
      for (int q = 0; q < k; ++q) a += ysol[q] * V[(int64_t)q * n + i];
      w[i] = a;
    });
    precond_apply(c, M, n, w, y);
    parallel_for(s, n, PFV_LAMBDA(int64_t i) { d_x[i] += y[i]; });
    // the loop head recomputes the true residual and decides
  }
  if (!res.converged) {  // final true residual
    sys_spmv(c, sys, d_x, w);
    parallel_for(s, n, PFV_LAMBDA(int64_t i) { w[i] = d_b[i] - w[i]; });
    gmres_multi_dot(c, n, w, n, 1, w, partial, scal, false);
    const double rr = read_scalar<double>(s, scal);
    res.relres = std::sqrt(rr / bb);
    res.converged = rr <= tol2;
  }
  return res;
}

}  // namespace pfv
