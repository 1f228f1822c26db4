// sweep.inc — the flow order of a face flux and the substitution along it (PFV_PRECOND_SWEEP).
//
//   order   An interior face with q != 0 (not NaN) is an edge upstream cell -> downstream cell, the upstream side as in
//           upwind_discretize (q >= 0: the cell with cell_faces sign +1).  Forward peel: level 0 = cells without an
//           incoming edge, level l + 1 = cells whose upstream cells all have level <= l (the longest upstream path).
//           Backward peel of the rest: cells without an edge into the remaining set, pass by pass; they get the highest
//           levels, the first pass the highest.  What both leave is the cyclic core: one level between the two.
//           Both peels run on a frontier worklist with integer degree counters: a pass touches the faces of its
//           frontier only, and the host reads one integer per pass (the new tail of the worklist).  The levels do not
//           depend on the order in which the atomics land; the order is a stable radix sort of the cells by level.
//   sweep   M = diagonal of S + the entries S[i,j] with level[j] < level[i].  Level by level, one thread per row:
//           z[i] = (r[i] - sum_{level[j] < level[i]} S[i,j] z[j]) / S[i,i], the sum in stored order.  Levels follow each
//           other by launch order on the handle's stream; a run of consecutive small levels is one launch of a single
//           workgroup that separates them with __syncthreads().  No workgroup waits for another.
//
// No floating-point atomics; every sum has a fixed order.
namespace pfv {

struct Sweep {
  bool valid = false;
  int for_system = -1;           // PFV_MAT_TRANSPORT_SYSTEM or PFV_MAT_ADVDIFF_SYSTEM: whose flux the order was built from
  int64_t nc = 0, n_core = 0;
  int nlev = 0, core_level = -1;
  Buf<int8_t> dir;               // [nf] +1 / -1: edge from the cell on that side of the face; 0: no edge
  Buf<int32_t> level, order;     // caller's cell numbering
  Buf<int32_t> level_s, order_s; // the solve's numbering (reorder.inc), when that differs
  int numbering = -1;            // which numbering level_s / order_s hold (-1: none, 1: the renumbered one)
  std::vector<int32_t> h_lptr;   // [nlev + 1] first position of every level in order
  Buf<int32_t> lptr;             // the same on the device
  struct Seg { int l0, l1; };    // levels [l0, l1) of one launch (l1 - l0 > 1: a single workgroup takes the run)
  std::vector<Seg> plan;
  int plan_key = -1;
  double order_ms = 0.0;
  const int32_t* lev(bool permuted) const { return permuted ? level_s.p : level.p; }
  const int32_t* ord(bool permuted) const { return permuted ? order_s.p : order.p; }
  bool permuted = false;         // numbering of the system the running solve works on
};

// the edge of every face for the flux q
static void sweep_classify(pfv_ctx_impl& c, const double* q, int8_t* dir) {
  const int64_t nf = c.nf;
  const int32_t* side = c.upw_side;
  parallel_for(c.stream, nf, PFV_LAMBDA(int64_t f) {
    const double qf = q[f];
    int8_t d = 0;
    if (side[f] >= 0 && side[nf + f] >= 0 && qf == qf && qf != 0.0) d = qf > 0.0 ? 1 : -1;
    dir[f] = d;
  });
}

// does the flux q have the edges the order was built from?
static bool sweep_same_edges(pfv_ctx_impl& c, const Sweep& sw, const double* q) {
  stream_t s = c.stream;
  const int64_t nf = c.nf;
  const int32_t* side = c.upw_side;
  const int8_t* dir = sw.dir;
  Buf<int32_t> flag_;
  int32_t* flag = flag_.ensure(1);
  be_memset(flag, 0, sizeof(int32_t), s);
  parallel_for(s, nf, PFV_LAMBDA(int64_t f) {
    const double qf = q[f];
    int8_t d = 0;
    if (side[f] >= 0 && side[nf + f] >= 0 && qf == qf && qf != 0.0) d = qf > 0.0 ? 1 : -1;
    if (d != dir[f]) atomic_max_i32(flag, 1);
  });
  return read_scalar<int32_t>(s, flag) == 0;
}

// stable sort of the cells by level (ascending index inside a level)
static void sweep_sort(pfv_ctx_impl& c, int64_t nc, int nlev, const int32_t* lev, int32_t* order) {
  stream_t s = c.stream;
  Buf<uint32_t> kin_, kout_;
  Buf<int32_t> vin_;
  uint32_t* kin = kin_.ensure(nc);
  int32_t* vin = vin_.ensure(nc);
  parallel_for(s, nc, PFV_LAMBDA(int64_t i) {
    kin[i] = (uint32_t)lev[i];
    vin[i] = (int32_t)i;
  });
  int bits = 1;
  while ((int64_t(1) << bits) < nlev) ++bits;
  sort_pairs(s, c.scratch, kin, kout_.ensure(nc), vin, order, (size_t)nc, bits);
  be_sync(s);  // (the key buffers are freed on return)
}

static void sweep_build_order(pfv_ctx_impl& c, Sweep& sw, const double* q, int for_system) {
  stream_t s = c.stream;
  Timer tm;
  tm.start(s);
  upwind_face_cells(c);
  const int64_t nc = c.nc, nf = c.nf;
  const int32_t* cf_ptr = c.cf_ptr;
  const int32_t* cf_idx = c.cf_idx;
  const int32_t* side = c.upw_side;
  sw.valid = false;
  sw.numbering = -1;
  sw.plan_key = -1;
  int8_t* dir = sw.dir.ensure(nf);
  int32_t* lev = sw.level.ensure(nc);
  Buf<int32_t> indeg_, outdeg_, wl_, blev_, tail_;
  int32_t* indeg = indeg_.ensure(nc);
  int32_t* outdeg = outdeg_.ensure(nc);
  int32_t* wl = wl_.ensure(nc);      // every cell enters the worklist at most once: a pass is a range of it
  int32_t* blev = blev_.ensure(nc);  // pass of the backward peel that removed the cell (-1: none)
  int32_t* tail = tail_.ensure(1);
  be_memset(indeg, 0, sizeof(int32_t) * (size_t)nc, s);
  be_memset(lev, 0xff, sizeof(int32_t) * (size_t)nc, s);
  be_memset(blev, 0xff, sizeof(int32_t) * (size_t)nc, s);
  be_memset(tail, 0, sizeof(int32_t), s);
  sweep_classify(c, q, dir);
  parallel_for(s, nf, PFV_LAMBDA(int64_t f) {
    const int d = dir[f];
    if (d) atomic_add_i32(indeg + (d > 0 ? side[nf + f] : side[f]), 1);
  });
  // ---- forward peel
  parallel_for(s, nc, PFV_LAMBDA(int64_t i) {
    if (indeg[i] == 0) {
      lev[i] = 0;
      wl[atomic_fetch_add_i32(tail, 1)] = (int32_t)i;
    }
  });
  std::vector<int32_t> fwd, bwd;  // cells per pass
  int32_t begin = 0, end = read_scalar<int32_t>(s, tail);
  while (end > begin) {
    fwd.push_back(end - begin);
    const int32_t next = (int32_t)fwd.size(), b0 = begin;
    parallel_for(s, end - begin, PFV_LAMBDA(int64_t k) {
      const int32_t cell = wl[b0 + k];
      for (int e = cf_ptr[cell]; e < cf_ptr[cell + 1]; ++e) {
        const int f = cf_idx[e];
        const int d = dir[f];
        if (!d) continue;
        const int32_t up = d > 0 ? side[f] : side[nf + f];
        if (up != cell) continue;
        const int32_t dn = d > 0 ? side[nf + f] : side[f];
        if (atomic_fetch_add_i32(indeg + dn, -1) == 1) {  // the last upstream cell of dn
          lev[dn] = next;
          wl[atomic_fetch_add_i32(tail, 1)] = dn;
        }
      }
    });
    begin = end;
    end = read_scalar<int32_t>(s, tail);
  }
  const int nfwd = (int)fwd.size();
  // ---- backward peel of the cells the forward peel left (lev < 0)
  if (end < nc) {
    parallel_for(s, nc, PFV_LAMBDA(int64_t i) {
      if (lev[i] >= 0) return;
      int m = 0;
      for (int e = cf_ptr[i]; e < cf_ptr[i + 1]; ++e) {
        const int f = cf_idx[e];
        const int d = dir[f];
        if (!d) continue;
        const int32_t up = d > 0 ? side[f] : side[nf + f];
        if (up != (int32_t)i) continue;
        const int32_t dn = d > 0 ? side[nf + f] : side[f];
        if (lev[dn] < 0) ++m;
      }
      outdeg[i] = m;
      if (m == 0) {
        blev[i] = 0;
        wl[atomic_fetch_add_i32(tail, 1)] = (int32_t)i;
      }
    });
    begin = end;
    end = read_scalar<int32_t>(s, tail);
    while (end > begin) {
      bwd.push_back(end - begin);
      const int32_t next = (int32_t)bwd.size(), b0 = begin;
      parallel_for(s, end - begin, PFV_LAMBDA(int64_t k) {
        const int32_t cell = wl[b0 + k];
        for (int e = cf_ptr[cell]; e < cf_ptr[cell + 1]; ++e) {
          const int f = cf_idx[e];
          const int d = dir[f];
          if (!d) continue;
          const int32_t dn = d > 0 ? side[nf + f] : side[f];
          if (dn != cell) continue;
          const int32_t up = d > 0 ? side[f] : side[nf + f];
          if (lev[up] >= 0) continue;  // (not in the remaining set)
          if (atomic_fetch_add_i32(outdeg + up, -1) == 1) {  // the last edge of up into the remaining set
            blev[up] = next;
            wl[atomic_fetch_add_i32(tail, 1)] = up;
          }
        }
      });
      begin = end;
      end = read_scalar<int32_t>(s, tail);
    }
  }
  const int nbwd = (int)bwd.size();
  sw.nc = nc;
  sw.n_core = nc - end;
  const int has_core = sw.n_core > 0 ? 1 : 0;
  sw.core_level = has_core ? nfwd : -1;
  sw.nlev = nfwd + has_core + nbwd;
  if (has_core || nbwd) {
    parallel_for(s, nc, PFV_LAMBDA(int64_t i) {
      if (lev[i] >= 0) return;
      lev[i] = blev[i] >= 0 ? nfwd + has_core + (nbwd - 1 - blev[i]) : nfwd;
    });
  }
  sw.h_lptr.assign(1, 0);
  for (int32_t m : fwd) sw.h_lptr.push_back(sw.h_lptr.back() + m);
  if (has_core) sw.h_lptr.push_back(sw.h_lptr.back() + (int32_t)sw.n_core);
  for (int k = nbwd - 1; k >= 0; --k) sw.h_lptr.push_back(sw.h_lptr.back() + bwd[(size_t)k]);
  be_h2d(sw.lptr.ensure((size_t)sw.nlev + 1), sw.h_lptr.data(), sizeof(int32_t) * ((size_t)sw.nlev + 1), s);
  sweep_sort(c, nc, sw.nlev, lev, sw.order.ensure(nc));
  sw.for_system = for_system;
  sw.valid = true;
  sw.order_ms = tm.stop(s);
}

// level[] / order[] in the numbering the Krylov loop works in
static void sweep_set_numbering(pfv_ctx_impl& c, Sweep& sw, bool permuted) {
  sw.permuted = permuted;
  if (!permuted || sw.numbering == 1) return;
  const int64_t nc = sw.nc;
  const int32_t* perm = c.cell_perm;
  const int32_t* lev = sw.level;
  int32_t* ls = sw.level_s.ensure(nc);
  parallel_for(c.stream, nc, PFV_LAMBDA(int64_t r) { ls[r] = lev[perm[r]]; });
  sweep_sort(c, nc, sw.nlev, ls, sw.order_s.ensure(nc));
  sw.numbering = 1;
}

// which levels go into which launch.  PFV_SWEEP_MERGE=0: one launch per level; else runs of consecutive levels of at
// most PFV_SWEEP_MERGE_ROWS rows (default 512) are handed to one workgroup each
static void sweep_make_plan(Sweep& sw) {
  const int merge = env_int("PFV_SWEEP_MERGE", 1) != 0 ? 1 : 0;
  const int rows = std::max(1, std::min(env_int("PFV_SWEEP_MERGE_ROWS", 512), 1 << 20));
  const int key = merge ? rows : 0;
  if (sw.plan_key == key) return;
  sw.plan.clear();
  for (int l = 0; l < sw.nlev; ++l) {
    const bool small = merge && sw.h_lptr[(size_t)l + 1] - sw.h_lptr[(size_t)l] <= rows;
    const bool prev_small = merge && l > 0 && sw.h_lptr[(size_t)l] - sw.h_lptr[(size_t)l - 1] <= rows;
    if (small && prev_small) sw.plan.back().l1 = l + 1;
    else sw.plan.push_back({l, l + 1});
  }
  sw.plan_key = key;
}

// one row of the substitution (shared by both launch forms: they give the same bits)
PFV_FN void sweep_row(int32_t i, const int32_t* ip, const int32_t* ix, const double* val, const double* diag,
                      const int32_t* lev, const double* r, double* z) {
  const int32_t li = lev[i];
  double sum = 0.0;
  for (int e = ip[i]; e < ip[i + 1]; ++e) {
    const int32_t j = ix[e];
    if (lev[j] < li) sum += val[e] * z[j];
  }
  z[i] = (r[i] - sum) / diag[i];
}

// ---- the launch rule, once.  Levels [l0, l1) of the order in the chosen numbering, `items` work items per row:
// body(row, a) for a in [0, items).  One level is one launch over its rows; a run of levels is one launch of a single
// workgroup that takes them one after the other.  OnePerRow makes the count a compile-time 1 (no division in the
// kernel); an int is the run-time count.  (Both forms name `ord` before `body`: the kernel's arguments then lie in the
// order the row functions' register use was measured with -- DESIGN.md 18, 19.)
struct OnePerRow {
  PFV_FN constexpr operator int() const { return 1; }
};
// The direction the levels are taken in: Ascending is the substitution with S, Descending the one with its transpose
// (sweep_row_multi_t).  A compile-time tag: the loop over the levels of a run folds to one direction per instantiation.
struct Ascending {
  static constexpr bool reverse = false;
};
struct Descending {
  static constexpr bool reverse = true;
};
template <class Items, class Body, class Dir = Ascending>
static void sweep_levels(pfv_ctx_impl& c, const Sweep& sw, bool permuted, int l0, int l1, Items items, Body body,
                         Dir = Dir{}) {
  const int32_t* ord = sw.ord(permuted);
  if (l1 - l0 == 1) {
    const int32_t a0 = sw.h_lptr[(size_t)l0], m = sw.h_lptr[(size_t)l1] - a0;
    parallel_for(c.stream, (int64_t)m * items, PFV_LAMBDA(int64_t t) {
      const int k = items;
      const int32_t i = ord[a0 + t / k];
      body(i, (int)(t % k));
    });
  } else if (l1 > l0) {
    const int32_t* lp = sw.lptr;
    block_for<256>(c.stream, 1, 0, PFV_LAMBDA(const WaveCtx& w) {
      const int k = items;
      for (int l = Dir::reverse ? l1 - 1 : l0; Dir::reverse ? l >= l0 : l < l1; l += Dir::reverse ? -1 : 1) {
        const int32_t a0 = lp[l], m = lp[l + 1] - a0;
        PFV_LANES(t, m * k) {
          const int32_t i = ord[a0 + t / k];
          body(i, t % k);
        }
        w.sync();  // (the next level reads what this one wrote: same workgroup, same CU)
      }
    });
  }
}

// The segments of the launch plan cut to the levels [from, to) -- a run is cut where the core level, which is iterated
// on its own, falls into it --, each handed to levels(l0, l1); Descending: the segments from last to first.  Returns
// the launches.
template <class Levels, class Dir = Ascending>
static int sweep_plan_range(const Sweep& sw, int from, int to, Levels levels, Dir = Dir{}) {
  int launches = 0;
  const size_t ns = sw.plan.size();
  for (size_t n = 0; n < ns; ++n) {
    const Sweep::Seg& g = sw.plan[Dir::reverse ? ns - 1 - n : n];
    const int l0 = std::max(g.l0, from), l1 = std::min(g.l1, to);
    if (l0 >= l1) continue;
    levels(l0, l1);
    ++launches;
  }
  return launches;
}

static void sweep_apply(pfv_ctx_impl& c, const Sweep& sw, const CsrPattern& P, const double* val, const double* diag,
                        const double* in, double* out) {
  const int32_t* ip = P.indptr;
  const int32_t* ix = P.indices;
  const int32_t* lev = sw.lev(sw.permuted);
  sweep_plan_range(sw, 0, sw.nlev, [&](int l0, int l1) {
    sweep_levels(c, sw, sw.permuted, l0, l1, OnePerRow{},
                 PFV_LAMBDA(int32_t i, int) { sweep_row(i, ip, ix, val, diag, lev, in, out); });
  });
}

// out[0] = (b, b), out[1] = (b - t, b - t): fixed partition, fixed reduction order
static void sweep_residual_norms(pfv_ctx_impl& c, int64_t n, const double* b, const double* t, double* out) {
  stream_t s = c.stream;
  const int nb = (int)std::min<int64_t>(kGmresBlocks, (n + 2047) / 2048);
  double* partial = c.red.ensure(2 * (size_t)kGmresBlocks + 64);
  block_for<256>(s, nb, 2 * 256 * sizeof(double), PFV_LAMBDA(const WaveCtx& wc) {
    double* sh = reinterpret_cast<double*>(wc.lds);
    const int64_t blk = wc.item;
    const int64_t lo = n * blk / nb, hi = n * (blk + 1) / nb;
    double a0 = 0.0, a1 = 0.0;
    for (int64_t i = lo + wc.lane; i < hi; i += wc.width) {
      const double bi = b[i], ri = bi - t[i];
      a0 += bi * bi;
      a1 += ri * ri;
    }
    sh[wc.lane] = a0;
    sh[wc.width + wc.lane] = a1;
    wc.sync();
    for (int o = wc.width >> 1; o > 0; o >>= 1) {
      if (wc.lane < o) {
        sh[wc.lane] += sh[wc.lane + o];
        sh[wc.width + wc.lane] += sh[wc.width + wc.lane + o];
      }
      wc.sync();
    }
    if (wc.lane0()) {
      partial[blk] = sh[0];
      partial[nb + blk] = sh[wc.width];
    }
    wc.sync();
  });
  block_for<256>(s, 2, 256 * sizeof(double), PFV_LAMBDA(const WaveCtx& wc) {
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
    if (wc.lane0()) out[k] = sh[0];
    wc.sync();
  });
}

// ---- k vectors per sweep (pfv_transport_advance_multi).  The k systems share the pattern, the off-diagonal values and
// the level test; they differ in the diagonal A[i,i] + acc[i,a] and the right-hand side.  Vectors are interleaved,
// v[i * k + a].  One work item per (row, component) of a level: the k items of a row load val[e], ix[e] and lev[j] from
// the same address and z[j, 0..k) as one contiguous run, and a level has k times the work items of the single sweep.
// The order and the launch plan are those of sweep_apply; the sum runs in stored order, as in sweep_row.
PFV_FN void sweep_row_multi(int32_t i, int a, int k, const int32_t* ip, const int32_t* ix, const double* val,
                            const double* diag, const double* acc, const int32_t* lev, const double* r, double* z) {
  const int32_t li = lev[i];
  double sum = 0.0;
  for (int e = ip[i]; e < ip[i + 1]; ++e) {
    const int32_t j = ix[e];
    if (lev[j] < li) sum += val[e] * z[(int64_t)j * k + a];
  }
  const int64_t p = (int64_t)i * k + a;
  z[p] = (r[p] - sum) / (diag[i] + acc[p]);
}

static void sweep_apply_multi(pfv_ctx_impl& c, const Sweep& sw, const CsrPattern& P, const double* val,
                              const double* diag, const double* acc, int k, const double* in, double* out) {
  const int32_t* ip = P.indptr;
  const int32_t* ix = P.indices;
  const int32_t* lev = sw.lev(sw.permuted);
  sweep_plan_range(sw, 0, sw.nlev, [&](int l0, int l1) {
    sweep_levels(c, sw, sw.permuted, l0, l1, k,
                 PFV_LAMBDA(int32_t i, int a) { sweep_row_multi(i, a, k, ip, ix, val, diag, acc, lev, in, out); });
  });
}

// ---- the norms of k interleaved vectors, once.  pair(i, a) gives the two numbers (u, v) of row i, component a;
// out[a] = sum_i u^2, out[k + a] = sum_i v^2 over the n rows.  Fixed partition, fixed reduction order: a workgroup takes a
// range of rows, slot g * k + a of it the rows lo + g, lo + g + G, ... of component a (G = 256 / k), and the G sums of a
// component are folded pairwise; then one workgroup per number adds the workgroups' partial sums as
// sweep_residual_norms does.
struct NormPair {
  double u, v;
};
template <class Pair>
static void sweep_norms_pairs(pfv_ctx_impl& c, int64_t n, int k, double* out, Pair pair) {
  stream_t s = c.stream;
  const int nb = (int)std::min<int64_t>(kGmresBlocks, (n * k + 2047) / 2048);
  const int G = 256 / k, slots = G * k;
  int fold = 1;
  while (fold < G) fold <<= 1;
  double* partial = c.red.ensure(2 * (size_t)k * kGmresBlocks + 64);
  block_for<256>(s, nb, 2 * 256 * sizeof(double), PFV_LAMBDA(const WaveCtx& w) {
    double* sh = reinterpret_cast<double*>(w.lds);
    const int64_t blk = w.item;
    const int64_t lo = n * blk / nb, hi = n * (blk + 1) / nb;
    PFV_LANES(slot, slots) {
      const int a = slot % k, g = slot / k;
      double a0 = 0.0, a1 = 0.0;
      for (int64_t i = lo + g; i < hi; i += G) {
        const NormPair q = pair(i, a);
        a0 += q.u * q.u;
        a1 += q.v * q.v;
      }
      sh[slot] = a0;
      sh[256 + slot] = a1;
    }
    w.sync();
    for (int o = fold >> 1; o > 0; o >>= 1) {
      PFV_LANES(slot, slots) {
        if (slot / k < o && slot / k + o < G) {
          sh[slot] += sh[slot + o * k];
          sh[256 + slot] += sh[256 + slot + o * k];
        }
      }
      w.sync();
    }
    PFV_LANES(a, k) {
      partial[(int64_t)a * nb + blk] = sh[a];
      partial[(int64_t)(k + a) * nb + blk] = sh[256 + a];
    }
    w.sync();
  });
  block_for<256>(s, 2 * k, 256 * sizeof(double), PFV_LAMBDA(const WaveCtx& wc) {
    double* sh = reinterpret_cast<double*>(wc.lds);
    const int64_t m = wc.item;
    double a = 0.0;
    for (int i = wc.lane; i < nb; i += wc.width) a += partial[m * nb + i];
    sh[wc.lane] = a;
    wc.sync();
    for (int o = wc.width >> 1; o > 0; o >>= 1) {
      if (wc.lane < o) sh[wc.lane] += sh[wc.lane + o];
      wc.sync();
    }
    if (wc.lane0()) out[m] = sh[0];
    wc.sync();
  });
}

// out[a] = (r_a, r_a), out[k + a] = (r_a - t_a, r_a - t_a) of interleaved vectors of n rows
static void sweep_norms_interleaved(pfv_ctx_impl& c, int64_t n, int k, const double* r, const double* t, double* out) {
  sweep_norms_pairs(c, n, k, out, PFV_LAMBDA(int64_t i, int a) {
    const double ri = r[i * k + a];
    return NormPair{ri, ri - t[i * k + a]};
  });
}

// The residual check of all k components in one pass: t[i,a] = sum_e A[i,e] x[j,a] + acc[i,a] x[i,a] in stored order,
// out[a] = (r_a, r_a), out[k + a] = (r_a - t_a, r_a - t_a).
static void sweep_residual_norms_multi(pfv_ctx_impl& c, const CsrPattern& P, const double* val, const double* acc,
                                       int k, const double* r, const double* x, double* out) {
  const int32_t* ip = P.indptr;
  const int32_t* ix = P.indices;
  sweep_norms_pairs(c, P.nrows, k, out, PFV_LAMBDA(int64_t i, int a) {
    double t = 0.0;
    for (int e = ip[i]; e < ip[i + 1]; ++e) t += val[e] * x[(int64_t)ix[e] * k + a];
    const int64_t p = i * k + a;
    t += acc[p] * x[p];
    const double ri = r[p];
    return NormPair{ri, ri - t};
  });
}

// ---- the saturation step (pfv_transport_advance_nl): the quantity moves with q f(s), f nondecreasing (fluxfn.h).
// Per row  acc_i s_i + o_i f(s_i) = R_i,  o_i = A_ii + sink_i,  R_i = rhs_i - sum_{lev[j] < lev[i]} A_ij phi_j  with
// rhs = acc o s_old - b_ref + src and phi = f(s) carried beside s: a row reads the phi of its upstream cells and writes
// its own s and phi, so no row evaluates f for a neighbour.  g(x) = acc x + o f(x) - R is strictly increasing (acc > 0).
//   root   Newton from the start value clipped into the bracket [0, 1]; an iterate that leaves the bracket, or a |g|
//          that did not halve, is replaced by the midpoint.  Stop: |g| <= 2^-50 (|R| + acc + |o|) -- twice what evaluating
//          g in doubles resolves --, or a bracket of 2^-52, or kNlEvals evaluations.  Lanes of a wavefront need different
//          numbers of evaluations; they wait for the slowest.
//   leave  g(0) or g(1) beyond that tolerance on the wrong side: no root in [0, 1].  The row takes the end of the
//          interval and records its index with an integer atomic minimum.
//   core   rows of the core level (phi_prev != nullptr) take their in-core neighbours from phi_prev, the previous
//          iterate: nonlinear Jacobi, independent of the scheduling.
constexpr int kNlEvals = 64;
constexpr double kNlGTol = 8.881784197001252e-16;  // 2^-50
constexpr int kNlCoreCheck = 8;                    // the core's stop test is evaluated every 8th iteration

PFV_FN void sweep_row_nl(int32_t i, const int32_t* ip, const int32_t* ix, const double* val, const double* diag,
                         const double* sink, const double* acc, const double* rhs, const int32_t* lev, const FluxFn& F,
                         const double* s_start, const double* phi_prev, double* s, double* phi, int32_t* status) {
  const int32_t li = lev[i];
  double sum = 0.0;
  for (int e = ip[i]; e < ip[i + 1]; ++e) {
    const int32_t j = ix[e];
    const int32_t lj = lev[j];
    if (lj < li) sum += val[e] * phi[j];
    else if (phi_prev && lj == li && j != i) sum += val[e] * phi_prev[j];
  }
  const double R = rhs[i] - sum, a = acc[i], o = diag[i] + (sink ? sink[i] : 0.0);
  const double tol = kNlGTol * (fabs(R) + a + fabs(o));
  double df;
  double x = 0.0, f = fluxfn_eval(F, x, &df);
  if (o * f - R > tol) {  // g(0) > 0
    atomic_min_i32(status, i);
    s[i] = x;
    phi[i] = f;
    return;
  }
  x = 1.0;
  f = fluxfn_eval(F, x, &df);
  if (a + o * f - R < -tol) {  // g(1) < 0
    atomic_min_i32(status, i);
    s[i] = x;
    phi[i] = f;
    return;
  }
  double lo = 0.0, hi = 1.0, g_prev = 1.79769313486231570e308;
  x = s_start[i];
  x = x < lo ? lo : (x > hi ? hi : x);
  for (int it = 0;; ++it) {
    f = fluxfn_eval(F, x, &df);
    const double g = a * x + o * f - R;
    if (fabs(g) <= tol || it == kNlEvals - 1) break;
    if (g > 0.0) hi = x;
    else lo = x;
    if (hi - lo <= 2.220446049250313e-16) break;
    double xn = x - g / (a + o * df);
    if (!(xn > lo && xn < hi) || fabs(g) > 0.5 * g_prev) xn = 0.5 * (lo + hi);
    g_prev = fabs(g);
    x = xn;
  }
  s[i] = x;
  phi[i] = f;
}

// ---- k components carried by the transported phase (pfv_transport_advance_nl_multi).  Once s_i and phi_i = f(s_i) of a
// row are known, component a of the row is one division:
//     d = acc_i s_i + ads_ai + o_i phi_i,   c_ai = (rhs_ai - sum_{lev[j] < lev[i]} A_ij psi_aj) / d,   psi_ai = phi_i c_ai
// with psi = phi o c carried for the cells downstream as phi is.  Vectors are interleaved as in sweep_row_multi,
// v[i * k + a]: the k values of an upstream cell are one run of 8 k bytes.  The thread that found the root of the row
// takes its components, four accumulators at a time, the sums in stored order; the last chunk takes k mod 4.  d == 0 (a
// dry cell without sorption) keeps the value of the step's start; the acceptance check judges that row.  Core rows take psi_prev of their in-core neighbours, as phi_prev.
// `frozen` (core iterations after the saturation's own stop test has passed): s and phi of the row stay as they are and
// the components alone go on, so that the saturation stops where pfv_transport_advance_nl stops, bit for bit.
constexpr int kNlcGroup = 8;  // entries of a row whose loads are issued together (a tetrahedron's row has 5, a hexahedron's 7)
struct NlComp {
  int k = 0;                       // 0: the saturation alone
  const double* ads = nullptr;     // [n k] sorption capacity (may be nullptr)
  const double* rhs = nullptr;     // [n k]
  const double* c_start = nullptr; // [n k] the state of the step's start
  const double* psi_prev = nullptr;
  bool frozen = false;
  double* c = nullptr;
  double* psi = nullptr;
};

PFV_FN double sweep_nlc_divide(const NlComp& C, int64_t p, double as, double op, double u) {
  const double d = as + (C.ads ? C.ads[p] : 0.0) + op;
  return d != 0.0 ? (C.rhs[p] - u) / d : C.c_start[p];
}

PFV_FN void sweep_row_nlc(int32_t i, const int32_t* ip, const int32_t* ix, const double* val, const double* diag,
                          const double* sink, const double* acc, const double* rhs, const int32_t* lev, const FluxFn& F,
                          const double* s_start, const double* phi_prev, double* s, double* phi, int32_t* status,
                          const NlComp& C) {
  if (!C.frozen) sweep_row_nl(i, ip, ix, val, diag, sink, acc, rhs, lev, F, s_start, phi_prev, s, phi, status);
  const int k = C.k;
  const int32_t li = lev[i];
  const double ph = phi[i];
  const double as = acc[i] * s[i], op = (diag[i] + (sink ? sink[i] : 0.0)) * ph;
  const int64_t p = (int64_t)i * k;
  const int e_end = ip[i + 1];
  for (int a0 = 0; a0 < k; a0 += 4) {
    // Components a0 .. a0 + 3.  In the last chunk an accumulator beyond k takes component a0 again (offset 0): it sums
    // the same products in the same order and writes the same bits to the same place, so nothing below branches on k.
    // The entries are taken kNlcGroup at a time: the group's indices, then its levels, then its values are loaded
    // together, so a row of up to kNlcGroup entries pays three round trips to memory and not three per entry -- the
    // level is bound by that latency.  A slot past the row's end repeats the last entry, and a slot that is not
    // upstream reads the row's own rhs instead of psi (an address that is valid and that no thread writes here); both
    // enter the sums as + 0, in stored order.
    const int m = k - a0;
    const int o1 = m > 1 ? 1 : 0, o2 = m > 2 ? 2 : 0, o3 = m > 3 ? 3 : 0;
    const double* own = C.rhs + p + a0;
    double u0 = 0.0, u1 = 0.0, u2 = 0.0, u3 = 0.0;
    for (int e0 = ip[i]; e0 < e_end; e0 += kNlcGroup) {
      int32_t j[kNlcGroup];
      double v[kNlcGroup];
      const double* up[kNlcGroup];
#pragma unroll
      for (int t = 0; t < kNlcGroup; ++t) {
        const int e = e0 + t < e_end ? e0 + t : e_end - 1;
        j[t] = ix[e];
        v[t] = val[e];
      }
#pragma unroll
      for (int t = 0; t < kNlcGroup; ++t) {
        const int32_t lj = lev[j[t]];
        const double* src = lj < li ? C.psi : (C.psi_prev && lj == li && j[t] != i ? C.psi_prev : nullptr);
        up[t] = src && e0 + t < e_end ? src + (int64_t)j[t] * k + a0 : nullptr;
      }
#pragma unroll
      for (int t = 0; t < kNlcGroup; ++t) {
        const double* r = up[t] ? up[t] : own;
        const double w0 = r[0], w1 = r[o1], w2 = r[o2], w3 = r[o3];
        const double vt = up[t] ? v[t] : 0.0;
        u0 += vt * (up[t] ? w0 : 0.0);
        u1 += vt * (up[t] ? w1 : 0.0);
        u2 += vt * (up[t] ? w2 : 0.0);
        u3 += vt * (up[t] ? w3 : 0.0);
      }
    }
    const int64_t p0 = p + a0, p1 = p0 + o1, p2 = p0 + o2, p3 = p0 + o3;
    const double x0 = sweep_nlc_divide(C, p0, as, op, u0), x1 = sweep_nlc_divide(C, p1, as, op, u1);
    const double x2 = sweep_nlc_divide(C, p2, as, op, u2), x3 = sweep_nlc_divide(C, p3, as, op, u3);
    C.c[p0] = x0;  // (the loads of all four before the first store: a store could alias them for the compiler)
    C.c[p1] = x1;
    C.c[p2] = x2;
    C.c[p3] = x3;
    C.psi[p0] = ph * x0;
    C.psi[p1] = ph * x1;
    C.psi[p2] = ph * x2;
    C.psi[p3] = ph * x3;
  }
}

// levels [l0, l1) of the order by the launch rule (sweep_levels): with components (C.k > 0) the rows are those of
// sweep_row_nlc, else of sweep_row_nl
static void sweep_levels_nl(pfv_ctx_impl& c, const Sweep& sw, int l0, int l1, const CsrPattern& P, const double* val,
                            const double* diag, const double* sink, const double* acc, const double* rhs,
                            const FluxFn& F, const double* s_start, const double* phi_prev, double* s, double* phi,
                            int32_t* status, const NlComp& C) {
  const int32_t* ip = P.indptr;
  const int32_t* ix = P.indices;
  const int32_t* lev = sw.lev(false);
  if (C.k > 0) {
    sweep_levels(c, sw, false, l0, l1, OnePerRow{}, PFV_LAMBDA(int32_t i, int) {
      sweep_row_nlc(i, ip, ix, val, diag, sink, acc, rhs, lev, F, s_start, phi_prev, s, phi, status, C);
    });
  } else {
    sweep_levels(c, sw, false, l0, l1, OnePerRow{}, PFV_LAMBDA(int32_t i, int) {
      sweep_row_nl(i, ip, ix, val, diag, sink, acc, rhs, lev, F, s_start, phi_prev, s, phi, status);
    });
  }
}

// the launch plan's levels in [from, to), outside the core (phi_prev = nullptr).  Returns the launches.
static int sweep_apply_nl(pfv_ctx_impl& c, const Sweep& sw, int from, int to, const CsrPattern& P, const double* val,
                          const double* diag, const double* sink, const double* acc, const double* rhs,
                          const FluxFn& F, const double* s_start, double* s, double* phi, int32_t* status,
                          const NlComp& C) {
  return sweep_plan_range(sw, from, to, [&](int l0, int l1) {
    sweep_levels_nl(c, sw, l0, l1, P, val, diag, sink, acc, rhs, F, s_start, nullptr, s, phi, status, C);
  });
}

// t[i] = acc_i s_i + sum_e A_ie phi_j + sink_i phi_i in stored order: F(s) = rhs - t.  With lev: the entries up to the
// row's own level alone (the core's stop test runs before the levels behind it have a phi; their entries are the stored
// zeros of the downstream side)
PFV_FN double sweep_nl_row_image(int32_t i, const int32_t* ip, const int32_t* ix, const double* val, const double* sink,
                                 const double* acc, const double* s, const double* phi, const int32_t* lev) {
  double t = 0.0;
  for (int e = ip[i]; e < ip[i + 1]; ++e) {
    const int32_t j = ix[e];
    if (!lev || lev[j] <= lev[i]) t += val[e] * phi[j];
  }
  if (sink) t += sink[i] * phi[i];
  return t + acc[i] * s[i];
}

static void sweep_nl_image(pfv_ctx_impl& c, const CsrPattern& P, const double* val, const double* sink,
                           const double* acc, const double* s, const double* phi, double* t) {
  const int32_t* ip = P.indptr;
  const int32_t* ix = P.indices;
  parallel_for(c.stream, P.nrows, PFV_LAMBDA(int64_t i) {
    t[i] = sweep_nl_row_image((int32_t)i, ip, ix, val, sink, acc, s, phi, nullptr);
  });
}

// The components' images beside it: tc[i, a] = (acc_i s_i + ads_ai) c_ai + sum_e A_ie psi_aj + sink_i psi_ai, in stored
// order; lev as in sweep_nl_row_image.
PFV_FN double sweep_nlc_row_image(int32_t i, int a, int k, const int32_t* ip, const int32_t* ix, const double* val,
                                  const double* sink, const double* acc, const double* ads, const double* s,
                                  const double* c, const double* psi, const int32_t* lev) {
  double t = 0.0;
  for (int e = ip[i]; e < ip[i + 1]; ++e) {
    const int32_t j = ix[e];
    if (!lev || lev[j] <= lev[i]) t += val[e] * psi[(int64_t)j * k + a];
  }
  const int64_t p = (int64_t)i * k + a;
  if (sink) t += sink[i] * psi[p];
  return t + (acc[i] * s[i] + (ads ? ads[p] : 0.0)) * c[p];
}

// one kernel for the saturation's image and the k components': work item (row, a), a == k the saturation
static void sweep_nlc_image(pfv_ctx_impl& c, const CsrPattern& P, const double* val, const double* sink,
                            const double* acc, const double* s, const double* phi, double* t, const NlComp& C,
                            double* tc) {
  const int32_t* ip = P.indptr;
  const int32_t* ix = P.indices;
  const int k = C.k;
  parallel_for(c.stream, P.nrows * (k + 1), PFV_LAMBDA(int64_t w) {
    const int32_t i = (int32_t)(w / (k + 1));
    const int a = (int)(w % (k + 1));
    if (a == k) t[i] = sweep_nl_row_image(i, ip, ix, val, sink, acc, s, phi, nullptr);
    else tc[(int64_t)i * k + a] = sweep_nlc_row_image(i, a, k, ip, ix, val, sink, acc, C.ads, s, C.c, C.psi, nullptr);
  });
}

// ---- the core rows.  For each (core row, component): body(row, a, w), w = m * items + a the position of component a
// of the m-th core row among them (Items as in sweep_levels).
template <class Items, class Body>
static void sweep_core_rows(pfv_ctx_impl& c, const Sweep& sw, Items items, Body body) {
  const int32_t* ord = sw.ord(false);
  const int32_t a0 = sw.h_lptr[(size_t)sw.core_level];
  parallel_for(c.stream, sw.n_core * items, PFV_LAMBDA(int64_t w) {
    const int k = items;
    body(ord[a0 + w / k], (int)(w % k), w);
  });
}

// The core rows, compacted: cb[m] = rhs of the m-th core row, ct[m] = its image.  A row that sits at an end of [0, 1]
// with the residual pointing outwards (it took that end because it has no root inside) counts as solved: the
// iteration then settles, and the step is refused by the status word, not by maxit.
static void sweep_nl_core_image(pfv_ctx_impl& c, const Sweep& sw, const CsrPattern& P, const double* val,
                                const double* sink, const double* acc, const double* rhs, const double* s,
                                const double* phi, double* cb, double* ct) {
  const int32_t* ip = P.indptr;
  const int32_t* ix = P.indices;
  const int32_t* lev = sw.lev(false);
  sweep_core_rows(c, sw, OnePerRow{}, PFV_LAMBDA(int32_t i, int, int64_t m) {
    const double b = rhs[i];
    double t = sweep_nl_row_image(i, ip, ix, val, sink, acc, s, phi, lev);
    if ((s[i] == 0.0 && t > b) || (s[i] == 1.0 && t < b)) t = b;
    cb[m] = b;
    ct[m] = t;
  });
}

// the same for the components, interleaved: ccb[m k + a], cct[m k + a] of the m-th core row
static void sweep_nlc_core_image(pfv_ctx_impl& c, const Sweep& sw, const CsrPattern& P, const double* val,
                                 const double* sink, const double* acc, const double* s, const NlComp& C, double* ccb,
                                 double* cct) {
  const int32_t* ip = P.indptr;
  const int32_t* ix = P.indices;
  const int32_t* lev = sw.lev(false);
  const int k = C.k;
  sweep_core_rows(c, sw, k, PFV_LAMBDA(int32_t i, int a, int64_t w) {
    ccb[w] = C.rhs[(int64_t)i * k + a];
    cct[w] = sweep_nlc_row_image(i, a, k, ip, ix, val, sink, acc, C.ads, s, C.c, C.psi, lev);
  });
}

// before the first core iteration: the core rows start from the state of the step's start
static void sweep_nl_core_init(pfv_ctx_impl& c, const Sweep& sw, const FluxFn& F, const double* s_old, double* s,
                               double* phi) {
  sweep_core_rows(c, sw, OnePerRow{}, PFV_LAMBDA(int32_t i, int, int64_t) {
    double df;
    s[i] = s_old[i];
    phi[i] = fluxfn_eval(F, s_old[i], &df);
  });
}

// ... and so do their components: c <- c_start, psi <- phi c_start (after sweep_nl_core_init)
static void sweep_nlc_core_init(pfv_ctx_impl& c, const Sweep& sw, const double* phi, const NlComp& C) {
  const int k = C.k;
  sweep_core_rows(c, sw, k, PFV_LAMBDA(int32_t i, int a, int64_t) {
    const int64_t p = (int64_t)i * k + a;
    C.c[p] = C.c_start[p];
    C.psi[p] = phi[i] * C.c_start[p];
  });
}

// to <- from on the core rows of an interleaved vector (psi_prev <- psi before every core iteration of the saturation's
// components; the reactive step's start state and its previous iterate)
static void sweep_core_copy(pfv_ctx_impl& c, const Sweep& sw, int k, const double* from, double* to) {
  sweep_core_rows(c, sw, k, PFV_LAMBDA(int32_t i, int a, int64_t) {
    const int64_t p = (int64_t)i * k + a;
    to[p] = from[p];
  });
}

// before every core iteration: phi_prev <- phi on the core rows; the core's status word starts afresh
static void sweep_nl_core_keep(pfv_ctx_impl& c, const Sweep& sw, const double* phi, double* phi_prev,
                               int32_t* core_status) {
  sweep_core_rows(c, sw, OnePerRow{}, PFV_LAMBDA(int32_t i, int, int64_t m) {
    phi_prev[i] = phi[i];
    if (m == 0) *core_status = 0x7f7f7f7f;
  });
}

// b_ref = div (rhs_neu bc + rhs_dir diag(q) f(bc)) by the rule and in the order of upwind_assemble
static void upwind_bref_nl(pfv_ctx_impl& c, const FluxFn& F, const double* d_q, const double* bc, double* bref) {
  const int64_t nf = c.nf;
  const int32_t* cf_ptr = c.cf_ptr;
  const int32_t* cf_idx = c.cf_idx;
  const int8_t* cf_sgn = c.cf_sgn;
  const uint8_t* cls = c.upw_cls;
  const int32_t* cnt = c.upw_cnt;
  parallel_for(c.stream, c.nc, PFV_LAMBDA(int64_t cell) {
    double b = 0.0;
    for (int e = cf_ptr[cell]; e < cf_ptr[cell + 1]; ++e) {
      const int f = cf_idx[e];
      const unsigned cl = cls[f];
      if (cl & (UPW_NEU | UPW_DIRIN)) {
        double v = 0.0, df;  // the entry of rhs_neu bc + rhs_dir diag(q) f(bc) in row f
        if (cl & UPW_NEU) v = (double)(cnt[f] - cnt[nf + f]) * bc[f];
        if (cl & UPW_DIRIN) v += d_q[f] * fluxfn_eval(F, bc[f], &df);
        b += (double)cf_sgn[e] * v;
      }
    }
    bref[cell] = b;
  });
}

// b_ref of component a = div (rhs_neu cbc_a + rhs_dir diag(q) (f(bc) o cbc_a)), by the same rule and in the same face
// order: on a Dirichlet inflow face cbc is the concentration in the entering phase, on a Neumann face the component's
// flux.  cbc is component-major [k][nf] as the caller passed it, bref interleaved.
static void upwind_bref_nlc(pfv_ctx_impl& c, const FluxFn& F, int k, const double* d_q, const double* bc,
                            const double* cbc, double* bref) {
  const int64_t nf = c.nf;
  const int32_t* cf_ptr = c.cf_ptr;
  const int32_t* cf_idx = c.cf_idx;
  const int8_t* cf_sgn = c.cf_sgn;
  const uint8_t* cls = c.upw_cls;
  const int32_t* cnt = c.upw_cnt;
  parallel_for(c.stream, c.nc * k, PFV_LAMBDA(int64_t t) {
    const int64_t cell = t / k, a = t % k;
    double b = 0.0;
    for (int e = cf_ptr[cell]; e < cf_ptr[cell + 1]; ++e) {
      const int f = cf_idx[e];
      const unsigned cl = cls[f];
      if (cl & (UPW_NEU | UPW_DIRIN)) {
        const double cb = cbc[a * nf + f];
        double v = 0.0, df;
        if (cl & UPW_NEU) v = (double)(cnt[f] - cnt[nf + f]) * cb;
        if (cl & UPW_DIRIN) v += d_q[f] * (fluxfn_eval(F, bc[f], &df) * cb);
        b += (double)cf_sgn[e] * v;
      }
    }
    bref[t] = b;
  });
}

// right-hand side of the components' step: rhs_a = (acc o s_old + ads_a) o c_old_a - b_ref_a + src_a (interleaved)
static void upwind_step_rhs_nlc(pfv_ctx_impl& c, int k, const double* acc, const double* s_old, const double* ads,
                                const double* src, const double* bref, const double* x, double* rhs) {
  parallel_for(c.stream, c.nc * k, PFV_LAMBDA(int64_t t) {
    const int64_t i = t / k;
    double r = (acc[i] * s_old[i] + (ads ? ads[t] : 0.0)) * x[t];
    r -= bref[t];
    if (src) r += src[t];
    rhs[t] = r;
  });
}

// A boundary face with inflow under q that carries neither a Dirichlet nor a Neumann condition: it has no upstream
// cell.  Refused by the saturation and the reactive step alike, with one message.
constexpr const char* kUnmarkedInflowFace =
    "negative axis 1 index: -1 (neither Dirichlet nor Neumann, with inflow: no upstream cell) face ";
PFV_FN bool upwind_unmarked_inflow(int64_t f, int64_t nf, const int32_t* cnt, const uint8_t* flag, const int32_t* side,
                                   const double* d_q) {
  if (!(cnt[f] + cnt[nf + f] == 1 && flag && !(flag[f] & (PFV_BC_DIR | PFV_BC_NEU)))) return false;
  return (d_q[f] >= 0.0 ? side[f] : side[nf + f]) < 0;
}

// What the call refuses in its arrays, each with the lowest index: st[0] accumulation <= 0 or NaN, st[1] sink < 0,
// st[2] s outside [0, 1], st[3] a Dirichlet inflow value outside [0, 1], st[4] a boundary face with inflow under q that
// is neither Dirichlet nor Neumann.  With k > 0 components (component-major arrays as the caller passed them; an
// offender is reported as index * k + component, so the lowest cell or face comes first): st[5] a negative or NaN
// sorption, st[6] a non-finite c, st[7] a non-finite c_bc on a face that is read.  (0x7f7f7f7f: none.)
constexpr int kNlChecks = 8;
static void sweep_nl_check_inputs(pfv_ctx_impl& c, const double* d_q, const double* bc, const double* acc,
                                  const double* sink, const double* s, int k, const double* ads, const double* cc,
                                  const double* cbc, int32_t out[kNlChecks]) {
  stream_t st_ = c.stream;
  const int64_t nc = c.nc, nf = c.nf;
  const uint8_t* cls = c.upw_cls;
  const int32_t* side = c.upw_side;
  const int32_t* cnt = c.upw_cnt;
  const uint8_t* flag = c.have_upw_bc ? c.upw_bc.p : nullptr;
  int32_t* st = c.status.ensure(16);
  be_memset(st, 0x7f, sizeof(int32_t) * kNlChecks, st_);
  parallel_for(st_, std::max(nc, nf), PFV_LAMBDA(int64_t t) {
    const double big = 1.79769313486231570e308;
    if (t < nc) {
      if (!(acc[t] > 0.0)) atomic_min_i32(st, (int32_t)t);
      if (sink && !(sink[t] >= 0.0)) atomic_min_i32(st + 1, (int32_t)t);
      if (!(s[t] >= 0.0 && s[t] <= 1.0)) atomic_min_i32(st + 2, (int32_t)t);
      for (int a = 0; a < k; ++a) {
        if (ads && !(ads[a * nc + t] >= 0.0)) atomic_min_i32(st + 5, (int32_t)(t * k + a));
        if (!(fabs(cc[a * nc + t]) <= big)) atomic_min_i32(st + 6, (int32_t)(t * k + a));
      }
    }
    if (t < nf) {
      if ((cls[t] & UPW_DIRIN) && !(bc[t] >= 0.0 && bc[t] <= 1.0)) atomic_min_i32(st + 3, (int32_t)t);
      if (cls[t] & (UPW_NEU | UPW_DIRIN))
        for (int a = 0; a < k; ++a)
          if (!(fabs(cbc[a * nf + t]) <= big)) atomic_min_i32(st + 7, (int32_t)(t * k + a));
      if (upwind_unmarked_inflow(t, nf, cnt, flag, side, d_q)) atomic_min_i32(st + 4, (int32_t)t);
    }
  });
  be_d2h(out, st, sizeof(int32_t) * kNlChecks, st_);
}

// ---- k coupled components (pfv_transport_advance_react): per cell and component
//     acc_ia (c_ia - c_old_ia) + w_a (sum_j A_ij c_ja + b_ref_ia) + rho_i sum_b K_ab c_ib = src_ia
// with the rate matrix K of dc/dt = -K c, the mobilities w >= 0 (react.h) and the weight rho >= 0 of the reaction term.
// Once the upstream cells of a row are known its k unknowns are one k x k system
//     B_i c_i = R_i,   B_i = diag(acc_ia + w_a A_ii) + rho_i K,   R_ia = rhs_ia - w_a sum_{lev[j] < lev[i]} A_ij c_ja
// with rhs_a = acc_a o c_old_a - w_a b_ref_a + src_a.  B_i is a strictly column-diagonally-dominant M-matrix (react.h):
// it is eliminated without pivoting.  One thread per row; k is a template parameter, so that B, R and the sums are
// registers under compile-time indices and every loop over them is unrolled (a per-thread array under a run-time
// index goes to scratch memory).  The sums run in stored order and the entries are taken kNlcGroup at a time, by the
// rules of sweep_row_nlc: a slot past the row's end repeats the last entry, a slot that is not upstream reads the
// row's own rhs and enters as + 0.  With K = 0 and w = 1 the row is (rhs - sum) / (A_ii + acc), the bits of
// sweep_row_multi: w_a sum, + rho 0 and the elimination of a diagonal block are exact.
//   core   rows of the core level (c_prev != nullptr) take their in-core neighbours from c_prev, the previous
//          iterate: block Jacobi, independent of the scheduling.
//   status the lowest row with a pivot that is not positive and finite (it cannot happen with finite admissible data)
//   Dir    Ascending: the step itself, upstream = lev[j] < lev[i].  Descending: the row of the transposed system
//          M^T lambda = r of pfv_transport_adjoint_react -- val is valT (sweep_transpose_values), the cells that are
//          known are those with lev[j] > lev[i], and the caller hands a ReactPar that holds K^T, so that the block is
//          B_i^T and the elimination below is shared.  B_i^T is a strictly ROW-diagonally-dominant M-matrix: row
//          dominance is inherited by every Schur complement, so each pivot stays at least its row's excess, the growth
//          factor of the unpivoted elimination is at most 2 (Wilkinson), and there is still no pivoted path.  With
//          K = 0 and w = 1 the row gives the bits of sweep_row_multi_t.
struct ReactRow {
  const int32_t *ip, *ix, *lev;
  const double *val, *diag, *acc, *rho, *rhs;  // rho may be nullptr (1)
  const double* c_prev;
  double* c;
  int32_t* status;
};

template <int K, class Dir = Ascending>
PFV_FN void sweep_row_react(int32_t i, const ReactRow& A, const ReactPar& P) {
  const int32_t li = A.lev[i];
  const int64_t p = (int64_t)i * K;
  const int e_end = A.ip[i + 1];
  const double* own = A.rhs + p;
  double u[K];
#pragma unroll
  for (int a = 0; a < K; ++a) u[a] = 0.0;
  for (int e0 = A.ip[i]; e0 < e_end; e0 += kNlcGroup) {
    int32_t j[kNlcGroup];
    double v[kNlcGroup];
    const double* up[kNlcGroup];
#pragma unroll
    for (int t = 0; t < kNlcGroup; ++t) {
      const int e = e0 + t < e_end ? e0 + t : e_end - 1;
      j[t] = A.ix[e];
      v[t] = A.val[e];
    }
#pragma unroll
    for (int t = 0; t < kNlcGroup; ++t) {
      const int32_t lj = A.lev[j[t]];
      const bool known = Dir::reverse ? lj > li : lj < li;
      const double* src = known ? A.c : (A.c_prev && lj == li && j[t] != i ? A.c_prev : nullptr);
      up[t] = src && e0 + t < e_end ? src + (int64_t)j[t] * K : nullptr;
    }
#pragma unroll
    for (int t = 0; t < kNlcGroup; ++t) {
      const double* r = up[t] ? up[t] : own;
      const double vt = up[t] ? v[t] : 0.0;
      double x[K];
#pragma unroll
      for (int a = 0; a < K; ++a) x[a] = r[a];
#pragma unroll
      for (int a = 0; a < K; ++a) u[a] += vt * (up[t] ? x[a] : 0.0);
    }
  }
  const double rw = A.rho ? A.rho[i] : 1.0, d = A.diag[i];
  double B[K][K], R[K];
#pragma unroll
  for (int a = 0; a < K; ++a) {
    R[a] = A.rhs[p + a] - P.w[a] * u[a];
#pragma unroll
    for (int b = 0; b < K; ++b) B[a][b] = rw * P.K[a * K + b];
    B[a][a] += A.acc[p + a] + P.w[a] * d;
  }
  // elimination without pivoting: the factors by one reciprocal per pivot, the solution by a true division
  bool bad = false;
#pragma unroll
  for (int a = 0; a < K; ++a) {
    const double piv = B[a][a];
    bad = bad || !(piv > 0.0 && piv <= 1.79769313486231570e308);
    if (a + 1 < K) {
      const double inv = 1.0 / piv;
#pragma unroll
      for (int b = a + 1; b < K; ++b) {
        const double f = B[b][a] * inv;
#pragma unroll
        for (int m = a + 1; m < K; ++m) B[b][m] -= f * B[a][m];
        R[b] -= f * R[a];
      }
    }
  }
  double x[K];
#pragma unroll
  for (int a = K - 1; a >= 0; --a) {
    double s = R[a];
#pragma unroll
    for (int b = a + 1; b < K; ++b) s -= B[a][b] * x[b];
    x[a] = s / B[a][a];
  }
#pragma unroll
  for (int a = 0; a < K; ++a) A.c[p + a] = x[a];
  if (bad) atomic_min_i32(A.status, i);
}

// levels [l0, l1) of the order by the launch rule (sweep_levels); the kernel holds ReactRow and ReactPar by value.
// Dir as in sweep_levels: Descending takes a run of levels from last to first with the transposed row.
template <int K, class Dir>
static void sweep_levels_react_k(pfv_ctx_impl& c, const Sweep& sw, int l0, int l1, const ReactRow& A_,
                                 const ReactPar& P_) {
  const ReactRow A = A_;
  const ReactPar P = P_;
  sweep_levels(c, sw, false, l0, l1, OnePerRow{}, PFV_LAMBDA(int32_t i, int) { sweep_row_react<K, Dir>(i, A, P); },
               Dir{});
}

template <class Dir = Ascending>
static void sweep_levels_react(pfv_ctx_impl& c, const Sweep& sw, int l0, int l1, int k, const ReactRow& A,
                               const ReactPar& P, Dir = Dir{}) {
  switch (k) {
    case 1: sweep_levels_react_k<1, Dir>(c, sw, l0, l1, A, P); break;
    case 2: sweep_levels_react_k<2, Dir>(c, sw, l0, l1, A, P); break;
    case 3: sweep_levels_react_k<3, Dir>(c, sw, l0, l1, A, P); break;
    case 4: sweep_levels_react_k<4, Dir>(c, sw, l0, l1, A, P); break;
    case 5: sweep_levels_react_k<5, Dir>(c, sw, l0, l1, A, P); break;
    case 6: sweep_levels_react_k<6, Dir>(c, sw, l0, l1, A, P); break;
    case 7: sweep_levels_react_k<7, Dir>(c, sw, l0, l1, A, P); break;
    case 8: sweep_levels_react_k<8, Dir>(c, sw, l0, l1, A, P); break;
    default: throw Error(PFV_ERR_ARGUMENT, "k must lie in 1 .. 8");
  }
}

// the launch plan's levels in [from, to) (Descending: from last to first).  Returns the launches.
template <class Dir = Ascending>
static int sweep_apply_react(pfv_ctx_impl& c, const Sweep& sw, int from, int to, int k, const ReactRow& A,
                             const ReactPar& P, Dir = Dir{}) {
  return sweep_plan_range(sw, from, to, [&](int l0, int l1) { sweep_levels_react(c, sw, l0, l1, k, A, P, Dir{}); },
                          Dir{});
}

// After the sweep, per (row, a) in stored order: the image t_a = acc_a c_a + w_a (A c_a) + rho (K c)_a, of which
// F[i, a] = rhs_a - t_a is kept, and the scale g[i, a] = rhs_a - rho sum_{b != a} K_ab c_b: what component a is solved
// against once its partners are known (a daughter that starts from nothing has rhs_a = 0 and lives on the second term).
// par: ReactPar on the device (w, then K), read under run-time indices.  upto >= 0 (the core's stop test, before the
// levels behind the core have a c): rows behind level upto give g = F = 0, rows before it F = 0, and a row's entries
// beyond its own level (the stored zeros of the downstream side) are skipped.  descending (the transposed system: val
// is valT, par holds K^T, the levels are taken from last to first): "behind", "before" and "beyond" change sides -- the
// entries of the lower levels are the ones that do not exist yet.
static void sweep_react_image(pfv_ctx_impl& c, const CsrPattern& P, const double* val, int k, const double* acc,
                              const double* rho, const double* rhs, const double* par, const double* x,
                              const int32_t* lev, int upto, double* g, double* F, bool descending = false) {
  const int32_t* ip = P.indptr;
  const int32_t* ix = P.indices;
  const double* w = par;
  const double* Km = par + kReactMax;
  parallel_for(c.stream, P.nrows * k, PFV_LAMBDA(int64_t t) {
    const int32_t i = (int32_t)(t / k);
    const int a = (int)(t % k);
    const int32_t li = lev[i];
    if (upto >= 0 && (descending ? li < upto : li > upto)) {
      g[t] = 0.0;
      F[t] = 0.0;
      return;
    }
    double s = 0.0;
    for (int e = ip[i]; e < ip[i + 1]; ++e) {
      const int32_t j = ix[e];
      if (upto < 0 || (descending ? lev[j] >= li : lev[j] <= li)) s += val[e] * x[(int64_t)j * k + a];
    }
    const int64_t p = (int64_t)i * k;
    double kc = 0.0, off = 0.0;
    for (int b = 0; b < k; ++b) {
      const double m = Km[a * k + b] * x[p + b];
      kc += m;
      if (b != a) off += m;
    }
    const double rw = rho ? rho[i] : 1.0, r = rhs[t];
    g[t] = r - rw * off;
    const bool done = upto >= 0 && (descending ? li > upto : li < upto);
    F[t] = done ? 0.0 : r - (acc[t] * x[t] + w[a] * s + rw * kc);
  });
}

// out[a] = (g_a, g_a), out[k + a] = (F_a, F_a) of interleaved vectors of n rows
static void sweep_react_norms(pfv_ctx_impl& c, int64_t n, int k, const double* g, const double* F, double* out) {
  sweep_norms_pairs(c, n, k, out, PFV_LAMBDA(int64_t i, int a) { return NormPair{g[i * k + a], F[i * k + a]}; });
}

// What the call refuses in its arrays, each with the lowest index (component-major arrays as the caller passed them;
// an offender with a component is reported as index * k + component, so the lowest cell or face comes first):
// st[0] accumulation <= 0 or NaN, st[1] a negative or NaN rate_weight, st[2] a non-finite c, st[3] a non-finite
// bc_values on a Dirichlet inflow or Neumann face of a component with w_a > 0, st[4] a boundary face with inflow under
// q that is neither Dirichlet nor Neumann.  (0x7f7f7f7f: none.)  par: ReactPar on the device.
constexpr int kReactChecks = 5;
static void sweep_react_check_inputs(pfv_ctx_impl& c, const double* d_q, int k, const double* bc, const double* acc,
                                     const double* rho, const double* cc, const double* par,
                                     int32_t out[kReactChecks]) {
  stream_t st_ = c.stream;
  const int64_t nc = c.nc, nf = c.nf;
  const uint8_t* cls = c.upw_cls;
  const int32_t* side = c.upw_side;
  const int32_t* cnt = c.upw_cnt;
  const uint8_t* flag = c.have_upw_bc ? c.upw_bc.p : nullptr;
  int32_t* st = c.status.ensure(16);
  be_memset(st, 0x7f, sizeof(int32_t) * kReactChecks, st_);
  parallel_for(st_, std::max(nc, nf), PFV_LAMBDA(int64_t t) {
    const double big = 1.79769313486231570e308;
    if (t < nc) {
      if (rho && !(rho[t] >= 0.0)) atomic_min_i32(st + 1, (int32_t)t);
      for (int a = 0; a < k; ++a) {
        if (!(acc[a * nc + t] > 0.0)) atomic_min_i32(st, (int32_t)(t * k + a));
        if (!(fabs(cc[a * nc + t]) <= big)) atomic_min_i32(st + 2, (int32_t)(t * k + a));
      }
    }
    if (t < nf) {
      if (cls[t] & (UPW_NEU | UPW_DIRIN))
        for (int a = 0; a < k; ++a)
          if (par[a] > 0.0 && !(fabs(bc[a * nf + t]) <= big)) atomic_min_i32(st + 3, (int32_t)(t * k + a));
      if (upwind_unmarked_inflow(t, nf, cnt, flag, side, d_q)) atomic_min_i32(st + 4, (int32_t)t);
    }
  });
  be_d2h(out, st, sizeof(int32_t) * kReactChecks, st_);
}

// b_ref of every component, times its mobility: w_a div (rhs_neu + rhs_dir diag(q)) bc[a] by the rule and in the order
// of upwind_bref_multi (w_a = 1: its bits).  An immobile component (w_a = 0) gets 0 and its bc values are not read.
static void upwind_bref_react(pfv_ctx_impl& c, int k, const double* d_q, const double* bc, const double* par,
                              double* bref) {
  const int64_t nc = c.nc, nf = c.nf;
  const int32_t* cf_ptr = c.cf_ptr;
  const int32_t* cf_idx = c.cf_idx;
  const int8_t* cf_sgn = c.cf_sgn;
  const uint8_t* cls = c.upw_cls;
  const int32_t* cnt = c.upw_cnt;
  parallel_for(c.stream, nc * k, PFV_LAMBDA(int64_t t) {
    const int64_t cell = t / k, a = t % k;
    const double wa = par[a];
    double b = 0.0;
    if (wa > 0.0) {
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
      b = wa * b;
    }
    bref[t] = b;
  });
}

// ---- sorbing transport (pfv_transport_advance_sorb): per cell and component
//     acc_ia (c_ia - c_old_ia) + cap_ia (S_a(c_ia) - S_a(c_old_ia)) + sum_j A_ij c_ja + b_ref_ia = src_ia
// with the isotherm S_a of the component (isotherm.h).  The nonlinearity sits in the accumulation, the transport part is
// linear: once the upstream cells of a row are known, with D = acc + A_ii and R = rhs - sum_{lev[j] < lev[i]} A_ij c_j,
// the unknown of (row, component) is the root of  g(x) = D x + cap S(x) - R,  strictly increasing.  S(0) = 0 and S >= 0
// put the root into [0, R / D]; the right end has g = cap S >= 0, so the caller gives no upper bound.
//   items  one work item per (row, component), as sweep_row_multi: the k items of a row load val[e], ix[e] and lev[j]
//          from the same address and c[j, 0..k) as one run.  The sum runs in stored order.  Lanes of a wavefront need
//          different numbers of evaluations (and a linear component none); they wait for the slowest.
//   root   Newton from the start value clipped into the bracket; an iterate that leaves the bracket, or a |g| that did
//          not halve, is replaced by the midpoint -- an infinite slope (Freundlich n < 1 at 0) gives a step of 0, or a
//          NaN where cap S' is 0 * inf, and both fail the bracket test.  Stop: |g| <= 2^-50 (|rhs| + |sum|), the
//          magnitudes that enter R and, at the root, bound D x and cap S(x) --, or a bracket of one ulp of its upper
//          end, or kNlEvals evaluations.  (sweep_row_nl measures its bracket in [0, 1]; here the root has no scale but
//          its own, and one as small as 1e-8 is still found to rounding.)
//   leave  R < -2^-50 (|rhs| + |sum|): g(0) > 0, no root c >= 0.  The row takes 0 and records i * k + a with an integer
//          atomic minimum.  A linear component that comes out negative beyond that tolerance is recorded too.
//   sigma  the row writes sigma = S(c) beside c: the right-hand side of the next step and the image read it, so that no
//          power is evaluated outside the root-finder.
//   fold   a linear component is folded at set-up into accf = acc + cap Kd with capn = 0: its row is the division of
//          sweep_row_multi, (rhs - sum) / (A_ii + accf), and no isotherm is evaluated for it but sigma = Kd c.  So is a
//          row without capacity.
//   core   rows of the core level (c_prev != nullptr) take their in-core neighbours from c_prev, the previous iterate:
//          nonlinear Jacobi, independent of the scheduling.
struct SorbRow {
  const int32_t *ip, *ix, *lev;
  const double *val, *diag, *accf, *capn, *rhs;  // capn may be nullptr (no sorption)
  const Isotherm* iso;                           // [k], device memory
  const double* c_start;                         // the start values of the root-finder
  const double* c_prev;
  double *c, *sig;
  int32_t* status;
};

PFV_FN void sweep_row_sorb(int32_t i, int a, int k, const SorbRow& A) {
  const int32_t li = A.lev[i];
  double sum = 0.0;
  for (int e = A.ip[i]; e < A.ip[i + 1]; ++e) {
    const int32_t j = A.ix[e];
    const int32_t lj = A.lev[j];
    if (lj < li) sum += A.val[e] * A.c[(int64_t)j * k + a];
    else if (A.c_prev && lj == li && j != i) sum += A.val[e] * A.c_prev[(int64_t)j * k + a];
  }
  const int64_t p = (int64_t)i * k + a;
  const Isotherm I = A.iso[a];
  const double r = A.rhs[p], D = A.diag[i] + A.accf[p];
  const double cp = A.capn ? A.capn[p] : 0.0;
  const double tol = kNlGTol * (fabs(r) + fabs(sum));
  const double R = r - sum;
  double dS;
  if (I.kind == PFV_ISOTHERM_LINEAR) {  // folded: the division of sweep_row_multi
    const double x = (r - sum) / D;
    A.c[p] = x;
    A.sig[p] = I.p0 * x;
    if (R < -tol) atomic_min_i32(A.status, (int32_t)p);
    return;
  }
  if (!(R > 0.0)) {  // g(0) >= 0: the root is 0, or there is none
    if (R < -tol) atomic_min_i32(A.status, (int32_t)p);
    A.c[p] = 0.0;
    A.sig[p] = 0.0;
    return;
  }
  double lo = 0.0, hi = R / D;
  double x = hi, S;
  if (cp > 0.0) {
    double g_prev = 1.79769313486231570e308;
    x = A.c_start[p];
    x = x < lo ? lo : (x > hi ? hi : x);
    for (int it = 0;; ++it) {
      S = isotherm_eval(I, x, &dS);
      const double g = D * x + cp * S - R;
      if (fabs(g) <= tol || it == kNlEvals - 1) break;
      if (g > 0.0) hi = x;
      else lo = x;
      if (hi - lo <= 2.220446049250313e-16 * hi) break;
      double xn = x - g / (D + cp * dS);
      if (!(xn > lo && xn < hi) || fabs(g) > 0.5 * g_prev) xn = 0.5 * (lo + hi);
      g_prev = fabs(g);
      x = xn;
    }
  } else {
    S = isotherm_eval(I, x, &dS);
  }
  A.c[p] = x;
  A.sig[p] = S;
}

// levels [l0, l1) of the order by the launch rule (sweep_levels), k work items per row; the kernel holds SorbRow by value
static void sweep_levels_sorb(pfv_ctx_impl& c, const Sweep& sw, int l0, int l1, int k, const SorbRow& A_) {
  const SorbRow A = A_;
  sweep_levels(c, sw, false, l0, l1, k, PFV_LAMBDA(int32_t i, int a) { sweep_row_sorb(i, a, k, A); });
}

// the launch plan's levels in [from, to), outside the core.  Returns the launches.
static int sweep_apply_sorb(pfv_ctx_impl& c, const Sweep& sw, int from, int to, int k, const SorbRow& A) {
  return sweep_plan_range(sw, from, to, [&](int l0, int l1) { sweep_levels_sorb(c, sw, l0, l1, k, A); });
}

// The image and the norms in one pass: t[i, a] = sum_e A[i, e] x[j, a] + accf x + capn sigma in stored order, sigma the
// carried S(x); out[a] = (rhs_a, rhs_a) over all rows, out[k + a] = (F_a, F_a), F = rhs - t.  core >= 0 (the core's stop
// test, before the levels behind it have a value): F of the core rows alone, from the entries up to the core level.
static void sweep_sorb_norms(pfv_ctx_impl& c, const CsrPattern& P, const double* val, int k, const double* accf,
                             const double* capn, const double* rhs, const double* x, const double* sig,
                             const int32_t* lev, int32_t core, double* out) {
  const int32_t* ip = P.indptr;
  const int32_t* ix = P.indices;
  sweep_norms_pairs(c, P.nrows, k, out, PFV_LAMBDA(int64_t i, int a) {
    const int64_t p = i * k + a;
    const double ri = rhs[p];
    if (core >= 0 && lev[i] != core) return NormPair{ri, 0.0};
    double t = 0.0;
    for (int e = ip[i]; e < ip[i + 1]; ++e) {
      const int32_t j = ix[e];
      if (core < 0 || lev[j] <= core) t += val[e] * x[(int64_t)j * k + a];
    }
    t += accf[p] * x[p];
    if (capn) t += capn[p] * sig[p];
    return NormPair{ri, ri - t};
  });
}

// The set-up on the interleaved vectors: the folded accumulation accf and the root-finder's capacity capn (cap may be
// nullptr: then capn is not written), and sigma = S(c0) of the state the call starts from.
static void sweep_sorb_setup(pfv_ctx_impl& c, int k, const Isotherm* iso, const double* acc, const double* cap,
                             const double* x, double* accf, double* capn, double* sig) {
  parallel_for(c.stream, c.nc * k, PFV_LAMBDA(int64_t t) {
    const Isotherm I = iso[t % k];
    const bool lin = I.kind == PFV_ISOTHERM_LINEAR;
    double dS;
    accf[t] = lin && cap ? acc[t] + cap[t] * I.p0 : acc[t];
    if (cap) capn[t] = lin ? 0.0 : cap[t];
    sig[t] = isotherm_eval(I, x[t], &dS);
  });
}

// right-hand side of the step: rhs = accf c_old - b_ref + src + capn sigma_old (interleaved).  Up to the last term it is
// the expression of upwind_step_rhs_multi, which a linear component (capn = 0) then has bit for bit.
static void upwind_step_rhs_sorb(pfv_ctx_impl& c, int k, const double* accf, const double* capn, const double* src,
                                 const double* bref, const double* x, const double* sig, double* rhs) {
  parallel_for(c.stream, c.nc * k, PFV_LAMBDA(int64_t t) {
    double r = accf[t] * x[t];
    r -= bref[t];
    if (src) r += src[t];
    if (capn) r += capn[t] * sig[t];
    rhs[t] = r;
  });
}

// What the call refuses in its arrays, each with the lowest index (component-major arrays as the caller passed them; an
// offender is reported as index * k + component, so the lowest cell or face comes first): st[0] accumulation <= 0 or
// NaN, st[1] a negative or NaN capacity, st[2] a c that is negative or not finite, st[3] a Dirichlet inflow value that
// is negative or not finite, st[4] a non-finite Neumann value, st[5] a boundary face with inflow under q that is neither
// Dirichlet nor Neumann.  (0x7f7f7f7f: none.)
constexpr int kSorbChecks = 6;
static void sweep_sorb_check_inputs(pfv_ctx_impl& c, const double* d_q, int k, const double* bc, const double* acc,
                                    const double* cap, const double* cc, int32_t out[kSorbChecks]) {
  stream_t st_ = c.stream;
  const int64_t nc = c.nc, nf = c.nf;
  const uint8_t* cls = c.upw_cls;
  const int32_t* side = c.upw_side;
  const int32_t* cnt = c.upw_cnt;
  const uint8_t* flag = c.have_upw_bc ? c.upw_bc.p : nullptr;
  int32_t* st = c.status.ensure(16);
  be_memset(st, 0x7f, sizeof(int32_t) * kSorbChecks, st_);
  parallel_for(st_, std::max(nc, nf), PFV_LAMBDA(int64_t t) {
    const double big = 1.79769313486231570e308;
    if (t < nc) {
      for (int a = 0; a < k; ++a) {
        if (!(acc[a * nc + t] > 0.0)) atomic_min_i32(st, (int32_t)(t * k + a));
        if (cap && !(cap[a * nc + t] >= 0.0)) atomic_min_i32(st + 1, (int32_t)(t * k + a));
        if (!(cc[a * nc + t] >= 0.0 && cc[a * nc + t] <= big)) atomic_min_i32(st + 2, (int32_t)(t * k + a));
      }
    }
    if (t < nf) {
      for (int a = 0; a < k; ++a) {
        const double v = bc[a * nf + t];
        if ((cls[t] & UPW_DIRIN) && !(v >= 0.0 && v <= big)) atomic_min_i32(st + 3, (int32_t)(t * k + a));
        if ((cls[t] & UPW_NEU) && !(fabs(v) <= big)) atomic_min_i32(st + 4, (int32_t)(t * k + a));
      }
      if (upwind_unmarked_inflow(t, nf, cnt, flag, side, d_q)) atomic_min_i32(st + 5, (int32_t)t);
    }
  });
  be_d2h(out, st, sizeof(int32_t) * kSorbChecks, st_);
}

// ---- the adjoint of the k-component step (pfv_transport_adjoint_multi): S_a^T lambda_a = r_a.  S_a = diag(acc_a) + A is
// triangular in flow order, S_a^T in reverse flow order: one substitution over the same levels from last to first.
//   tpos    the pattern of A (a cell and its face neighbours) is structurally symmetric: tpos[e] is the position of
//           (j, i) for the entry e = (i, j).  A property of the pattern, kept with it.
//   valT    valT[e] = val[tpos[e]], once per assembly: row i of valT is column i of A on the pattern of row i, so the
//           transposed row has the load chain of sweep_row_multi -- no search in a level, no atomics.
// first entry without a partner in tpos' status word (0x7f7f7f7f: none)
static void sweep_transpose_positions(pfv_ctx_impl& c, const CsrPattern& P, int32_t* tpos,
                                      const char* what = "the transport system") {
  stream_t s = c.stream;
  const int32_t* ip = P.indptr;
  const int32_t* ix = P.indices;
  int32_t* st = c.status.ensure(16);
  be_memset(st, 0x7f, sizeof(int32_t), s);
  parallel_for(s, P.nrows, PFV_LAMBDA(int64_t i) {
    for (int e = ip[i]; e < ip[i + 1]; ++e) {
      const int32_t j = ix[e];
      const int b0 = ip[j], len = ip[j + 1] - b0;
      const int pos = lower_bound_idx<int32_t>(ix + b0, len, (int32_t)i);
      const bool found = pos < len && ix[b0 + pos] == (int32_t)i;
      tpos[e] = found ? b0 + pos : e;  // (an address inside the values in any case)
      if (!found) atomic_min_i32(st, e);
    }
  });
  const int32_t bad = read_scalar<int32_t>(s, st);
  if (bad != 0x7f7f7f7f)
    throw Error(PFV_ERR_UNSUPPORTED, std::string("the pattern of ") + what + " is not structurally symmetric (entry " +
                                         std::to_string(bad) + " has no transposed partner)");
}

static void sweep_transpose_values(pfv_ctx_impl& c, int64_t nnz, const int32_t* tpos, const double* val, double* valT) {
  parallel_for(c.stream, nnz, PFV_LAMBDA(int64_t e) { valT[e] = val[tpos[e]]; });
}

// one (row, component) of the transposed substitution: the cells downstream of i have the higher levels
PFV_FN void sweep_row_multi_t(int32_t i, int a, int k, const int32_t* ip, const int32_t* ix, const double* valT,
                              const double* diag, const double* acc, const int32_t* lev, const double* r, double* z) {
  const int32_t li = lev[i];
  double sum = 0.0;
  for (int e = ip[i]; e < ip[i + 1]; ++e) {
    const int32_t j = ix[e];
    if (lev[j] > li) sum += valT[e] * z[(int64_t)j * k + a];
  }
  const int64_t p = (int64_t)i * k + a;
  z[p] = (r[p] - sum) / (diag[i] + acc[p]);
}

// ... of the core level: the in-core neighbours from z_prev, the previous iterate (Jacobi, independent of the scheduling)
PFV_FN void sweep_row_multi_t_core(int32_t i, int a, int k, const int32_t* ip, const int32_t* ix, const double* valT,
                                   const double* diag, const double* acc, const int32_t* lev, const double* r,
                                   const double* z_prev, double* z) {
  const int32_t li = lev[i];
  double sum = 0.0;
  for (int e = ip[i]; e < ip[i + 1]; ++e) {
    const int32_t j = ix[e];
    const int32_t lj = lev[j];
    if (lj > li) sum += valT[e] * z[(int64_t)j * k + a];
    else if (lj == li && j != i) sum += valT[e] * z_prev[(int64_t)j * k + a];
  }
  const int64_t p = (int64_t)i * k + a;
  z[p] = (r[p] - sum) / (diag[i] + acc[p]);
}

// the launch plan's levels in [from, to), from last to first.  Returns the launches.
static int sweep_apply_multi_t(pfv_ctx_impl& c, const Sweep& sw, int from, int to, const CsrPattern& P,
                               const double* valT, const double* diag, const double* acc, int k, const double* in,
                               double* out) {
  const int32_t* ip = P.indptr;
  const int32_t* ix = P.indices;
  const int32_t* lev = sw.lev(false);
  return sweep_plan_range(sw, from, to, [&](int l0, int l1) {
    sweep_levels(c, sw, false, l0, l1, k,
                 PFV_LAMBDA(int32_t i, int a) { sweep_row_multi_t(i, a, k, ip, ix, valT, diag, acc, lev, in, out); },
                 Descending{});
  }, Descending{});
}

// one Jacobi iteration of the core level on its transposed rows
static void sweep_core_multi_t(pfv_ctx_impl& c, const Sweep& sw, const CsrPattern& P, const double* valT,
                               const double* diag, const double* acc, int k, const double* in, const double* prev,
                               double* out) {
  const int32_t* ip = P.indptr;
  const int32_t* ix = P.indices;
  const int32_t* lev = sw.lev(false);
  sweep_core_rows(c, sw, k, PFV_LAMBDA(int32_t i, int a, int64_t) {
    sweep_row_multi_t_core(i, a, k, ip, ix, valT, diag, acc, lev, in, prev, out);
  });
}

// to <- 0 on the core rows of an interleaved vector (the start of the core's iteration)
static void sweep_core_zero(pfv_ctx_impl& c, const Sweep& sw, int k, double* to) {
  sweep_core_rows(c, sw, k, PFV_LAMBDA(int32_t i, int a, int64_t) { to[(int64_t)i * k + a] = 0.0; });
}

// The core's stop test: out[a] = (r_a, r_a) over all rows, out[k + a] = the squared residual of the core rows, the
// image taken from the entries of the row's own level and above (the levels below have no value yet; their entries
// are the stored zeros of the upstream side).
static void sweep_core_norms_multi_t(pfv_ctx_impl& c, const Sweep& sw, const CsrPattern& P, const double* valT,
                                     const double* acc, int k, const double* r, const double* x, double* out) {
  const int32_t* ip = P.indptr;
  const int32_t* ix = P.indices;
  const int32_t* lev = sw.lev(false);
  const int32_t core = sw.core_level;
  sweep_norms_pairs(c, P.nrows, k, out, PFV_LAMBDA(int64_t i, int a) {
    const int64_t p = i * k + a;
    const double ri = r[p];
    if (lev[i] != core) return NormPair{ri, 0.0};
    double t = 0.0;
    for (int e = ip[i]; e < ip[i + 1]; ++e) {
      const int32_t j = ix[e];
      if (lev[j] >= core) t += valT[e] * x[(int64_t)j * k + a];
    }
    t += acc[p] * x[p];
    return NormPair{ri, ri - t};
  });
}

// The right-hand side of adjoint step n, r = g^n + acc o lambda^{n+1}, fused with what lambda^{n+1} adds to the
// gradients that live on the cells: grad_source += lambda^{n+1}, grad_accumulation += lambda^{n+1} o (c^n - c^{n+1}).
// lam == nullptr (the first step): r = g^n.  loads == nullptr (after the last step): r = acc o lambda^1 = grad_c0.
// loads is [k][n_obs]; slot[i] is the position of cell i among the observation cells (-1: not observed; slot ==
// nullptr: every cell, in order).  Interleaved vectors; c_n, c_np1 only with gacc.
static void adjoint_step_rhs(pfv_ctx_impl& c, int k, const double* acc, const double* lam, const int32_t* slot,
                             const double* loads, int64_t n_obs, const double* c_n, const double* c_np1, double* gsrc,
                             double* gacc, double* r) {
  parallel_for(c.stream, c.nc * k, PFV_LAMBDA(int64_t t) {
    const int64_t i = t / k, a = t % k;
    double g = 0.0;
    if (loads) {
      const int64_t m = slot ? (int64_t)slot[i] : i;
      if (m >= 0) g = loads[a * n_obs + m];
    }
    double v = g;
    if (lam) {
      const double l = lam[t];
      v = g + acc[t] * l;
      if (gsrc) gsrc[t] += l;
      if (gacc) gacc[t] += l * (c_n[t] - c_np1[t]);
    }
    r[t] = v;
  });
}

// slot[obs[m]] = m (slot preset to -1)
static void adjoint_obs_slots(pfv_ctx_impl& c, int64_t n_obs, const int32_t* obs, int32_t* slot) {
  parallel_for(c.stream, n_obs, PFV_LAMBDA(int64_t m) { slot[obs[m]] = (int32_t)m; });
}

// first non-finite entry of v[0 .. n), -1: none
static int64_t adjoint_first_nonfinite(pfv_ctx_impl& c, int64_t n, const double* v) {
  stream_t s = c.stream;
  int32_t* st = c.status.ensure(16);
  be_memset(st, 0x7f, sizeof(int32_t), s);
  parallel_for(s, n, PFV_LAMBDA(int64_t t) {
    if (!(fabs(v[t]) <= 1.79769313486231570e308)) atomic_min_i32(st, (int32_t)t);
  });
  const int32_t bad = read_scalar<int32_t>(s, st);
  return bad == 0x7f7f7f7f ? -1 : (int64_t)bad;
}

// grad_bc_values[a][f] -= sum_i B[i, f] lambda[i, a], B = div (rhs_neu + rhs_dir diag(q)): the transpose of
// upwind_bref_multi.  One work item per (face, component); a face reads the cells on its two sides (a boundary face
// has one).  gbc is component-major [k][nf], lam interleaved.  par (may be nullptr: every mobility 1): ReactPar on the
// device -- the term is scaled by w_a, and an immobile component (w_a = 0) keeps its zeros.
static void adjoint_grad_bc(pfv_ctx_impl& c, int k, const double* d_q, const double* lam, double* gbc,
                            const double* par = nullptr) {
  const int64_t nf = c.nf;
  const uint8_t* cls = c.upw_cls;
  const int32_t* cnt = c.upw_cnt;
  const int32_t* side = c.upw_side;
  parallel_for(c.stream, nf * k, PFV_LAMBDA(int64_t t) {
    const int64_t f = t / k, a = t % k;
    const unsigned cl = cls[f];
    if (!(cl & (UPW_NEU | UPW_DIRIN))) return;
    const double wa = par ? par[a] : 1.0;
    if (!(wa > 0.0)) return;
    double m = 0.0;
    if (cl & UPW_NEU) m = (double)(cnt[f] - cnt[nf + f]);
    if (cl & UPW_DIRIN) m += 1.0 * d_q[f];
    const int32_t cp = side[f], cm = side[nf + f];
    double s = 0.0;
    if (cp >= 0) s += m * lam[(int64_t)cp * k + a];
    if (cm >= 0) s -= m * lam[(int64_t)cm * k + a];
    gbc[a * nf + f] -= wa * s;  // (w_a = 1: the bits of the unscaled term)
  });
}

// grad_flux[f] -= sum_a (lambda[p, a] - lambda[m, a]) cup[a, f] with p / m the cells on the +1 / -1 side of f and cup the
// value the upwind rule takes at f: the upstream cell's c^n (interior and outflow faces), the boundary value (Dirichlet
// inflow); a Neumann face gives 0.  One work item per face, the components summed in order.  bc is component-major.
// par (may be nullptr: every mobility 1): ReactPar on the device -- component a enters with w_a, and an immobile one
// (w_a = 0) is skipped, not multiplied: its boundary values are not read (they may be NaN).
static void adjoint_grad_flux(pfv_ctx_impl& c, int k, const double* bc, const double* lam, const double* c_n,
                              double* gq, const double* par = nullptr) {
  const int64_t nf = c.nf;
  const uint8_t* cls = c.upw_cls;
  const int32_t* up = c.upw_up;
  const int32_t* side = c.upw_side;
  parallel_for(c.stream, nf, PFV_LAMBDA(int64_t f) {
    const unsigned cl = cls[f];
    if (!(cl & (UPW_KEPT | UPW_DIRIN))) return;
    const int32_t cp = side[f], cm = side[nf + f];
    const int32_t u = up[f];
    double s = 0.0;
    for (int a = 0; a < k; ++a) {
      const double wa = par ? par[a] : 1.0;
      if (!(wa > 0.0)) continue;
      double d = 0.0;
      if (cp >= 0) d = lam[(int64_t)cp * k + a];
      if (cm >= 0) d -= lam[(int64_t)cm * k + a];
      const double cup = (cl & UPW_KEPT) ? c_n[(int64_t)u * k + a] : bc[a * nf + f];
      s += (wa * d) * cup;  // (w_a = 1: the bits of d * cup)
    }
    gq[f] -= s;
  });
}

// ---- the gradients of pfv_transport_adjoint_react with respect to the reaction term rho_i sum_b K_ab c_ib, after an
// accepted step (lam = lambda^n, c_n = c^n, both interleaved):
//     grad_rate_weight[i] -= sum_a lambda_ia sum_b K_ab c_ib      one work item per row, the sums in index order
//     grad_rate[a][b]     -= sum_i rho_i lambda_ia c_ib           k^2 sums over all rows
// The k^2 sums take a fixed partition that depends on the number of rows and k alone, in the manner of
// sweep_norms_pairs: a workgroup takes a range of rows, slot g * k^2 + (a k + b) of it the rows lo + g, lo + g + G, ...
// of the pair (a, b) (G = 256 / k^2), the G sums of a pair are folded pairwise in LDS, and one workgroup per pair adds
// the workgroups' partial sums and subtracts the result from the pair's accumulator: the steps add in step order.  No
// floating-point atomics, no per-thread array.  Km: the caller's K on the device (not the transposed one).
static void adjoint_grad_rate_weight(pfv_ctx_impl& c, int k, const double* Km, const double* lam, const double* c_n,
                                     double* grho) {
  parallel_for(c.stream, c.nc, PFV_LAMBDA(int64_t i) {
    const int64_t p = i * k;
    double s = 0.0;
    for (int a = 0; a < k; ++a) {
      double kc = 0.0;
      for (int b = 0; b < k; ++b) kc += Km[a * k + b] * c_n[p + b];
      s += lam[p + a] * kc;
    }
    grho[i] -= s;
  });
}

static void adjoint_grad_rate(pfv_ctx_impl& c, int k, const double* rho, const double* lam, const double* c_n,
                              double* gK) {
  stream_t s = c.stream;
  const int64_t n = c.nc;
  const int P = k * k, G = 256 / P, slots = G * P;
  const int nb = (int)std::min<int64_t>(kGmresBlocks, (n * P + 2047) / 2048);
  int fold = 1;
  while (fold < G) fold <<= 1;
  double* partial = c.red.ensure((size_t)kReactMax * kReactMax * kGmresBlocks + 64);
  block_for<256>(s, nb, 256 * sizeof(double), PFV_LAMBDA(const WaveCtx& w) {
    double* sh = reinterpret_cast<double*>(w.lds);
    const int64_t blk = w.item;
    const int64_t lo = n * blk / nb, hi = n * (blk + 1) / nb;
    PFV_LANES(slot, slots) {
      const int pair = slot % P, g = slot / P;
      const int a = pair / k, b = pair % k;
      double sum = 0.0;
      for (int64_t i = lo + g; i < hi; i += G) sum += ((rho ? rho[i] : 1.0) * lam[i * k + a]) * c_n[i * k + b];
      sh[slot] = sum;
    }
    w.sync();
    for (int o = fold >> 1; o > 0; o >>= 1) {
      PFV_LANES(slot, slots) {
        if (slot / P < o && slot / P + o < G) sh[slot] += sh[slot + o * P];
      }
      w.sync();
    }
    PFV_LANES(pair, P) { partial[(int64_t)pair * nb + blk] = sh[pair]; }
    w.sync();
  });
  block_for<256>(s, P, 256 * sizeof(double), PFV_LAMBDA(const WaveCtx& wc) {
    double* sh = reinterpret_cast<double*>(wc.lds);
    const int64_t m = wc.item;
    double a = 0.0;
    for (int i = wc.lane; i < nb; i += wc.width) a += partial[m * nb + i];
    sh[wc.lane] = a;
    wc.sync();
    for (int o = wc.width >> 1; o > 0; o >>= 1) {
      if (wc.lane < o) sh[wc.lane] += sh[wc.lane + o];
      wc.sync();
    }
    if (wc.lane0()) gK[m] -= sh[0];
    wc.sync();
  });
}

// ---- the adjoint of the saturation step (pfv_transport_adjoint_nl).  The step acc o (s - s_old) + M f(s) + b_ref = src,
// M = A + diag(sink), has the Jacobian J = diag(acc) + M diag(d) with d = f'(s^n), so that
//     J^T lambda = (diag(acc) + diag(d) M^T) lambda = r
// and row i, once the cells downstream of it are known, is one division:
//     lambda_i = (r_i - d_i sum_{lev[j] > lev[i]} valT[e] lambda_j) / (acc_i + d_i (A_ii + sink_i)).
// No root-finding and no pow in a level: d and phi = f(s^n) come from ONE streaming pass over the step's slab of states
// (adjoint_nl_slopes).  J is strictly column-diagonally dominant (acc > 0, M an M-matrix by columns), so Jacobi on the
// transposed rows of a cyclic core converges; a row with d_i = 0 (a cell at or beyond a residual saturation) is
// acc_i lambda_i = r_i.  The levels, the launch plan and the load chain of a row are those of sweep_row_multi_t.
static void adjoint_nl_slopes(pfv_ctx_impl& c, const FluxFn& F, const double* s, double* d, double* phi) {
  parallel_for(c.stream, c.nc, PFV_LAMBDA(int64_t i) {
    double df;
    phi[i] = fluxfn_eval(F, s[i], &df);
    d[i] = df;
  });
}

PFV_FN void sweep_row_nl_t(int32_t i, const int32_t* ip, const int32_t* ix, const double* valT, const double* diag,
                           const double* sink, const double* acc, const double* d, const int32_t* lev, const double* r,
                           double* z) {
  const int32_t li = lev[i];
  double sum = 0.0;
  for (int e = ip[i]; e < ip[i + 1]; ++e) {
    const int32_t j = ix[e];
    if (lev[j] > li) sum += valT[e] * z[j];
  }
  const double di = d[i];
  z[i] = (r[i] - di * sum) / (acc[i] + di * (diag[i] + (sink ? sink[i] : 0.0)));
}

// ... of the core level: the in-core neighbours from z_prev, the previous iterate (Jacobi, independent of the scheduling)
PFV_FN void sweep_row_nl_t_core(int32_t i, const int32_t* ip, const int32_t* ix, const double* valT, const double* diag,
                                const double* sink, const double* acc, const double* d, const int32_t* lev,
                                const double* r, const double* z_prev, double* z) {
  const int32_t li = lev[i];
  double sum = 0.0;
  for (int e = ip[i]; e < ip[i + 1]; ++e) {
    const int32_t j = ix[e];
    const int32_t lj = lev[j];
    if (lj > li) sum += valT[e] * z[j];
    else if (lj == li && j != i) sum += valT[e] * z_prev[j];
  }
  const double di = d[i];
  z[i] = (r[i] - di * sum) / (acc[i] + di * (diag[i] + (sink ? sink[i] : 0.0)));
}

// the launch plan's levels in [from, to), from last to first.  Returns the launches.
static int sweep_apply_nl_t(pfv_ctx_impl& c, const Sweep& sw, int from, int to, const CsrPattern& P, const double* valT,
                            const double* diag, const double* sink, const double* acc, const double* d,
                            const double* in, double* out) {
  const int32_t* ip = P.indptr;
  const int32_t* ix = P.indices;
  const int32_t* lev = sw.lev(false);
  return sweep_plan_range(sw, from, to, [&](int l0, int l1) {
    sweep_levels(c, sw, false, l0, l1, OnePerRow{},
                 PFV_LAMBDA(int32_t i, int) { sweep_row_nl_t(i, ip, ix, valT, diag, sink, acc, d, lev, in, out); },
                 Descending{});
  }, Descending{});
}

// one Jacobi iteration of the core level on its transposed rows
static void sweep_core_nl_t(pfv_ctx_impl& c, const Sweep& sw, const CsrPattern& P, const double* valT,
                            const double* diag, const double* sink, const double* acc, const double* d,
                            const double* in, const double* prev, double* out) {
  const int32_t* ip = P.indptr;
  const int32_t* ix = P.indices;
  const int32_t* lev = sw.lev(false);
  sweep_core_rows(c, sw, OnePerRow{}, PFV_LAMBDA(int32_t i, int, int64_t) {
    sweep_row_nl_t_core(i, ip, ix, valT, diag, sink, acc, d, lev, in, prev, out);
  });
}

// (M^T x)_i = sum_e valT[e] x_j + sink_i x_i in stored order; from >= 0: the entries of the levels from `from` on alone
PFV_FN double sweep_nl_t_row_image(int64_t i, const int32_t* ip, const int32_t* ix, const double* valT,
                                   const double* sink, const double* x, const int32_t* lev, int32_t from) {
  double t = 0.0;
  for (int e = ip[i]; e < ip[i + 1]; ++e) {
    const int32_t j = ix[e];
    if (from < 0 || lev[j] >= from) t += valT[e] * x[j];
  }
  if (sink) t += sink[i] * x[i];
  return t;
}

// The acceptance check: out[0] = (r, r), out[1] = (r - J^T x, r - J^T x) over all rows.  core_only (the core's stop test):
// out[1] is the squared residual of the core rows, the image taken from the entries of the row's own level and above
// (the levels below have no value yet; their entries are the stored zeros of the upstream side).
static void sweep_norms_nl_t(pfv_ctx_impl& c, const Sweep& sw, const CsrPattern& P, const double* valT,
                             const double* sink, const double* acc, const double* d, const double* r, const double* x,
                             bool core_only, double* out) {
  const int32_t* ip = P.indptr;
  const int32_t* ix = P.indices;
  const int32_t* lev = sw.lev(false);
  const int32_t core = core_only ? sw.core_level : -1;
  sweep_norms_pairs(c, P.nrows, 1, out, PFV_LAMBDA(int64_t i, int) {
    const double ri = r[i];
    if (core >= 0 && lev[i] != core) return NormPair{ri, 0.0};
    const double t = acc[i] * x[i] + d[i] * sweep_nl_t_row_image(i, ip, ix, valT, sink, x, lev, core);
    return NormPair{ri, ri - t};
  });
}

// grad_sink[i] -= lambda_i phi_i (the sink takes fluid at the cell's own f(s))
static void adjoint_nl_grad_sink(pfv_ctx_impl& c, const double* lam, const double* phi, double* gsink) {
  parallel_for(c.stream, c.nc, PFV_LAMBDA(int64_t i) { gsink[i] -= lam[i] * phi[i]; });
}

// grad_bc_values[f] -= m_f (lambda[p] - lambda[m]), m_f the derivative of the entry of rhs_neu bc + rhs_dir diag(q) f(bc)
// in row f (upwind_bref_nl) with respect to bc_f: the Neumann count, q_f f'(bc_f) on a Dirichlet inflow face.  With
// f(s) = s these are the bits of adjoint_grad_bc.
static void adjoint_nl_grad_bc(pfv_ctx_impl& c, const FluxFn& F, const double* d_q, const double* bc, const double* lam,
                               double* gbc) {
  const int64_t nf = c.nf;
  const uint8_t* cls = c.upw_cls;
  const int32_t* cnt = c.upw_cnt;
  const int32_t* side = c.upw_side;
  parallel_for(c.stream, nf, PFV_LAMBDA(int64_t f) {
    const unsigned cl = cls[f];
    if (!(cl & (UPW_NEU | UPW_DIRIN))) return;
    double m = 0.0;
    if (cl & UPW_NEU) m = (double)(cnt[f] - cnt[nf + f]);
    if (cl & UPW_DIRIN) {
      double df;
      fluxfn_eval(F, bc[f], &df);
      m += df * d_q[f];
    }
    const int32_t cp = side[f], cm = side[nf + f];
    double s = 0.0;
    if (cp >= 0) s += m * lam[cp];
    if (cm >= 0) s -= m * lam[cm];
    gbc[f] -= s;
  });
}

// grad_flux[f] -= (lambda[p] - lambda[m]) phiup_f with phiup the value the upwind rule moves through f: phi = f(s^n) of
// the upstream cell (interior and outflow faces), f(bc_f) on a Dirichlet inflow face; a Neumann face gives 0.  The
// upstream side is fixed, as in adjoint_grad_flux.
static void adjoint_nl_grad_flux(pfv_ctx_impl& c, const FluxFn& F, const double* bc, const double* lam,
                                 const double* phi, double* gq) {
  const int64_t nf = c.nf;
  const uint8_t* cls = c.upw_cls;
  const int32_t* up = c.upw_up;
  const int32_t* side = c.upw_side;
  parallel_for(c.stream, nf, PFV_LAMBDA(int64_t f) {
    const unsigned cl = cls[f];
    if (!(cl & (UPW_KEPT | UPW_DIRIN))) return;
    const int32_t cp = side[f], cm = side[nf + f];
    double d = 0.0, df;
    if (cp >= 0) d = lam[cp];
    if (cm >= 0) d -= lam[cm];
    const double pu = (cl & UPW_KEPT) ? phi[up[f]] : fluxfn_eval(F, bc[f], &df);
    gq[f] -= d * pu;
  });
}

// grad_fluxfn[m] -= sum_i (M^T lambda)_i df/dtheta_m(s_i) + sum_{Dirichlet inflow f} (lambda[p] - lambda[m]) q_f
// df/dtheta_m(bc_f) for the six Corey parameters (fluxfn_eval_params).  The terms are the cells in index order, then the
// faces: item t < nc is cell t -- its (M^T lambda) from the valT row in stored order --, item nc + f is face f.  The six
// sums take a fixed partition that depends on the numbers of cells and faces alone: a workgroup takes a range of the
// items, lane l of it the items lo + l, lo + l + 256, ... with its six sums in registers, the 256 lanes' sums are folded
// pairwise in LDS, and one workgroup per parameter adds the workgroups' partial sums and subtracts the result from the
// parameter's accumulator: the steps add in step order.  No floating-point atomics, no per-thread array under a
// run-time index.
// The scheme with the two weights as functors: cell_w(i) is the weight of cell i, face_w(f) that of the Dirichlet inflow
// face f.  adjoint_nl_grad_fluxfn hands in the weights above; the step with phase-carried components adds the
// components' terms to both (adjoint_nlc_grad_fluxfn).
template <class CellW, class FaceW>
static void adjoint_nl_grad_fluxfn_weighted(pfv_ctx_impl& c, const FluxFn& F, const double* bc, const double* s_n,
                                            double* gF, CellW cell_w, FaceW face_w) {
  stream_t s = c.stream;
  const int64_t nc = c.nc, nf = c.nf, n = nc + nf;
  const uint8_t* cls = c.upw_cls;
  const int nb = (int)std::min<int64_t>(kGmresBlocks, (n + 2047) / 2048);
  double* partial = c.red.ensure(6 * (size_t)kGmresBlocks + 64);
  block_for<256>(s, nb, 6 * 256 * sizeof(double), PFV_LAMBDA(const WaveCtx& w) {
    double* sh = reinterpret_cast<double*>(w.lds);
    const int64_t blk = w.item;
    const int64_t lo = n * blk / nb, hi = n * (blk + 1) / nb;
    PFV_LANES(l, 256) {
      double a0 = 0.0, a1 = 0.0, a2 = 0.0, a3 = 0.0, a4 = 0.0, a5 = 0.0;
      for (int64_t t = lo + l; t < hi; t += 256) {
        double wt = 0.0, at = 0.0;  // the weight of the item and the saturation its derivatives are taken at
        bool live = false;
        if (t < nc) {
          wt = cell_w(t);
          at = s_n[t];
          live = true;
        } else {
          const int64_t f = t - nc;
          if (cls[f] & UPW_DIRIN) {
            wt = face_w(f);
            at = bc[f];
            live = true;
          }
        }
        if (live) {
          double dp[6];
          fluxfn_eval_params(F, at, dp);
          a0 += wt * dp[0];
          a1 += wt * dp[1];
          a2 += wt * dp[2];
          a3 += wt * dp[3];
          a4 += wt * dp[4];
          a5 += wt * dp[5];
        }
      }
      sh[l] = a0;
      sh[256 + l] = a1;
      sh[512 + l] = a2;
      sh[768 + l] = a3;
      sh[1024 + l] = a4;
      sh[1280 + l] = a5;
    }
    w.sync();
    for (int o = 128; o > 0; o >>= 1) {
      PFV_LANES(l, o) {
        for (int m = 0; m < 6; ++m) sh[m * 256 + l] += sh[m * 256 + l + o];
      }
      w.sync();
    }
    PFV_LANES(m, 6) { partial[(int64_t)m * nb + blk] = sh[m * 256]; }
    w.sync();
  });
  block_for<256>(s, 6, 256 * sizeof(double), PFV_LAMBDA(const WaveCtx& wc) {
    double* sh = reinterpret_cast<double*>(wc.lds);
    const int64_t m = wc.item;
    double a = 0.0;
    for (int i = wc.lane; i < nb; i += wc.width) a += partial[m * nb + i];
    sh[wc.lane] = a;
    wc.sync();
    for (int o = wc.width >> 1; o > 0; o >>= 1) {
      if (wc.lane < o) sh[wc.lane] += sh[wc.lane + o];
      wc.sync();
    }
    if (wc.lane0()) gF[m] -= sh[0];
    wc.sync();
  });
}

static void adjoint_nl_grad_fluxfn(pfv_ctx_impl& c, const FluxFn& F, const CsrPattern& P, const double* valT,
                                   const double* sink, const double* d_q, const double* bc, const double* lam,
                                   const double* s_n, double* gF) {
  const int64_t nf = c.nf;
  const int32_t* ip = P.indptr;
  const int32_t* ix = P.indices;
  const int32_t* side = c.upw_side;
  adjoint_nl_grad_fluxfn_weighted(c, F, bc, s_n, gF, PFV_LAMBDA(int64_t t) {
    return sweep_nl_t_row_image(t, ip, ix, valT, sink, lam, nullptr, -1);
  }, PFV_LAMBDA(int64_t f) {
    const int32_t cp = side[f], cm = side[nf + f];
    double dl = 0.0;
    if (cp >= 0) dl = lam[cp];
    if (cm >= 0) dl -= lam[cm];
    return dl * d_q[f];
  });
}

// ---- the adjoint of the saturation step with phase-carried components (pfv_transport_adjoint_nl_multi).  With the
// multipliers lambda of the saturation's equation and mu_a of component a's, e_a = acc o s^n + ads_a, phi = f(s^n),
// d = f'(s^n) and M = A + diag(sink), step n solves
//     (diag(e_a) + diag(phi) M^T) mu_a = rmu_a                                                        (a = 0 .. k-1)
//     (diag(acc) + diag(d) M^T) lambda = rl - sum_a c_a^n o [acc o (mu_a - mu_a^{n+1}) + d o (M^T mu_a)]
// -- block triangular: the mu blocks, then lambda.  In reverse flow order row i is k + 1 divisions once the cells
// downstream of it are known: with o = A_ii + sink_i and u_a = sum_{lev[j] > lev[i]} valT[e] mu_aj
//     mu_ai = (rmu_ai - phi_i u_a) / (acc_i s_i + ads_ai + phi_i o),      (M^T mu_a)_i = u_a + o mu_ai
// so the coupling term of lambda's right-hand side is known inside the row, and lambda_i is the division of
// sweep_row_nl_t on rl_i minus that term.  One thread per row, the load chain of sweep_row_nlc: the components four
// accumulators at a time with the entries in groups of kNlcGroup, the sums in stored order; a slot past the row's end
// repeats the last entry, a slot that is not downstream reads the row's own right-hand side (an address that is valid
// and that no thread writes here) and enters as + 0; in the last chunk an accumulator beyond k takes component a0 again
// and its coupling term is selected away, so nothing branches on k; all loads of a chunk come before its first store.
// The first chunk's groups carry lambda's downstream sum beside the four of mu (the indices, levels and values are
// loaded once for both); the coupling sum is carried across the chunks; lambda's division comes last.
//   core   rows of the core level take their in-core neighbours of both mu and lambda from the previous iterate:
//          Jacobi on a block-triangular system, which converges at the rate of its diagonal blocks -- those of the
//          forward components' step and of sweep_row_nl_t_core.
struct NlCompT {
  int k = 0;
  const double* ads = nullptr;       // [n k] sorption capacity (may be nullptr)
  const double* r = nullptr;         // [n k] the right-hand side of mu
  const double* mu_next = nullptr;   // [n k] mu^{n+1} (zeros in the first step)
  const double* c = nullptr;         // [n k] c^n
  const double* mu_prev = nullptr;   // [n k] the core's previous iterate of mu ...
  const double* lam_prev = nullptr;  // [n]   ... and of lambda
  double* mu = nullptr;
};
struct NlcTSums {
  double u0, u1, u2, u3, sl;
};

// the sums of the chunk a0 .. a0 + 3 over the row's entries; WithLam: lambda's sum beside them
template <bool Core, bool WithLam>
PFV_FN NlcTSums sweep_nlc_t_sums(int32_t i, int32_t li, int e_begin, int e_end, const int32_t* ix, const double* valT,
                                 const int32_t* lev, int k, int a0, int o1, int o2, int o3, const double* mu,
                                 const double* mu_prev, const double* own, const double* lam, const double* lam_prev,
                                 const double* own_l) {
  NlcTSums S{0.0, 0.0, 0.0, 0.0, 0.0};
  for (int e0 = e_begin; e0 < e_end; e0 += kNlcGroup) {
    int32_t j[kNlcGroup];
    double v[kNlcGroup];
    const double* up[kNlcGroup];
    const double* upl[kNlcGroup];
#pragma unroll
    for (int t = 0; t < kNlcGroup; ++t) {
      const int e = e0 + t < e_end ? e0 + t : e_end - 1;
      j[t] = ix[e];
      v[t] = valT[e];
    }
#pragma unroll
    for (int t = 0; t < kNlcGroup; ++t) {
      const int32_t lj = lev[j[t]];
      const bool down = lj > li, in_core = Core && lj == li && j[t] != i;
      const bool live = (down || in_core) && e0 + t < e_end;
      up[t] = live ? (down ? mu : mu_prev) + (int64_t)j[t] * k + a0 : nullptr;
      if (WithLam) upl[t] = live ? (down ? lam : lam_prev) + j[t] : nullptr;
    }
#pragma unroll
    for (int t = 0; t < kNlcGroup; ++t) {
      const double* r = up[t] ? up[t] : own;
      const double w0 = r[0], w1 = r[o1], w2 = r[o2], w3 = r[o3];
      const double vt = up[t] ? v[t] : 0.0;
      S.u0 += vt * (up[t] ? w0 : 0.0);
      S.u1 += vt * (up[t] ? w1 : 0.0);
      S.u2 += vt * (up[t] ? w2 : 0.0);
      S.u3 += vt * (up[t] ? w3 : 0.0);
      if (WithLam) {
        const double wl = *(upl[t] ? upl[t] : own_l);
        S.sl += vt * (upl[t] ? wl : 0.0);
      }
    }
  }
  return S;
}

// the four divisions of the chunk and its part of lambda's coupling term (m = k - a0 components are the chunk's own)
PFV_FN double sweep_nlc_t_divide(const NlCompT& C, int64_t p0, int o1, int o2, int o3, int m, double as, double op,
                                 double ph, double o, double ac, double di, const NlcTSums& S) {
  const int64_t p1 = p0 + o1, p2 = p0 + o2, p3 = p0 + o3;
  const double r0 = C.r[p0], r1 = C.r[p1], r2 = C.r[p2], r3 = C.r[p3];
  const double g0 = C.ads ? C.ads[p0] : 0.0, g1 = C.ads ? C.ads[p1] : 0.0;
  const double g2 = C.ads ? C.ads[p2] : 0.0, g3 = C.ads ? C.ads[p3] : 0.0;
  const double n0 = C.mu_next[p0], n1 = C.mu_next[p1], n2 = C.mu_next[p2], n3 = C.mu_next[p3];
  const double c0 = C.c[p0], c1 = C.c[p1], c2 = C.c[p2], c3 = C.c[p3];
  const double x0 = (r0 - ph * S.u0) / (as + g0 + op), x1 = (r1 - ph * S.u1) / (as + g1 + op);
  const double x2 = (r2 - ph * S.u2) / (as + g2 + op), x3 = (r3 - ph * S.u3) / (as + g3 + op);
  C.mu[p0] = x0;  // (the loads of all four before the first store: a store could alias them for the compiler)
  C.mu[p1] = x1;
  C.mu[p2] = x2;
  C.mu[p3] = x3;
  const double t0 = c0 * (ac * (x0 - n0) + di * (S.u0 + o * x0)), t1 = c1 * (ac * (x1 - n1) + di * (S.u1 + o * x1));
  const double t2 = c2 * (ac * (x2 - n2) + di * (S.u2 + o * x2)), t3 = c3 * (ac * (x3 - n3) + di * (S.u3 + o * x3));
  double sum = t0;
  sum += m > 1 ? t1 : 0.0;
  sum += m > 2 ? t2 : 0.0;
  sum += m > 3 ? t3 : 0.0;
  return sum;
}

template <bool Core>
PFV_FN void sweep_row_nlc_t_rule(int32_t i, const int32_t* ip, const int32_t* ix, const double* valT, const double* diag,
                                 const double* sink, const double* acc, const double* d, const double* phi,
                                 const double* s, const int32_t* lev, const double* rl, double* lam, const NlCompT& C) {
  const int k = C.k;
  const int32_t li = lev[i];
  const double ph = phi[i], di = d[i], ac = acc[i], o = diag[i] + (sink ? sink[i] : 0.0);
  const double as = ac * s[i], op = o * ph;
  const int64_t p = (int64_t)i * k;
  const int e_begin = ip[i], e_end = ip[i + 1];
  const double ri = rl[i];
  int o1 = k > 1 ? 1 : 0, o2 = k > 2 ? 2 : 0, o3 = k > 3 ? 3 : 0;
  const NlcTSums S0 = sweep_nlc_t_sums<Core, true>(i, li, e_begin, e_end, ix, valT, lev, k, 0, o1, o2, o3, C.mu, C.mu_prev,
                                                   C.r + p, lam, C.lam_prev, rl + i);
  double cpl = sweep_nlc_t_divide(C, p, o1, o2, o3, k, as, op, ph, o, ac, di, S0);
  for (int a0 = 4; a0 < k; a0 += 4) {
    const int m = k - a0;
    o1 = m > 1 ? 1 : 0, o2 = m > 2 ? 2 : 0, o3 = m > 3 ? 3 : 0;
    const NlcTSums S = sweep_nlc_t_sums<Core, false>(i, li, e_begin, e_end, ix, valT, lev, k, a0, o1, o2, o3, C.mu,
                                                     C.mu_prev, C.r + p + a0, nullptr, nullptr, nullptr);
    cpl += sweep_nlc_t_divide(C, p + a0, o1, o2, o3, m, as, op, ph, o, ac, di, S);
  }
  lam[i] = ((ri - cpl) - di * S0.sl) / (ac + di * o);
}

PFV_FN void sweep_row_nlc_t(int32_t i, const int32_t* ip, const int32_t* ix, const double* valT, const double* diag,
                            const double* sink, const double* acc, const double* d, const double* phi, const double* s,
                            const int32_t* lev, const double* rl, double* lam, const NlCompT& C) {
  sweep_row_nlc_t_rule<false>(i, ip, ix, valT, diag, sink, acc, d, phi, s, lev, rl, lam, C);
}

// ... of the core level: C.mu_prev and C.lam_prev hold the previous iterate
PFV_FN void sweep_row_nlc_t_core(int32_t i, const int32_t* ip, const int32_t* ix, const double* valT, const double* diag,
                                 const double* sink, const double* acc, const double* d, const double* phi,
                                 const double* s, const int32_t* lev, const double* rl, double* lam, const NlCompT& C) {
  sweep_row_nlc_t_rule<true>(i, ip, ix, valT, diag, sink, acc, d, phi, s, lev, rl, lam, C);
}

// the launch plan's levels in [from, to), from last to first.  Returns the launches.
static int sweep_apply_nlc_t(pfv_ctx_impl& c, const Sweep& sw, int from, int to, const CsrPattern& P, const double* valT,
                             const double* diag, const double* sink, const double* acc, const double* d,
                             const double* phi, const double* s, const double* rl, double* lam, const NlCompT& C) {
  const int32_t* ip = P.indptr;
  const int32_t* ix = P.indices;
  const int32_t* lev = sw.lev(false);
  return sweep_plan_range(sw, from, to, [&](int l0, int l1) {
    sweep_levels(c, sw, false, l0, l1, OnePerRow{}, PFV_LAMBDA(int32_t i, int) {
      sweep_row_nlc_t(i, ip, ix, valT, diag, sink, acc, d, phi, s, lev, rl, lam, C);
    }, Descending{});
  }, Descending{});
}

// one Jacobi iteration of the core level on its transposed rows
static void sweep_core_nlc_t(pfv_ctx_impl& c, const Sweep& sw, const CsrPattern& P, const double* valT,
                             const double* diag, const double* sink, const double* acc, const double* d,
                             const double* phi, const double* s, const double* rl, double* lam, const NlCompT& C) {
  const int32_t* ip = P.indptr;
  const int32_t* ix = P.indices;
  const int32_t* lev = sw.lev(false);
  sweep_core_rows(c, sw, OnePerRow{}, PFV_LAMBDA(int32_t i, int, int64_t) {
    sweep_row_nlc_t_core(i, ip, ix, valT, diag, sink, acc, d, phi, s, lev, rl, lam, C);
  });
}

// The streaming pass over the step's slab: phi = f(s^n), d = f'(s^n), and the dry rows -- a divisor acc_i s_i + ads_ia +
// phi_i (A_ii + sink_i) of a component that is zero (the forward step keeps c there and does not determine it): the
// lowest i k + a in *dry, by the integer atomic minimum of sweep_nl_check_inputs (preset to 0x7f7f7f7f).
static void adjoint_nlc_slopes(pfv_ctx_impl& c, const FluxFn& F, int k, const double* s, const double* diag,
                               const double* sink, const double* acc, const double* ads, double* d, double* phi,
                               int32_t* dry) {
  parallel_for(c.stream, c.nc, PFV_LAMBDA(int64_t i) {
    double df;
    const double ph = fluxfn_eval(F, s[i], &df);
    phi[i] = ph;
    d[i] = df;
    const double as = acc[i] * s[i], op = (diag[i] + (sink ? sink[i] : 0.0)) * ph;
    for (int a = 0; a < k; ++a)
      if (as + (ads ? ads[i * k + a] : 0.0) + op == 0.0) atomic_min_i32(dry, (int32_t)(i * k + a));
  });
}

// The right-hand sides of adjoint step n, rmu_a = c_loads_a^n + (acc o s^n + ads_a) o mu_a^{n+1} and rl = s_loads^n +
// acc o lambda^{n+1}, fused with what the multipliers of step n + 1 add to the gradients that live on the cells:
//     grad_source += lambda^{n+1},   grad_c_source_a += mu_a^{n+1},   grad_sorption_a -= mu_a^{n+1} o (c_a^{n+1} - c_a^n),
//     grad_accumulation -= lambda^{n+1} o (s^{n+1} - s^n) + sum_a mu_a^{n+1} o (s^{n+1} o c_a^{n+1} - s^n o c_a^n).
// Work item (row, a); a == k is the saturation's.  lam == nullptr (the first step): the loads alone.  closing (after the
// last step, no loads, slab 0 in s_n / c_n): rmu_a = (acc o s^0 + ads_a) o mu_a^1 = grad_c0 and rl = acc o lambda^1 +
// sum_a acc o c_a^0 o mu_a^1 = grad_s0.  s_loads is [n_obs], c_loads [k][n_obs] (either may be nullptr: zeros); slot as
// in adjoint_step_rhs.  Interleaved vectors.
static void adjoint_nlc_step_rhs(pfv_ctx_impl& c, int k, const double* acc, const double* ads, const double* s_n,
                                 const double* c_n, const double* s_np1, const double* c_np1, const double* lam,
                                 const double* mu, const int32_t* slot, const double* s_loads, const double* c_loads,
                                 int64_t n_obs, bool closing, double* gsrc, double* gcsrc, double* gacc, double* gads,
                                 double* rl, double* rmu) {
  parallel_for(c.stream, c.nc * (k + 1), PFV_LAMBDA(int64_t w) {
    const int64_t i = w / (k + 1);
    const int a = (int)(w % (k + 1));
    const int64_t m = (s_loads || c_loads) ? (slot ? (int64_t)slot[i] : i) : -1;
    if (a < k) {
      const int64_t t = i * k + a;
      const double g = c_loads && m >= 0 ? c_loads[a * n_obs + m] : 0.0;
      double v = g;
      if (lam) {
        const double x = mu[t];
        v = g + (acc[i] * s_n[i] + (ads ? ads[t] : 0.0)) * x;
        if (gcsrc) gcsrc[t] += x;
        if (gads) gads[t] -= x * (c_np1[t] - c_n[t]);
      }
      rmu[t] = v;
    } else {
      const double g = s_loads && m >= 0 ? s_loads[m] : 0.0;
      double v = g;
      if (lam) {
        const double l = lam[i];
        v = g + acc[i] * l;
        if (gsrc) gsrc[i] += l;
        if (gacc || closing) {
          const double s0 = s_n[i], s1 = s_np1[i];
          double da = 0.0, cm = 0.0;
          for (int b = 0; b < k; ++b) {
            const int64_t t = i * k + b;
            const double x = mu[t];
            da += x * (s1 * c_np1[t] - s0 * c_n[t]);
            cm += c_n[t] * x;
          }
          if (gacc) gacc[i] -= l * (s1 - s0) + da;
          if (closing) v += acc[i] * cm;
        }
      }
      rl[i] = v;
    }
  });
}

// (M^T mu_a)_i = sum_e valT[e] mu_aj + sink_i mu_ai in stored order; from >= 0: the entries of the levels from `from` on alone
PFV_FN double sweep_nlc_t_row_image(int64_t i, int a, int k, const int32_t* ip, const int32_t* ix, const double* valT,
                                    const double* sink, const double* mu, const int32_t* lev, int32_t from) {
  double t = 0.0;
  for (int e = ip[i]; e < ip[i + 1]; ++e) {
    const int32_t j = ix[e];
    if (from < 0 || lev[j] >= from) t += valT[e] * mu[(int64_t)j * k + a];
  }
  if (sink) t += sink[i] * mu[i * k + a];
  return t;
}

// the coupling term of lambda's right-hand side from the image of mu: sum_a c_ai [acc_i (mu_ai - mu+_ai) + d_i (M^T mu_a)_i]
PFV_FN double sweep_nlc_t_coupling(int64_t i, int k, const int32_t* ip, const int32_t* ix, const double* valT,
                                   const double* sink, const double* acc, const double* d, const NlCompT& C,
                                   const int32_t* lev, int32_t from) {
  double cpl = 0.0;
  for (int b = 0; b < k; ++b) {
    const int64_t p = i * k + b;
    const double img = sweep_nlc_t_row_image(i, b, k, ip, ix, valT, sink, C.mu, lev, from);
    cpl += C.c[p] * (acc[i] * (C.mu[p] - C.mu_next[p]) + d[i] * img);
  }
  return cpl;
}

// The acceptance check, k + 1 pairs in one kernel: out[a] = (rmu_a, rmu_a) and out[k + 1 + a] the squared residual of
// mu_a's system; out[k] and out[2 k + 1] the same for lambda, whose right-hand side rl - coupling is RECOMPUTED from the
// image of the final mu (not taken from what the row used: a wrong coupling in the row shows as a residual).
// core_only (the core's stop test): the residuals of the core rows alone, the images taken from the entries of the
// row's own level and above; lambda's scale takes the coupling on the rows from the core level on (the levels below
// have no mu yet) and rl alone below.
static void sweep_norms_nlc_t(pfv_ctx_impl& c, const Sweep& sw, const CsrPattern& P, const double* valT,
                              const double* sink, const double* acc, const double* d, const double* phi,
                              const double* s, const double* rl, const double* lam, const NlCompT& C, bool core_only,
                              double* out) {
  const int32_t* ip = P.indptr;
  const int32_t* ix = P.indices;
  const int32_t* lev = sw.lev(false);
  const int32_t core = core_only ? sw.core_level : -1;
  const int k = C.k;
  sweep_norms_pairs(c, P.nrows, k + 1, out, PFV_LAMBDA(int64_t i, int a) {
    const bool judged = core < 0 || lev[i] == core;
    if (a < k) {
      const int64_t p = i * k + a;
      const double ri = C.r[p];
      if (!judged) return NormPair{ri, 0.0};
      const double img = sweep_nlc_t_row_image(i, a, k, ip, ix, valT, sink, C.mu, lev, core);
      const double t = (acc[i] * s[i] + (C.ads ? C.ads[p] : 0.0)) * C.mu[p] + phi[i] * img;
      return NormPair{ri, ri - t};
    }
    if (core >= 0 && lev[i] < core) return NormPair{rl[i], 0.0};
    const double ri = rl[i] - sweep_nlc_t_coupling(i, k, ip, ix, valT, sink, acc, d, C, lev, core);
    if (!judged) return NormPair{ri, 0.0};
    const double t = acc[i] * lam[i] + d[i] * sweep_nl_t_row_image(i, ip, ix, valT, sink, lam, lev, core);
    return NormPair{ri, ri - t};
  });
}

// grad_sink[i] -= phi_i (lambda_i + sum_a mu_ai c_ai): the sink takes the phase at f(s) and the components with it
static void adjoint_nlc_grad_sink(pfv_ctx_impl& c, int k, const double* lam, const double* mu, const double* c_n,
                                  const double* phi, double* gsink) {
  parallel_for(c.stream, c.nc, PFV_LAMBDA(int64_t i) {
    double sum = 0.0;
    for (int a = 0; a < k; ++a) sum += mu[i * k + a] * c_n[i * k + a];
    gsink[i] -= (lam[i] + sum) * phi[i];
  });
}

// lambda[p] - lambda[m] of face f (a missing cell contributes nothing); stride k, offset a for an interleaved vector
PFV_FN double adjoint_face_jump(int64_t f, int64_t nf, const int32_t* side, const double* x, int k, int a) {
  const int32_t cp = side[f], cm = side[nf + f];
  double dx = 0.0;
  if (cp >= 0) dx = x[(int64_t)cp * k + a];
  if (cm >= 0) dx -= x[(int64_t)cm * k + a];
  return dx;
}

// grad_bc_values[f] (the saturation's boundary value): a Neumann face as adjoint_nl_grad_bc, from lambda alone; a
// Dirichlet inflow face  -= q_f f'(bc_f) [(lambda[p] - lambda[m]) + sum_a (mu_a[p] - mu_a[m]) cbc_af].  cbc is
// component-major [k][nf].
static void adjoint_nlc_grad_bc(pfv_ctx_impl& c, const FluxFn& F, int k, const double* d_q, const double* bc,
                                const double* cbc, const double* lam, const double* mu, double* gbc) {
  const int64_t nf = c.nf;
  const uint8_t* cls = c.upw_cls;
  const int32_t* cnt = c.upw_cnt;
  const int32_t* side = c.upw_side;
  parallel_for(c.stream, nf, PFV_LAMBDA(int64_t f) {
    const unsigned cl = cls[f];
    if (!(cl & (UPW_NEU | UPW_DIRIN))) return;
    double m = 0.0, md = 0.0;
    if (cl & UPW_NEU) m = (double)(cnt[f] - cnt[nf + f]);
    if (cl & UPW_DIRIN) {
      double df;
      fluxfn_eval(F, bc[f], &df);
      md = df * d_q[f];
      m += md;
    }
    const int32_t cp = side[f], cm = side[nf + f];
    double s = 0.0;
    if (cp >= 0) s += m * lam[cp];
    if (cm >= 0) s -= m * lam[cm];
    if (cl & UPW_DIRIN) {
      double dm = 0.0;
      for (int a = 0; a < k; ++a) dm += adjoint_face_jump(f, nf, side, mu, k, a) * cbc[a * nf + f];
      s += md * dm;
    }
    gbc[f] -= s;
  });
}

// grad_c_bc_values[a][f] -= m_f (mu_a[p] - mu_a[m]), m_f the derivative of the entry of rhs_neu cbc_a + rhs_dir diag(q)
// (f(bc) o cbc_a) in row f (upwind_bref_nlc) with respect to cbc_af: the Neumann count, q_f f(bc_f) on a Dirichlet inflow
// face.  One work item per (face, component); gcbc is component-major [k][nf].
static void adjoint_nlc_grad_cbc(pfv_ctx_impl& c, const FluxFn& F, int k, const double* d_q, const double* bc,
                                 const double* mu, double* gcbc) {
  const int64_t nf = c.nf;
  const uint8_t* cls = c.upw_cls;
  const int32_t* cnt = c.upw_cnt;
  const int32_t* side = c.upw_side;
  parallel_for(c.stream, nf * k, PFV_LAMBDA(int64_t t) {
    const int64_t f = t / k, a = t % k;
    const unsigned cl = cls[f];
    if (!(cl & (UPW_NEU | UPW_DIRIN))) return;
    double m = 0.0, df;
    if (cl & UPW_NEU) m = (double)(cnt[f] - cnt[nf + f]);
    if (cl & UPW_DIRIN) m += d_q[f] * fluxfn_eval(F, bc[f], &df);
    const int32_t cp = side[f], cm = side[nf + f];
    double s = 0.0;
    if (cp >= 0) s += m * mu[(int64_t)cp * k + a];
    if (cm >= 0) s -= m * mu[(int64_t)cm * k + a];
    gcbc[a * nf + f] -= s;
  });
}

// grad_flux[f] -= (lambda[p] - lambda[m]) phiup_f + sum_a (mu_a[p] - mu_a[m]) phiup_f cup_af: phiup as in
// adjoint_nl_grad_flux, cup the concentration the phase carries through f -- the upstream cell's c^n (interior and
// outflow faces), cbc on a Dirichlet inflow face; a Neumann face gives 0.  The upstream side is fixed.
static void adjoint_nlc_grad_flux(pfv_ctx_impl& c, const FluxFn& F, int k, const double* bc, const double* cbc,
                                  const double* lam, const double* mu, const double* phi, const double* c_n,
                                  double* gq) {
  const int64_t nf = c.nf;
  const uint8_t* cls = c.upw_cls;
  const int32_t* up = c.upw_up;
  const int32_t* side = c.upw_side;
  parallel_for(c.stream, nf, PFV_LAMBDA(int64_t f) {
    const unsigned cl = cls[f];
    if (!(cl & (UPW_KEPT | UPW_DIRIN))) return;
    const int32_t u = up[f];
    double df;
    const double pu = (cl & UPW_KEPT) ? phi[u] : fluxfn_eval(F, bc[f], &df);
    double s = adjoint_face_jump(f, nf, side, lam, 1, 0) * pu;
    for (int a = 0; a < k; ++a) {
      const double cup = (cl & UPW_KEPT) ? c_n[(int64_t)u * k + a] : cbc[a * nf + f];
      s += adjoint_face_jump(f, nf, side, mu, k, a) * (pu * cup);
    }
    gq[f] -= s;
  });
}

// The six Corey sums by the scheme of adjoint_nl_grad_fluxfn with the components' terms in both weights: cell i weighs
// (M^T lambda)_i + sum_a c_ai (M^T mu_a)_i, the Dirichlet inflow face f  q_f [(lambda[p] - lambda[m]) + sum_a (mu_a[p] -
// mu_a[m]) cbc_af].
static void adjoint_nlc_grad_fluxfn(pfv_ctx_impl& c, const FluxFn& F, const CsrPattern& P, const double* valT,
                                    const double* sink, int k, const double* d_q, const double* bc, const double* cbc,
                                    const double* lam, const double* mu, const double* s_n, const double* c_n,
                                    double* gF) {
  const int64_t nf = c.nf;
  const int32_t* ip = P.indptr;
  const int32_t* ix = P.indices;
  const int32_t* side = c.upw_side;
  adjoint_nl_grad_fluxfn_weighted(c, F, bc, s_n, gF, PFV_LAMBDA(int64_t t) {
    double wt = sweep_nl_t_row_image(t, ip, ix, valT, sink, lam, nullptr, -1);
    for (int a = 0; a < k; ++a)
      wt += c_n[t * k + a] * sweep_nlc_t_row_image(t, a, k, ip, ix, valT, sink, mu, nullptr, -1);
    return wt;
  }, PFV_LAMBDA(int64_t f) {
    double dl = adjoint_face_jump(f, nf, side, lam, 1, 0);
    for (int a = 0; a < k; ++a) dl += adjoint_face_jump(f, nf, side, mu, k, a) * cbc[a * nf + f];
    return dl * d_q[f];
  });
}

// The direct solve of the transport system of an acyclic flux: x = M^-1 b with M = S, then the true residual.  Should
// the check fail (a flux array in the assembly that disagrees with the discretization's, NaN entries), GMRES
// preconditioned by the sweep goes on from that x.
static SolveResult sweep_direct_solve(pfv_ctx_impl& c, const LinSys& sys, const Precond& M, double rtol, int maxit,
                                      int restart, double* d_x, bool& fell_back) {
  stream_t s = c.stream;
  const int64_t n = sys.n;
  SolveResult res;
  fell_back = false;
  precond_apply(c, M, n, sys.rhs, d_x);
  double* t = c.kry[6].ensure(n);
  double* nrm = c.kry[7].ensure(2);
  sys_spmv(c, sys, d_x, t);
  sweep_residual_norms(c, n, sys.rhs, t, nrm);
  double h[2];
  be_d2h(h, nrm, sizeof(h), s);
  res.iterations = 1;
  if (!(h[0] > 0.0)) {  // b = 0 -> x = 0 (what the sweep has left)
    res.converged = h[0] == 0.0;
    return res;
  }
  res.relres = std::sqrt(h[1] / h[0]);
  res.converged = h[1] <= rtol * rtol * h[0];
  if (res.converged) return res;
  fell_back = true;
  SolveResult g = gmres_solve(c, sys, rtol, maxit, restart, d_x, false, &M);
  g.iterations += 1;
  return g;
}

}  // namespace pfv
