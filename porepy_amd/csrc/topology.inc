// topology.inc — device construction of the sub-cell topology and the CSR patterns.
//
// Replaces SubcellTopology.__init__ (numerics/fv/_fvutils.py:51-172: rldecode + two
// sparse products + a 4-key lexsort + two np.unique) by one stable radix sort of the
// (cell, face, node) triples on the node id, and replaces the value-dependent patterns
// that fall out of the reference's SpGEMM chain by the structural stencil
// {cells / boundary faces sharing a node with the face}.  Everything here is integer,
// HBM-bound work: thread-per-element kernels with coalesced reads of the CSC arrays.

namespace pfv {

// The reference construction (PFV_TOPO_LEGACY=1, and the path that reports what build_topology_nodes cannot represent):
// one global sort of the (node, entry) pairs.
static void build_topology_legacy(pfv_ctx_impl& c) {
  stream_t s = c.stream;
  const int nd = c.nd;
  const int64_t nc = c.nc, nf = c.nf, nn = c.nn, ncf = c.ncf, nsf = c.nsf;
  const int32_t* cf_ptr = c.cf_ptr;
  const int32_t* cf_idx = c.cf_idx;
  const int8_t* cf_sgn = c.cf_sgn;
  const int32_t* fn_ptr = c.fn_ptr;
  const int32_t* fn_idx = c.fn_idx;

  int bits = 1;
  while ((int64_t(1) << bits) < nn + 1 && bits < 32) ++bits;

  // --- cell of every cell_faces entry, #nodes of its face -> offsets of its triples
  Buf<int32_t> cell_of_e, cnt_e;
  Buf<int64_t> h_off;
  cell_of_e.ensure(ncf);
  cnt_e.ensure(ncf + 1);
  h_off.ensure(ncf + 1);
  {
    int32_t* coe = cell_of_e;
    parallel_for(s, nc, PFV_LAMBDA(int64_t cell) {
      for (int e = cf_ptr[cell]; e < cf_ptr[cell + 1]; ++e) coe[e] = (int32_t)cell;
    });
    int32_t* cnt = cnt_e;
    parallel_for(s, ncf, PFV_LAMBDA(int64_t e) {
      const int f = cf_idx[e];
      cnt[e] = fn_ptr[f + 1] - fn_ptr[f];
    });
  }
  exclusive_scan<int32_t, int64_t>(s, c.scratch, cnt_e.p, h_off.p, (size_t)ncf);
  const int64_t nh = read_scalar<int64_t>(s, h_off.p + ncf);
  if (nh >= (int64_t(1) << 31)) throw Error(5, "more than 2^31 sub-half-faces on one device");
  c.nh = nh;

  // --- (node, entry) pairs in (cell, face, node-of-face) order, stable sort by node
  Buf<uint32_t> key_in, key_out;
  Buf<int32_t> val_in, val_out;
  key_in.ensure(std::max(nh, nsf));
  key_out.ensure(std::max(nh, nsf));
  val_in.ensure(std::max(nh, nsf));
  val_out.ensure(std::max(nh, nsf));
  {
    uint32_t* k = key_in;
    int32_t* v = val_in;
    const int64_t* off = h_off;
    parallel_for(s, ncf, PFV_LAMBDA(int64_t e) {
      const int f = cf_idx[e];
      const int64_t o = off[e];
      const int a = fn_ptr[f], n = fn_ptr[f + 1] - a;
      for (int i = 0; i < n; ++i) {
        k[o + i] = (uint32_t)fn_idx[a + i];
        v[o + i] = (int32_t)e;
      }
    });
  }
  sort_pairs(s, c.scratch, key_in.p, key_out.p, val_in.p, val_out.p, (size_t)nh, bits);

  c.node_hptr.ensure(nn + 1);
  c.h_cell.ensure(nh);
  c.h_lf.ensure(nh);
  c.h_sgn.ensure(nh);
  c.h_first.ensure(nh);
  Buf<int32_t> h_face;
  h_face.ensure(nh);
  {
    int32_t* hp = c.node_hptr;
    const uint32_t* ks = key_out;
    parallel_for(s, nn + 1, PFV_LAMBDA(int64_t v) {
      hp[v] = lower_bound_idx<uint32_t>(ks, (int)nh, (uint32_t)v);
    });
    int32_t* hc = c.h_cell;
    int32_t* hf = h_face;
    int8_t* hs = c.h_sgn;
    const int32_t* ev = val_out;
    const int32_t* coe = cell_of_e;
    parallel_for(s, nh, PFV_LAMBDA(int64_t h) {
      const int e = ev[h];
      hc[h] = coe[e];
      hf[h] = cf_idx[e];
      hs[h] = cf_sgn[e];
    });
  }
  // keep the sorted node id of every h for the next kernels
  Buf<uint32_t> h_node;
  h_node.ensure(nh);
  be_d2d(h_node.p, key_out.p, sizeof(uint32_t) * nh, s);

  // --- subfaces (face, node) grouped by node: second stable sort, on face_nodes itself
  c.node_fptr.ensure(nn + 1);
  c.node_sf.ensure(nsf);
  c.sf_face.ensure(nsf);
  c.sf_ls.ensure(nsf);
  {
    uint32_t* k = key_in;
    int32_t* v = val_in;
    parallel_for(s, nsf, PFV_LAMBDA(int64_t i) {
      k[i] = (uint32_t)fn_idx[i];
      v[i] = (int32_t)i;
    });
    int32_t* sff = c.sf_face;
    parallel_for(s, nf, PFV_LAMBDA(int64_t f) {
      for (int i = fn_ptr[f]; i < fn_ptr[f + 1]; ++i) sff[i] = (int32_t)f;
    });
  }
  sort_pairs(s, c.scratch, key_in.p, key_out.p, val_in.p, c.node_sf.p, (size_t)nsf, bits);
  {
    Buf<int32_t> mx;
    mx.ensure(2);
    be_memset(mx.p, 0, 2 * sizeof(int32_t), s);
    int32_t* m = mx;
    // (two maxima, one read: every host read is a stream synchronisation)
    parallel_for(s, nf, PFV_LAMBDA(int64_t f) { track_max_i32(m, fn_ptr[f + 1] - fn_ptr[f]); });
    parallel_for(s, nc, PFV_LAMBDA(int64_t cell) { track_max_i32(m + 1, cf_ptr[cell + 1] - cf_ptr[cell]); });
    int32_t mxh[2];
    be_d2h(mxh, mx.p, sizeof(mxh), s);
    c.max_face_nodes = mxh[0];
    if (c.max_face_nodes > kMaxFaceNodes)
      throw Error(PFV_ERR_UNSUPPORTED, "faces with more than 8 nodes are not supported");
    c.max_cell_faces = mxh[1];
    if (c.max_cell_faces > kMaxCellFaces)
      throw Error(PFV_ERR_UNSUPPORTED, "cells with more than 16 faces are not supported");
  }
  c.status.ensure(16);
  be_memset(c.status.p, 0, sizeof(int32_t) * 16, s);
  {
    int32_t* fp = c.node_fptr;
    const uint32_t* ks = key_out;
    parallel_for(s, nn + 1, PFV_LAMBDA(int64_t v) {
      fp[v] = lower_bound_idx<uint32_t>(ks, (int)nsf, (uint32_t)v);
    });
    const int32_t* nsf_sorted = c.node_sf;
    uint8_t* ls = c.sf_ls;
    int32_t* st = c.status;
    parallel_for(s, nsf, PFV_LAMBDA(int64_t pos) {
      const int v = (int)ks[pos];
      const int l = (int)pos - fp[v];
      if (l > kMaxBlock) atomic_max_i32(st + 1, l);
      ls[nsf_sorted[pos]] = (uint8_t)(l & 0xff);
    });
  }

  // --- faces: number of sides, lowest neighbouring cell (the side fluxes are taken from)
  c.face_nsides.ensure(nf);
  Buf<int32_t> face_first;
  face_first.ensure(nf);
  be_memset(c.face_nsides.p, 0, sizeof(int32_t) * nf, s);
  be_memset(face_first.p, 0x7f, sizeof(int32_t) * nf, s);
  {
    int32_t* ns = c.face_nsides;
    int32_t* ff = face_first;
    const int32_t* coe = cell_of_e;
    parallel_for(s, ncf, PFV_LAMBDA(int64_t e) {
      atomic_add_i32(ns + cf_idx[e], 1);
      atomic_min_i32(ff + cf_idx[e], coe[e]);
    });
  }

  // --- face id and boundary flag of every sub-face in node-major order: the per-node loops below read them from
  // consecutive addresses instead of chasing node_sf -> sf_face -> face_nsides per element
  Buf<uint8_t> nm_bnd_;
  int32_t* nm_face = c.node_face.ensure(nsf);  // (kept: the interaction-region kernel reads it too)
  uint8_t* nm_bnd = nm_bnd_.ensure(nsf);
  {
    const int32_t* nsfp = c.node_sf;
    const int32_t* sff = c.sf_face;
    const int32_t* ns = c.face_nsides;
    parallel_for(s, nsf, PFV_LAMBDA(int64_t pos) {
      const int f = sff[nsfp[pos]];
      nm_face[pos] = f;
      nm_bnd[pos] = ns[f] == 1 ? 1 : 0;
    });
  }

  // --- local face index of every h (binary search in the node's ascending face list)
  {
    const int32_t* fp = c.node_fptr;
    const int32_t* nsfp = c.node_sf;
    const int32_t* sff = c.sf_face;
    const int32_t* hf = h_face;
    const int32_t* hc = c.h_cell;
    const uint32_t* hn = h_node;
    const int32_t* ff = face_first;
    uint8_t* lf = c.h_lf;
    uint8_t* first = c.h_first;
    int32_t* st = c.status;
    parallel_for(s, nh, PFV_LAMBDA(int64_t h) {
      const int v = (int)hn[h];
      const int a = fp[v], n = fp[v + 1] - a;
      const int f = hf[h];
      int lo = 0, hi = n;
      while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (nm_face[a + mid] < f) lo = mid + 1; else hi = mid;
      }
      (void)nsfp; (void)sff;
      if (lo >= n || nm_face[a + lo] != f) atomic_max_i32(st + 0, 1);  // inconsistent grid
      lf[h] = (uint8_t)(lo & 0xff);
      first[h] = (hc[h] == ff[f]) ? 1 : 0;
    });
  }

  // --- per node: validate "nd faces of a cell meet in a node", sizes, boundary faces
  c.node_bptr.ensure(nn + 1);
  c.node_tptr.ensure(nn + 1);
  c.node_tbptr.ensure(nn + 1);
  Buf<int32_t> nb_cnt;
  Buf<int64_t> nsq, ntab, ntabb;
  Buf<double> nflop, nflop_scan;
  nb_cnt.ensure(nn + 1);
  nflop.ensure(nn + 1);
  nflop_scan.ensure(nn + 1);
  nsq.ensure(nn + 1);
  ntab.ensure(nn + 1);
  ntabb.ensure(nn + 1);
  {
    const int32_t* hp = c.node_hptr;
    const int32_t* fp = c.node_fptr;
    const int32_t* hc = c.h_cell;
    const int32_t* nsfp = c.node_sf;
    const int32_t* sff = c.sf_face;
    const int32_t* ns = c.face_nsides;
    int32_t* st = c.status;
    int32_t* nbc = nb_cnt;
    int64_t* sq = nsq;
    int64_t* tb = ntab;
    int64_t* tbb = ntabb;
    double* fl = nflop;
    parallel_for(s, nn, PFV_LAMBDA(int64_t v) {
      const int h0 = hp[v], cnt = hp[v + 1] - h0;
      bool ok = (cnt % nd) == 0;
      const int deg = cnt / nd;
      int prev = -1;
      for (int j = 0; ok && j < deg; ++j) {
        const int cc = hc[h0 + nd * j];
        for (int k = 1; k < nd; ++k) ok = ok && (hc[h0 + nd * j + k] == cc);
        ok = ok && (cc > prev);
        prev = cc;
      }
      if (!ok) atomic_max_i32(st + 0, 2);
      const int n = fp[v + 1] - fp[v];
      track_max_i32(st + 1, n);
      track_max_i32(st + 2, deg);
      sq[v] = (int64_t)n * n;
      int nb = 0;
      for (int l = 0; l < n; ++l) nb += nm_bnd[fp[v] + l];
      (void)nsfp; (void)sff; (void)ns;
      nbc[v] = nb;
      track_max_i32(st + 3, nb);
      // response table: n rows + the e-row, stride = nh rounded up to even (16-byte rows)
      tb[v] = (int64_t)(n + 1) * ((cnt + 1) & ~1);
      tbb[v] = 2 * (int64_t)n * nb;
      fl[v] = 2.0 * n * n * n + 2.0 * nd * n * cnt + 2.0 * (1 + nd) * n * nb + 60.0 * nd * nd * deg;
    });
  }
  int32_t st_host[4];
  be_d2h(st_host, c.status.p, sizeof(st_host), s);
  if (st_host[0] == 2)
    throw Error(PFV_ERR_CELL_SHAPE,
                "a cell does not have exactly nd faces meeting in one of its nodes (e.g. pyramid)");
  if (st_host[0] == 1) throw Error(PFV_ERR_ARGUMENT, "cell_faces / face_nodes are inconsistent");
  c.max_block = st_host[1];
  c.max_deg = st_host[2];
  c.max_bnd_per_node = st_host[3];
  if (c.max_block > kMaxBlock || c.max_deg > kMaxBlock)
    throw Error(PFV_ERR_UNSUPPORTED, "more than 255 faces or cells meet in one node");
  Buf<int64_t> sq_scan;
  sq_scan.ensure(nn + 1);
  exclusive_scan<int64_t, int64_t>(s, c.scratch, nsq.p, sq_scan.p, (size_t)nn);
  exclusive_scan<double, double>(s, c.scratch, nflop.p, nflop_scan.p, (size_t)nn);
  exclusive_scan<int64_t, int64_t>(s, c.scratch, ntab.p, c.node_tptr.p, (size_t)nn);
  exclusive_scan<int64_t, int64_t>(s, c.scratch, ntabb.p, c.node_tbptr.p, (size_t)nn);
  exclusive_scan<int32_t, int32_t>(s, c.scratch, nb_cnt.p, c.node_bptr.p, (size_t)nn);
  // the five totals in one packed read
  int32_t nb_total = 0;
  {
    Buf<double> tot;
    double* tp = tot.ensure(8);
    const int64_t* sqs = sq_scan;
    const double* fls = nflop_scan;
    const int64_t* tpt = c.node_tptr;
    const int64_t* tbp = c.node_tbptr;
    const int32_t* nbp = c.node_bptr;
    parallel_for(s, 1, PFV_LAMBDA(int64_t) {
      int64_t* ti = reinterpret_cast<int64_t*>(tp);
      ti[0] = sqs[nn];
      tp[1] = fls[nn];
      ti[2] = tpt[nn];
      ti[3] = tbp[nn];
      ti[4] = (int64_t)nbp[nn];
    });
    double th[5];
    be_d2h(th, tp, sizeof(th), s);
    const int64_t* thi = reinterpret_cast<const int64_t*>(th);
    c.sum_block_sq = thi[0];
    c.stats.node_flops = th[1];
    c.tab_len = thi[2];
    c.tabb_len = thi[3];
    nb_total = (int32_t)thi[4];
  }
  c.node_bfaces.ensure(nb_total);
  c.node_bls.ensure(nb_total);
  c.node_cells.ensure(nh / nd + 1);
  {
    const int32_t* fp = c.node_fptr;
    const int32_t* nsfp = c.node_sf;
    const int32_t* sff = c.sf_face;
    const int32_t* ns = c.face_nsides;
    const int32_t* bp = c.node_bptr;
    int32_t* bf = c.node_bfaces;
    uint8_t* bl = c.node_bls;
    parallel_for(s, nn, PFV_LAMBDA(int64_t v) {
      int o = bp[v];
      const int n = fp[v + 1] - fp[v];
      for (int l = 0; l < n; ++l) {
        if (nm_bnd[fp[v] + l]) {
          bf[o] = nm_face[fp[v] + l];
          bl[o] = (uint8_t)l;
          ++o;
        }
      }
      (void)nsfp; (void)sff; (void)ns;
    });
    const int32_t* hc = c.h_cell;
    int32_t* ncl = c.node_cells;
    parallel_for(s, nh / nd, PFV_LAMBDA(int64_t i) { ncl[i] = hc[(int64_t)nd * i]; });
  }

  // --- processing order of the face kernels: Morton curve through the face centres.  Faces that
  // share nodes then run close together in time, so the per-node coefficient tables they all read
  // stay in L2 (in face-id order the reuse distance on a 2 M-cell grid is ~1 GB and every face
  // re-fetched its 7 KB of tables from HBM: FETCH_SIZE 42 GB instead of ~9 GB).
  c.face_order.ensure(nf);
  {
    uint32_t* k = key_in.ensure(nf);
    int32_t* v = val_in.ensure(nf);
    key_out.ensure(nf);
    const double* fc = c.fcen;
    double lo[3], sc[3];
    for (int d = 0; d < 3; ++d) {
      lo[d] = c.bbox_lo[d];
      const double ext = c.bbox_hi[d] - c.bbox_lo[d];
      sc[d] = ext > 0 ? 1023.999 / ext : 0.0;
    }
    const double lo0 = lo[0], lo1 = lo[1], lo2 = lo[2], sc0 = sc[0], sc1 = sc[1], sc2 = sc[2];
    parallel_for(s, nf, PFV_LAMBDA(int64_t f) {
      uint32_t q[3];
      q[0] = (uint32_t)((fc[f] - lo0) * sc0);
      q[1] = (uint32_t)((fc[nf + f] - lo1) * sc1);
      q[2] = (uint32_t)((fc[2 * nf + f] - lo2) * sc2);
      uint32_t code = 0;
      for (int d = 0; d < 3; ++d) {
        uint32_t x = q[d] & 0x3ffu;  // spread 10 bits to every third position
        x = (x | (x << 16)) & 0x030000ffu;
        x = (x | (x << 8)) & 0x0300f00fu;
        x = (x | (x << 4)) & 0x030c30c3u;
        x = (x | (x << 2)) & 0x09249249u;
        code |= x << d;
      }
      k[f] = code;
      v[f] = (int32_t)f;
    });
    sort_pairs(s, c.scratch, key_in.p, key_out.p, val_in.p, c.face_order.p, (size_t)nf, 30);
  }

  // --- launch order of the interaction-region kernel: nodes bucketed by block size
  {
    const int nclass = kNumClasses;
    Buf<int32_t> bnd_dev;
    bnd_dev.ensure(nclass);
    be_h2d(bnd_dev.p, kClassBounds, sizeof(int) * nclass, s);
    uint32_t* k = key_in.ensure(nn);
    int32_t* v = val_in.ensure(nn);
    key_out.ensure(nn);
    c.node_order.ensure(nn);
    const int32_t* fp = c.node_fptr;
    const int32_t* bd = bnd_dev;
    parallel_for(s, nn, PFV_LAMBDA(int64_t node) {
      const int n = fp[node + 1] - fp[node];
      int cls = 0;
      while (cls < nclass - 1 && n > bd[cls]) ++cls;
      k[node] = (uint32_t)cls;
      v[node] = (int32_t)node;
    });
    sort_pairs(s, c.scratch, key_in.p, key_out.p, val_in.p, c.node_order.p, (size_t)nn, 4);
    // class boundaries: lower bounds in the sorted keys, searched on the device (nclass + 1 values come back, not the
    // nn keys)
    Buf<int32_t> cb_dev;
    int32_t* cbd = cb_dev.ensure(nclass + 1);
    const uint32_t* ks = key_out;
    parallel_for(s, nclass + 1, PFV_LAMBDA(int64_t cls) { cbd[cls] = lower_bound_idx<uint32_t>(ks, (int)nn, (uint32_t)cls); });
    std::vector<int32_t> cbh(nclass + 1);
    be_d2h(cbh.data(), cbd, sizeof(int32_t) * (nclass + 1), s);
    c.class_begin.assign(nclass + 1, nn);
    for (int cls = 0; cls <= nclass; ++cls) c.class_begin[cls] = cbh[cls];
  }
  c.have_topology = true;
  c.topo_key = 0;
  c.stats.num_nodes = nn;
  c.stats.num_sub_half_faces = nh;
  c.stats.sum_block_sq = c.sum_block_sq;
  c.stats.max_block = c.max_block;
  c.stats.node_table_doubles = c.tab_len + c.tabb_len;
}

// ------------------------------------------------------------------------------------
// Node-cooperative construction (the default).  The half-face records of a node are, in the stable order of the global
// sort above, simply its (face, side) pairs by ascending cell-face entry e -- at most 2 * 255 of them -- so every node
// orders its own records in LDS (rank = number of smaller keys) instead of 24 M pairs going through a radix sort, a
// gather, a copy and a binary search each.  Phases:
//   1  the sort keys of the sub-faces; then one pass over faces and cells: face of every sub-face, cell of every
//      cell-face entry, max nodes per face / faces per cell with one atomic per workgroup.  The (at most two) entries that
//      name a face are found WITHOUT atomics: every entry stores itself into slot[f] (any one of them stays), a second
//      pass stores every entry that is not slot[f] into other[f], a third flags an entry that is in neither (a third
//      side).  Which entry lands where depends on the order, the pair {slot, other} does not -- and only its minimum
//      and maximum are used.  (Three atomics per entry, 24 M of them, took 0.5 ms.)
//   2  sub-faces by node: the stable sort of the nsf (node, sub-face) pairs, as in the reference path
//   3  per node (16 lanes): face id and local index of its sub-faces, number of records and of boundary faces
//   4  ONE scan of the 6-field record (records, boundary faces, n^2, table sizes, flops) over the nodes
//   5  per node (one wavefront): keys = entries of its faces, ranked in LDS; cells of the records through LDS in
//      record order (validation, coalesced stores), their bytes straight to their rank; maxima, boundary-face lists,
//      cells around the node
//   6  face order and node order as in the reference path; everything the host needs comes back in ONE packed read.
// Buffers whose size the reference path reads back are sized by host-known bounds (nh <= 2 nsf, boundary faces <= nsf).
// What this construction cannot represent -- a face with more than two sides, more than 255 faces in a node, 2^31
// records -- raises a flag and returns false: the caller runs the reference path, which reports it.
struct TopoRec {
  int64_t h, nb, sq, tab, tabb;
  double fl;  // (a sum of integers below 2^53: exact in any order of summation)
};
PFV_HD inline TopoRec operator+(const TopoRec& a, const TopoRec& b) {
  return TopoRec{a.h + b.h, a.nb + b.nb, a.sq + b.sq, a.tab + b.tab, a.tabb + b.tabb, a.fl + b.fl};
}
struct alignas(16) TopoI4 {
  int32_t x, y, z, w;
};
struct TopoClassBounds {
  int b[kNumClasses];
};
constexpr int kTopoKeyCap = 512;           // key slots per node: 2 * kMaxBlock rounded up to a multiple of 4
constexpr int32_t kTopoNoKey = 0x7fffffff;  // key of an empty slot: never smaller than an entry

static bool build_topology_nodes(pfv_ctx_impl& c) {
  stream_t s = c.stream;
  const int nd = c.nd;
  const int64_t nc = c.nc, nf = c.nf, nn = c.nn, ncf = c.ncf, nsf = c.nsf;
  const int32_t* cf_ptr = c.cf_ptr;
  const int32_t* cf_idx = c.cf_idx;
  const int8_t* cf_sgn = c.cf_sgn;
  const int32_t* fn_ptr = c.fn_ptr;
  const int32_t* fn_idx = c.fn_idx;
  const int64_t hcap = 2 * nsf;  // bound on the number of records: a face has at most two sides
  if (hcap >= (int64_t(1) << 31)) return false;

  int bits = 1;
  while ((int64_t(1) << bits) < nn + 1 && bits < 32) ++bits;

  Buf<uint32_t> key_in, key_out;
  Buf<int32_t> val_in, val_out, cell_of_e, face_ends, cnt_n_, nb_n_;
  const int64_t nkey = std::max(nsf, std::max(nf, nn));
  key_in.ensure(nkey);
  key_out.ensure(nkey);
  val_in.ensure(nkey);
  int32_t* coe = cell_of_e.ensure(ncf);
  // [nf] slot, [nf] other: the one or two entries that name a face (-1: none)
  int32_t* fslot = face_ends.ensure(2 * nf);
  int32_t* fother = fslot + nf;
  Buf<int32_t> mx_;
  int32_t* mx = mx_.ensure(4);  // max nodes per face, max faces per cell, the "not representable" flag
  int32_t* ns = c.face_nsides.ensure(nf);
  int32_t* st = c.status.ensure(16);
  be_memset(fslot, 0xff, sizeof(int32_t) * 2 * nf, s);
  be_memset(mx, 0, sizeof(int32_t) * 4, s);
  be_memset(st, 0, sizeof(int32_t) * 16, s);

  c.node_fptr.ensure(nn + 1);
  c.node_sf.ensure(nsf);
  c.sf_face.ensure(nsf);
  c.sf_ls.ensure(nsf);
  // --- 1: faces and cells
  {
    uint32_t* k = key_in;
    int32_t* v = val_in;
    int32_t* sff = c.sf_face;
    parallel_for(s, nsf, PFV_LAMBDA(int64_t i) {
      k[i] = (uint32_t)fn_idx[i];
      v[i] = (int32_t)i;
    });
    // (the loads of a thread before its first store)
    parallel_for_max<2>(s, std::max(nc, nf), mx, PFV_LAMBDA(int64_t i, int32_t* m) {
      int fa = 0, fb = 0, ca = 0, cb = 0;
      if (i < nf) {
        fa = fn_ptr[i];
        fb = fn_ptr[i + 1];
      }
      if (i < nc) {
        ca = cf_ptr[i];
        cb = cf_ptr[i + 1];
      }
      int32_t f4[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) f4[u] = ca + u < cb ? cf_idx[ca + u] : -1;
      for (int t = fa; t < fb; ++t) sff[t] = (int32_t)i;
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        if (f4[u] >= 0) {
          coe[ca + u] = (int32_t)i;
          store_relaxed_i32(fslot + f4[u], ca + u);
        }
      }
      for (int e = ca + 4; e < cb; ++e) {
        const int f = cf_idx[e];
        coe[e] = (int32_t)i;
        store_relaxed_i32(fslot + f, e);
      }
      m[0] = fb - fa > m[0] ? fb - fa : m[0];
      m[1] = cb - ca > m[1] ? cb - ca : m[1];
    });
    parallel_for(s, ncf, PFV_LAMBDA(int64_t e) {
      const int f = cf_idx[e];
      if (fslot[f] != (int32_t)e) store_relaxed_i32(fother + f, (int32_t)e);
    });
    parallel_for(s, ncf, PFV_LAMBDA(int64_t e) {
      const int f = cf_idx[e];
      if (fslot[f] != (int32_t)e && fother[f] != (int32_t)e) atomic_max_i32(mx + 2, 1);
    });
  }
  // --- 2: sub-faces (face, node) grouped by node
  sort_pairs(s, c.scratch, key_in.p, key_out.p, val_in.p, c.node_sf.p, (size_t)nsf, bits);
  {
    int32_t* fp = c.node_fptr;
    const uint32_t* ks = key_out;
    parallel_for(s, nn + 1, PFV_LAMBDA(int64_t v) {
      fp[v] = lower_bound_idx<uint32_t>(ks, (int)nsf, (uint32_t)v);
    });
  }
  // --- 3: per node, face id and local index of every sub-face; records and boundary faces counted
  int32_t* nm_face = c.node_face.ensure(nsf);
  int32_t* cnt_n = cnt_n_.ensure(nn);
  int32_t* nb_n = nb_n_.ensure(nn);
  {
    const int32_t* fp = c.node_fptr;
    const int32_t* nsfp = c.node_sf;
    const int32_t* sff = c.sf_face;
    uint8_t* ls = c.sf_ls;
    wave_for<16>(s, nn, 2 * 16 * sizeof(int32_t), PFV_LAMBDA(const WaveCtx& w) {
      int32_t* part = reinterpret_cast<int32_t*>(w.lds);
      const int64_t v = w.item;
      const int a = fp[v], n = fp[v + 1] - a;
      int cnt = 0, nb = 0;
      const bool odd = n > kMaxBlock;
      PFV_LANES(l, n) {
        const int sfi = nsfp[a + l];
        const int f = sff[sfi];
        const int sides = (fslot[f] >= 0 ? 1 : 0) + (fother[f] >= 0 ? 1 : 0);
        nm_face[a + l] = f;
        ls[sfi] = (uint8_t)(l & 0xff);
        cnt += sides;
        nb += sides == 1 ? 1 : 0;
      }
      if (odd) atomic_max_i32(mx + 2, 1);
      part[w.lane] = cnt;
      part[16 + w.lane] = nb;
      w.lsync();
      if (w.lane0()) {
        int tc = 0, tb = 0;
        for (int i = 0; i < w.width; ++i) {
          tc += part[i];
          tb += part[16 + i];
        }
        cnt_n[v] = tc;
        nb_n[v] = tb;
      }
      w.lsync();
    });
  }
  // --- 4: one scan for the five row pointers / totals of the nodes
  Buf<TopoRec> rec_;
  TopoRec* rec = rec_.ensure(nn + 1);
  {
    const int32_t* fp = c.node_fptr;
    exclusive_scan_gen<TopoRec>(s, c.scratch, PFV_LAMBDA(int64_t v) -> TopoRec {
      const int n = fp[v + 1] - fp[v], cnt = cnt_n[v], nb = nb_n[v], deg = cnt / nd;
      TopoRec r;
      r.h = cnt;
      r.nb = nb;
      r.sq = (int64_t)n * n;
      // response table: n rows + the e-row, stride = nh rounded up to even (16-byte rows)
      r.tab = (int64_t)(n + 1) * ((cnt + 1) & ~1);
      r.tabb = 2 * (int64_t)n * nb;
      r.fl = 2.0 * n * n * n + 2.0 * nd * n * cnt + 2.0 * (1 + nd) * n * nb + 60.0 * nd * nd * deg;
      return r;
    }, rec, (size_t)nn);
  }
  // --- 5: per node, the records in entry order
  c.node_hptr.ensure(nn + 1);
  c.node_bptr.ensure(nn + 1);
  c.node_tptr.ensure(nn + 1);
  c.node_tbptr.ensure(nn + 1);
  c.h_cell.ensure(hcap);
  c.h_lf.ensure(hcap);
  c.h_sgn.ensure(hcap);
  c.h_first.ensure(hcap);
  c.node_bfaces.ensure(nsf);
  c.node_bls.ensure(nsf);
  c.node_cells.ensure(hcap / nd + 1);
  {
    const int32_t* fp = c.node_fptr;
    int32_t* hp = c.node_hptr;
    int32_t* bp = c.node_bptr;
    int64_t* tp = c.node_tptr;
    int64_t* tbp = c.node_tbptr;
    int32_t* hc = c.h_cell;
    uint8_t* lf = c.h_lf;
    int8_t* hs = c.h_sgn;
    uint8_t* first = c.h_first;
    int32_t* bf = c.node_bfaces;
    uint8_t* bl = c.node_bls;
    int32_t* ncl = c.node_cells;
    // (keys and record cells only: 4.3 KB per node.  With the cells and signs of the entries staged as well it was 9 KB,
    // 17 nodes in flight per CU, and the kernel -- a chain of dependent loads per node -- took 0.65 ms.)
    const size_t lds_bytes = (size_t)kTopoKeyCap * 2 * sizeof(int32_t) + 256;
    // One wavefront per node: a tetrahedral interior node has 36 faces (one pass of the lanes), a hexahedral one 12.
    // (Narrower lane groups were not measured; the kernel is bound by the rank loop, whose passes per node 32 lanes double
    // at 36 faces.)  The three maxima below are taken by one lane per node with a read before the atomic -- 1 M reads of
    // three addresses, not a reduction per workgroup: a wave_for work item has no hook for one.
    // Precondition of the ranks: the keys of a node are distinct, i.e. a face names a node once.  A face that lists a node
    // twice gives two sub-faces with equal keys; their records then share slots (in bounds, but which one stays is not
    // defined, unlike in the reference path).
    wave_for<64>(s, nn, lds_bytes, PFV_LAMBDA(const WaveCtx& w) {
      int32_t* keys = reinterpret_cast<int32_t*>(w.lds);   // [2n] lower / higher entry of every face of the node
      int32_t* cellS = keys + kTopoKeyCap;                 // [cnt] cells of the records, in record order
      uint8_t* bndL = reinterpret_cast<uint8_t*>(cellS + kTopoKeyCap);  // [n] boundary face
      const int64_t v = w.item;
      const int a = fp[v], n = fp[v + 1] - a;
      const TopoRec r0 = rec[v], r1 = rec[v + 1];
      const int h0 = (int)r0.h, cnt = (int)(r1.h - r0.h), b0 = (int)r0.nb, nb = (int)(r1.nb - r0.nb);
      if (w.lane0()) {
        hp[v] = h0;
        bp[v] = b0;
        tp[v] = r0.tab;
        tbp[v] = r0.tabb;
        if (v == nn - 1) {
          hp[nn] = (int32_t)r1.h;
          bp[nn] = (int32_t)r1.nb;
          tp[nn] = r1.tab;
          tbp[nn] = r1.tabb;
        }
        track_max_i32(st + 1, n);
        track_max_i32(st + 2, cnt / nd);
        track_max_i32(st + 3, nb);
        if (cnt % nd) atomic_max_i32(st + 0, 2);
      }
      if (n <= kMaxBlock) {  // (a larger node has raised the flag in phase 3)
        PFV_LANES(l, n) {
          const int f = nm_face[a + l];
          const int32_t e0 = fslot[f], e1 = fother[f];
          keys[l] = e0 < 0 ? kTopoNoKey : (e1 < 0 || e0 < e1 ? e0 : e1);
          keys[n + l] = e1 < 0 ? kTopoNoKey : (e0 < e1 ? e1 : e0);
          bndL[l] = (e0 >= 0 && e1 < 0) ? 1 : 0;
        }
        PFV_LANES(t, (4 - ((2 * n) & 3)) & 3) keys[2 * n + t] = kTopoNoKey;
        w.lsync();
        const int n4 = (2 * n + 3) >> 2;
        const TopoI4* k4 = reinterpret_cast<const TopoI4*>(keys);
        PFV_LANES(l, n) {
          const int32_t k0 = keys[l], k1 = keys[n + l];
          // (cell and sign of the two entries: loads in flight while the ranks are counted)
          const bool s0 = k0 != kTopoNoKey, s1 = k1 != kTopoNoKey;
          const int32_t c0 = s0 ? coe[k0] : -1, c1 = s1 ? coe[k1] : -1;
          const int8_t g0 = s0 ? cf_sgn[k0] : (int8_t)0, g1 = s1 ? cf_sgn[k1] : (int8_t)0;
          int q0 = 0, q1 = 0;
          for (int u = 0; u < n4; ++u) {
            const TopoI4 q = k4[u];
            q0 += (q.x < k0 ? 1 : 0) + (q.y < k0 ? 1 : 0) + (q.z < k0 ? 1 : 0) + (q.w < k0 ? 1 : 0);
            q1 += (q.x < k1 ? 1 : 0) + (q.y < k1 ? 1 : 0) + (q.z < k1 ? 1 : 0) + (q.w < k1 ? 1 : 0);
          }
          if (s0) {
            cellS[q0] = c0;
            lf[h0 + q0] = (uint8_t)l;
            first[h0 + q0] = 1;
            hs[h0 + q0] = g0;
          }
          if (s1) {
            cellS[q1] = c1;
            lf[h0 + q1] = (uint8_t)l;
            first[h0 + q1] = c1 == c0 ? 1 : 0;
            hs[h0 + q1] = g1;
          }
        }
        w.lsync();
        PFV_LANES(p, cnt) {
          const int32_t cc = cellS[p];
          hc[h0 + p] = cc;
          // nd faces of a cell meet here, cells ascending
          const bool bad = (p % nd) ? (cc != cellS[p - 1]) : (p > 0 && cc <= cellS[p - 1]);
          if (bad) atomic_max_i32(st + 0, 2);
          if (p % nd == 0) ncl[(h0 + p) / nd] = cc;
        }
        if (nb > 0) {
          PFV_LANES(l, n) {
            if (bndL[l]) {
              int o = b0;
              for (int t = 0; t < l; ++t) o += bndL[t];
              bf[o] = nm_face[a + l];
              bl[o] = (uint8_t)l;
            }
          }
        }
      }
      w.lsync();
    });
  }

  // --- 6: processing order of the face kernels (Morton curve through the face centres) and launch order of the
  // interaction-region kernel (nodes bucketed by block size), as in the reference path
  c.face_order.ensure(nf);
  {
    uint32_t* k = key_in;
    int32_t* v = val_in;
    const double* fc = c.fcen;
    double lo[3], sc[3];
    for (int d = 0; d < 3; ++d) {
      lo[d] = c.bbox_lo[d];
      const double ext = c.bbox_hi[d] - c.bbox_lo[d];
      sc[d] = ext > 0 ? 1023.999 / ext : 0.0;
    }
    const double lo0 = lo[0], lo1 = lo[1], lo2 = lo[2], sc0 = sc[0], sc1 = sc[1], sc2 = sc[2];
    parallel_for(s, nf, PFV_LAMBDA(int64_t f) {
      uint32_t q[3];
      q[0] = (uint32_t)((fc[f] - lo0) * sc0);
      q[1] = (uint32_t)((fc[nf + f] - lo1) * sc1);
      q[2] = (uint32_t)((fc[2 * nf + f] - lo2) * sc2);
      uint32_t code = 0;
      for (int d = 0; d < 3; ++d) {
        uint32_t x = q[d] & 0x3ffu;  // spread 10 bits to every third position
        x = (x | (x << 16)) & 0x030000ffu;
        x = (x | (x << 8)) & 0x0300f00fu;
        x = (x | (x << 4)) & 0x030c30c3u;
        x = (x | (x << 2)) & 0x09249249u;
        code |= x << d;
      }
      k[f] = code;
      v[f] = (int32_t)f;
      ns[f] = (fslot[f] >= 0 ? 1 : 0) + (fother[f] >= 0 ? 1 : 0);  // (this pass over the faces writes face_nsides too)
    });
    sort_pairs(s, c.scratch, key_in.p, key_out.p, val_in.p, c.face_order.p, (size_t)nf, 30);
  }
  constexpr int nclass = kNumClasses;
  constexpr int kPack = 13;  // words of the packed read before the class bounds
  Buf<int64_t> pack_;
  int64_t* pk = pack_.ensure(kPack + nclass + 1);
  {
    TopoClassBounds bd;
    for (int i = 0; i < nclass; ++i) bd.b[i] = kClassBounds[i];
    uint32_t* k = key_in;
    int32_t* v = val_in;
    c.node_order.ensure(nn);
    const int32_t* fp = c.node_fptr;
    parallel_for(s, nn, PFV_LAMBDA(int64_t node) {
      const int n = fp[node + 1] - fp[node];
      int cls = 0;
      while (cls < nclass - 1 && n > bd.b[cls]) ++cls;
      k[node] = (uint32_t)cls;
      v[node] = (int32_t)node;
    });
    sort_pairs(s, c.scratch, key_in.p, key_out.p, val_in.p, c.node_order.p, (size_t)nn, 4);
    const uint32_t* ks = key_out;
    parallel_for(s, nclass + 2, PFV_LAMBDA(int64_t t) {
      if (t <= nclass) {
        pk[kPack + t] = lower_bound_idx<uint32_t>(ks, (int)nn, (uint32_t)t);
      } else {
        const TopoRec tot = rec[nn];
        pk[0] = tot.h;
        pk[1] = tot.nb;
        pk[2] = tot.sq;
        pk[3] = tot.tab;
        pk[4] = tot.tabb;
        reinterpret_cast<double*>(pk)[5] = tot.fl;
        for (int i = 0; i < 4; ++i) pk[6 + i] = st[i];
        pk[10] = mx[2];
        pk[11] = mx[0];
        pk[12] = mx[1];
      }
    });
  }
  // the one blocking read of the rebuild; the checks in the order the reference path makes them
  int64_t ph[kPack + nclass + 1];
  be_d2h(ph, pk, sizeof(ph), s);
  if (ph[10] != 0) return false;
  const int64_t nh = ph[0];
  if (nh >= (int64_t(1) << 31)) throw Error(5, "more than 2^31 sub-half-faces on one device");
  c.nh = nh;
  c.max_face_nodes = (int)ph[11];
  if (c.max_face_nodes > kMaxFaceNodes)
    throw Error(PFV_ERR_UNSUPPORTED, "faces with more than 8 nodes are not supported");
  c.max_cell_faces = (int)ph[12];
  if (c.max_cell_faces > kMaxCellFaces)
    throw Error(PFV_ERR_UNSUPPORTED, "cells with more than 16 faces are not supported");
  if (ph[6] == 2)
    throw Error(PFV_ERR_CELL_SHAPE,
                "a cell does not have exactly nd faces meeting in one of its nodes (e.g. pyramid)");
  // (status 1, "cell_faces / face_nodes are inconsistent", is the reference path's alone: here every record comes from
  // the sub-face list it would be searched in)
  c.max_block = (int)ph[7];
  c.max_deg = (int)ph[8];
  c.max_bnd_per_node = (int)ph[9];
  if (c.max_block > kMaxBlock || c.max_deg > kMaxBlock)
    throw Error(PFV_ERR_UNSUPPORTED, "more than 255 faces or cells meet in one node");
  c.sum_block_sq = ph[2];
  std::memcpy(&c.stats.node_flops, &ph[5], sizeof(double));
  c.tab_len = ph[3];
  c.tabb_len = ph[4];
  c.class_begin.assign(nclass + 1, nn);
  for (int cls = 0; cls <= nclass; ++cls) c.class_begin[cls] = ph[kPack + cls];
  c.have_topology = true;
  c.topo_key = 0;
  c.stats.num_nodes = nn;
  c.stats.num_sub_half_faces = nh;
  c.stats.sum_block_sq = c.sum_block_sq;
  c.stats.max_block = c.max_block;
  c.stats.node_table_doubles = c.tab_len + c.tabb_len;
  return true;
}

static void build_topology(pfv_ctx_impl& c) {
  // PFV_TOPO_LEGACY=1 (read per call): the reference construction, the A/B partner of the node-cooperative one
  // A hand-over costs both constructions on every rebuild (a grid with a three-sided face is built by the reference path
  // without an error): pfv_stats.topology_reference_path shows it.
  c.topo_path = 1;
  if (env_int("PFV_TOPO_LEGACY", 0) != 0 || !build_topology_nodes(c)) {
    c.topo_path = 0;
    build_topology_legacy(c);
  }
  c.stats.topology_reference_path = c.topo_path == 0 ? 1 : 0;
}

// ------------------------------------------------------------------------------------
// Sorted set union in LDS, one wavefront per work item.  `buf` holds nl ascending lists
// (list j = buf[off[j] .. off[j+1]), no repeats inside a list).  Every element finds its
// rank in the merged sequence with one binary search per other list (ties: earlier list
// first), is scattered to merged[rank]; run heads are marked in a bit mask and their output
// positions are popcounts of the mask.  ~10 dependent LDS reads per element instead of a
// serial k-way merge per thread.  Returns the number of distinct values; writes them
// ascending to `out` (LDS or global) unless out == nullptr.
template <class RankT = uint8_t, int EPL = 4>
PFV_FN int merge_unique_lds(const WaveCtx& w, const int32_t* buf, const int32_t* off, int nl,
                            int32_t* merged, unsigned long long* mask, int32_t* out,
                            RankT* rank_out = nullptr) {
  const int m = off[nl];
  const int nw = (m + 63) >> 6;
  PFV_LANES(i, nw) mask[i] = 0ull;
  // Every lane ranks EPL of its elements at once: the binary searches of one element are a chain of
  // dependent LDS reads (~10 per element), those of different elements are independent -- run in
  // lockstep they overlap instead of queueing behind each other (the phase is bound by that latency).
  for (int e0 = w.lane; e0 < m; e0 += w.width * EPL) {
    int el[EPL], li[EPL], rank[EPL];
    int32_t v[EPL];
#pragma unroll
    for (int u = 0; u < EPL; ++u) {
      const int e = e0 + u * w.width;
      el[u] = e < m ? e : -1;
      const int ee = e < m ? e : 0;
      int l = 0;
      while (l + 1 < nl && ee >= off[l + 1]) ++l;
      li[u] = l;
      v[u] = buf[ee];
      rank[u] = ee - off[l];
    }
    for (int j = 0; j < nl; ++j) {
      const int32_t* Lj = buf + off[j];
      const int n = off[j + 1] - off[j];
      int lo[EPL], hi[EPL];
#pragma unroll
      for (int u = 0; u < EPL; ++u) { lo[u] = 0; hi[u] = (el[u] >= 0 && j != li[u]) ? n : 0; }
      for (int span = n; span > 0; span >>= 1) {  // ceil(log2(n + 1)) halvings settle every search
#pragma unroll
        for (int u = 0; u < EPL; ++u) {
          if (lo[u] < hi[u]) {
            const int mid = (lo[u] + hi[u]) >> 1;
            const int32_t a = Lj[mid];
            // lists before the element's own: count entries <= v (upper bound); after: entries < v
            const bool right = (j < li[u]) ? (a <= v[u]) : (a < v[u]);
            if (right) lo[u] = mid + 1; else hi[u] = mid;
          }
        }
      }
#pragma unroll
      for (int u = 0; u < EPL; ++u) rank[u] += lo[u];
    }
#pragma unroll
    for (int u = 0; u < EPL; ++u) {
      if (el[u] >= 0) {
        merged[rank[u]] = v[u];
        if (rank_out) rank_out[el[u]] = (RankT)rank[u];
      }
    }
  }
  w.sync();
  PFV_LANES(k, m) {
    if (k == 0 || merged[k] != merged[k - 1]) atomic_or_u64(mask + (k >> 6), 1ull << (k & 63));
  }
  w.sync();
  int total = 0;
  for (int i = 0; i < nw; ++i) total += popcount64(mask[i]);
  if (out) {
    PFV_LANES(k, m) {
      const unsigned long long word = mask[k >> 6];
      if ((word >> (k & 63)) & 1ull) {
        int pos = popcount64(word & ((1ull << (k & 63)) - 1ull));
        for (int i = 0; i < (k >> 6); ++i) pos += popcount64(mask[i]);
        out[pos] = merged[k];
      }
    }
  }
  w.sync();
  return total;
}

// ------------------------------------------------------------------------------------
// K-way merge of ascending id lists by ONE lane (the lists sit in the lane's own LDS strip, concatenated;
// list i = strip[beg[i] .. end[i])).  Emits the distinct ids ascending and, per output column, which element
// of every list fed it (its index in the concatenation, 0xff = none) -- what the cooperative
// merge_unique_lds + rank / popcount passes above produce with ~10 dependent LDS searches per element and
// several wavefront syncs per face.  Here a face costs ~(distinct ids) x K LDS reads in one lane, 64 faces
// advance per wavefront, and nothing is exchanged between lanes: the kernel is a plain grid of independent
// lanes (5.6 -> <1 ms for the 3.9 M face rows of the 2 M-cell grid).
template <int K>
PFV_FN int merge_lists_serial(const int32_t* const (&base)[K], const int (&len)[K], const int (&eoff)[K], int32_t* ids,
                              uint8_t* pairs, int pair_stride, uint8_t* first_src = nullptr) {
  // list i = base[i][0 .. len[i]); eoff[i] = index of its first element in the concatenation of the lists
  int pos[K];
#pragma unroll
  for (int i = 0; i < K; ++i) pos[i] = 0;
  int k = 0;
  for (;;) {
    int32_t h[K];
    int32_t mn = 0x7fffffff;
#pragma unroll
    for (int i = 0; i < K; ++i) {
      h[i] = pos[i] < len[i] ? base[i][pos[i]] : 0x7fffffff;
      mn = h[i] < mn ? h[i] : mn;
    }
    if (mn == 0x7fffffff) break;
    if (ids) ids[k] = mn;
    int first = -1;
#pragma unroll
    for (int i = 0; i < K; ++i) {
      const bool hit = h[i] == mn;
      if (pairs && i < pair_stride) pairs[k * pair_stride + i] = hit ? (uint8_t)(eoff[i] + pos[i]) : (uint8_t)0xff;
      if (hit && first < 0) first = eoff[i] + pos[i];
      pos[i] += hit ? 1 : 0;
    }
    if (first_src) first_src[k] = (uint8_t)first;  // one element (index in the concatenation) that carries the id
    ++k;
  }
  return k;
}

// rows of flux / bound_pressure_cell (which = 0: cells around the nodes of the face) or of bound_flux /
// bound_pressure_face (which = 1: boundary faces around them), one lane per face.  Count-only when ids_base
// is null; rows at ids_base + row_off(f) with row_off = ip[f] (compact) or f * SF (staging area).
template <int K>
static void symbolic_face_rows_serial(pfv_ctx_impl& c, int which, const int32_t* sub, int64_t nitems, int cap,
                                      const int32_t* ip, int64_t SF, int32_t* ids_base, uint8_t* pairs_base,
                                      int32_t* ln, int32_t* st) {
  stream_t s = c.stream;
  const int nd = c.nd;
  const int32_t* fn_ptr = c.fn_ptr;
  const int32_t* fn_idx = c.fn_idx;
  const int32_t* hp = c.node_hptr;
  const int32_t* ncl = c.node_cells;
  const int32_t* bp = c.node_bptr;
  const int32_t* bf = c.node_bfaces;
  const int maxfn = std::max(c.max_face_nodes, 1);
  // The lists are staged in an LDS strip per lane (64 x cap x 4 B per wavefront).  PFV_SYMB_LDS=0 reads the list heads
  // straight from the node lists instead (no LDS footprint, so that the kernel co-resides with the interaction-region
  // kernel on the second stream): measured 1.3 ms slower per step -- the node kernel loses more than this one gains.
  // Output through LDS (PFV_SYMB_OUT_LDS, default): a lane emitting its row entry by entry writes 4 bytes per store to
  // an address 64 lanes apart -- 218 M such stores for the flux rows of the 2 M-cell grid took 4 of the kernel's 5.3 ms
  // (count-only pass: 1 ms).  The lanes now merge into LDS strips and the wavefront copies the 64 rows out one after the
  // other with coalesced stores.  The list heads are then read in place (the strips of the inputs would not fit beside
  // those of the outputs; the lists are L2-resident and the heads of the K lists are independent loads).
  // With the column -> list-element map (pairs) asked for, the ids themselves need no LDS: the copy-out reads them
  // back from the lists through that map (PFV_SYMB_OUT_LDS=2, default) -- 15 KB instead of 33 KB of LDS per wavefront,
  // 10 instead of 4 wavefronts per CU to hide the latency of the list reads.
  const int out_mode = ids_base != nullptr ? env_int("PFV_SYMB_OUT_LDS", 2) : 0;
  const bool pairs_lds = out_mode == 2 && pairs_base != nullptr && (size_t)64 * cap * maxfn <= 48 * 1024;
  const bool out_lds = !pairs_lds && out_mode != 0 &&
                       (size_t)64 * ((size_t)(cap | 1) * 4 + (pairs_base ? (size_t)cap * maxfn : 0)) <= 60 * 1024;
  const bool use_lds = !out_lds && !pairs_lds && env_int("PFV_SYMB_LDS", 1) != 0;
  const int stride = cap | 1;  // odd: the 64 strips start in different LDS banks
  const int64_t nblocks = (nitems + 63) / 64;
  const size_t pair_bytes = pairs_base ? (size_t)cap * maxfn : 0;
  const size_t head_bytes = 64 * (sizeof(int64_t) + sizeof(int32_t));
  const size_t lds_bytes = pairs_lds ? head_bytes + (size_t)64 * K * (sizeof(int32_t) + 4) + 64 * pair_bytes + 16
                           : out_lds ? head_bytes + (size_t)64 * stride * sizeof(int32_t) + 64 * pair_bytes + 16
                                     : (use_lds ? (size_t)64 * stride * sizeof(int32_t) : (size_t)0);
  const int32_t* srcarr = which == 0 ? ncl : bf;
  // (block copy-out, below: staged rows of consecutive faces, column maps asked for, 4-byte aligned LDS rows)
  const bool block_out = pairs_lds && ip == nullptr && sub == nullptr && pairs_base != nullptr && (int64_t)cap == SF &&
                         env_int("PFV_SYMB_BLOCK_OUT", 1) != 0;
  wave_for<64>(s, nblocks, lds_bytes, PFV_LAMBDA(const WaveCtx& w) {
    int64_t* offL = reinterpret_cast<int64_t*>(w.lds);                         // [64] row offsets (out_lds / pairs_lds)
    int32_t* cntL = reinterpret_cast<int32_t*>(offL + 64);                     // [64] row lengths
    int32_t* outL = cntL + 64;                                                 // out_lds: [64][stride] merged ids
    uint8_t* prsL = reinterpret_cast<uint8_t*>(outL + (size_t)64 * stride);    //          [64][cap * maxfn] column -> list elements
    int32_t* boffL = cntL + 64;                                                // pairs_lds: [64][K] first element of every list in srcarr
    int32_t* eoffL = boffL + (size_t)64 * K;                                   //            [64][K] its index in the concatenation
    if (pairs_lds) prsL = reinterpret_cast<uint8_t*>(eoffL + (size_t)64 * K);
    PFV_LANES(fi, 64) {
      const int64_t it = w.item * 64 + fi;
      if (out_lds || pairs_lds) cntL[fi] = 0;
      if (it < nitems) {
        const int64_t f = sub ? (int64_t)sub[it] : it;
        int32_t* strip = use_lds ? reinterpret_cast<int32_t*>(w.lds) + (size_t)fi * stride : nullptr;
        const int a = fn_ptr[f], nl = fn_ptr[f + 1] - a;
        const int32_t* base[K];
        int len[K], eoff[K];
        int m = 0;
#pragma unroll
        for (int i = 0; i < K; ++i) {
          eoff[i] = m;
          len[i] = 0;
          base[i] = ncl;
          if (i < nl) {
            const int v = fn_idx[a + i];
            const int32_t* src = which == 0 ? ncl + hp[v] / nd : bf + bp[v];
            const int n = which == 0 ? (hp[v + 1] - hp[v]) / nd : bp[v + 1] - bp[v];
            if (use_lds) {
              for (int t = 0; t < n; ++t) strip[m + t] = src[t];
              base[i] = strip + m;
            } else {
              base[i] = src;
            }
            len[i] = n;
            m += n;
          }
          if (pairs_lds) {
            boffL[fi * K + i] = (int32_t)(base[i] - srcarr);
            eoffL[fi * K + i] = eoff[i];
          }
        }
        const int64_t off = ids_base ? (ip ? (int64_t)ip[f] : f * SF) : 0;
        int32_t* ids = ids_base ? ids_base + off : nullptr;
        uint8_t* pairs = (ids_base && pairs_base) ? pairs_base + off * maxfn : nullptr;
        if (out_lds) {
          ids = outL + (size_t)fi * stride;
          pairs = pairs_base ? prsL + (size_t)fi * pair_bytes : nullptr;
          offL[fi] = off;
        } else if (pairs_lds) {
          ids = nullptr;
          pairs = prsL + (size_t)fi * pair_bytes;
          offL[fi] = off;
        }
        const int cntv = merge_lists_serial<K>(base, len, eoff, ids, pairs, maxfn);
        if (out_lds || pairs_lds) cntL[fi] = cntv;
        if (ln) {
          ln[f] = cntv;
          track_max_i32(st + 5 + which, cntv);
        }
      }
    }
    if (pairs_lds && block_out) {
      // Staging area at a fixed stride and the faces of the wavefront consecutive: its 64 rows are ONE contiguous block
      // of ids (64 x SF) and one of column maps (64 x SF x maxfn bytes).  Copied out as blocks -- every lane walks the
      // block with stride 64 -- instead of row by row: ~1.3 k instead of ~3.2 k instructions per wavefront (the slots
      // behind a row's last entry carry whatever the LDS held: nobody reads them).
      w.sync();
      const int64_t f0 = w.item * 64;
      const int nvalid = (int)(nitems - f0 < 64 ? nitems - f0 : 64);
      {
        int32_t* dst = ids_base + f0 * SF;
        int r = 0, t = w.lane;
        while (t >= (int)SF) { t -= (int)SF; ++r; }
        for (; r < nvalid;) {
          if (t < cntL[r]) {
            const uint8_t* pr = prsL + (size_t)r * pair_bytes + (size_t)t * maxfn;
            int i = 0;
            while (i + 1 < maxfn && pr[i] == 0xff) ++i;
            dst[(int64_t)r * SF + t] = srcarr[boffL[r * K + i] + ((int)pr[i] - eoffL[r * K + i])];
          }
          t += w.width;
          while (t >= (int)SF) { t -= (int)SF; ++r; }
        }
      }
      if ((pair_bytes & 3) == 0) {
        uint32_t* dw = reinterpret_cast<uint32_t*>(pairs_base + f0 * SF * maxfn);  // (SF maxfn = pair_bytes per row)
        const uint32_t* sw = reinterpret_cast<const uint32_t*>(prsL);
        const int words = nvalid * (int)(pair_bytes >> 2);
        PFV_LANES(x, words) dw[x] = sw[x];
      } else {
        uint8_t* dp = pairs_base + f0 * SF * maxfn;
        PFV_LANES(x, nvalid * (int)pair_bytes) dp[x] = prsL[x];
      }
      w.sync();
    } else if (out_lds || pairs_lds) {
      w.sync();
      for (int r = 0; r < 64; ++r) {
        const int cntv = cntL[r];
        if (cntv > 0) {
          int32_t* dst = ids_base + offL[r];
          const uint8_t* sp = prsL + (size_t)r * pair_bytes;
          if (pairs_lds) {
            PFV_LANES(t, cntv) {
              const uint8_t* pr = sp + (size_t)t * maxfn;
              int i = 0;
              while (i + 1 < maxfn && pr[i] == 0xff) ++i;  // a list that fed the column
              dst[t] = srcarr[boffL[r * K + i] + ((int)pr[i] - eoffL[r * K + i])];
            }
          } else {
            const int32_t* src = outL + (size_t)r * stride;
            PFV_LANES(t, cntv) dst[t] = src[t];
          }
          if (pairs_base) {
            uint8_t* dp = pairs_base + offL[r] * maxfn;
            PFV_LANES(x, cntv * maxfn) dp[x] = sp[x];
          }
        }
      }
      w.sync();
    }
  });
}

// rows of A = div @ flux (cells around the nodes of the cell), one lane per cell: distinct nodes of its faces, then
// the K-way merge of their cell lists.  A cell with more than K distinct nodes raises st[14] (the caller falls back).
template <int K>
static void symbolic_cell_rows_serial(pfv_ctx_impl& c, int cap_n, int maxdeg, const int32_t* ap, int64_t SC,
                                      int32_t* ids_base, int32_t* ln, int32_t* st) {
  stream_t s = c.stream;
  const int nd = c.nd;
  const int64_t nc = c.nc;
  const int32_t* fn_ptr = c.fn_ptr;
  const int32_t* fn_idx = c.fn_idx;
  const int32_t* cf_ptr = c.cf_ptr;
  const int32_t* cf_idx = c.cf_idx;
  const int32_t* hp = c.node_hptr;
  const int32_t* ncl = c.node_cells;
  (void)maxdeg;
  const int stride = (cap_n + K) | 1;  // face nodes with repeats + the distinct ones
  const int64_t nblocks = (nc + 63) / 64;
  // rows merged into LDS strips and copied out with coalesced stores (see symbolic_face_rows_serial): a row has at most
  // K * maxdeg entries
  const int ostride = (K * std::max(maxdeg, 1)) | 1;
  // PFV_SYMB_OUT_LDS=2 (default): one byte per entry in LDS -- which element of the concatenated lists carries the id --
  // instead of the id; the copy-out reads the id back from the list (12 KB instead of 29 KB of LDS per wavefront)
  const int out_mode = ids_base != nullptr ? env_int("PFV_SYMB_OUT_LDS", 2) : 0;
  const bool src_lds = out_mode == 2 && K * std::max(maxdeg, 1) < 255;
  const bool out_lds = !src_lds && out_mode != 0 && (size_t)64 * (stride + ostride) * sizeof(int32_t) <= 60 * 1024;
  const int bstride = (ostride + 3) & ~3;  // bytes per row of the source map
  const size_t head_bytes = 64 * (sizeof(int64_t) + sizeof(int32_t));  // row offsets, row lengths
  const size_t lds_bytes = head_bytes + (size_t)64 * stride * sizeof(int32_t) +
                           (src_lds ? (size_t)64 * (2 * K * sizeof(int32_t) + bstride) : 0) +
                           (out_lds ? (size_t)64 * ostride * sizeof(int32_t) : 0) + 16;
  wave_for<64>(s, nblocks, lds_bytes, PFV_LAMBDA(const WaveCtx& w) {
    int64_t* offL = reinterpret_cast<int64_t*>(w.lds);
    int32_t* cntL = reinterpret_cast<int32_t*>(offL + 64);
    int32_t* nodeL = cntL + 64;                       // [64][stride] face nodes / distinct nodes of every cell
    int32_t* outL = nodeL + (size_t)64 * stride;      // out_lds: [64][ostride] merged rows
    int32_t* boffL = outL;                            // src_lds: [64][K] first element of every list in node_cells
    int32_t* eoffL = boffL + (size_t)64 * K;          //          [64][K] its index in the concatenation
    uint8_t* srcL = reinterpret_cast<uint8_t*>(eoffL + (size_t)64 * K);  // [64][bstride] entry -> element
    PFV_LANES(ci, 64) {
      const int64_t cell = w.item * 64 + ci;
      if (out_lds || src_lds) cntL[ci] = 0;
      if (cell < nc) {
        int32_t* nodes = nodeL + (size_t)ci * stride;  // face nodes, with repeats
        int32_t* un = nodes + cap_n;                                               // distinct nodes (<= K)
        int m = 0;
        for (int e = cf_ptr[cell]; e < cf_ptr[cell + 1]; ++e) {
          const int f = cf_idx[e];
          for (int t = fn_ptr[f]; t < fn_ptr[f + 1]; ++t) nodes[m++] = fn_idx[t];
        }
        int k1 = 0;
        bool over = false;
        for (int e = 0; e < m; ++e) {
          const int32_t v = nodes[e];
          bool seen = false;
          for (int q = 0; q < k1; ++q) seen = seen || (un[q] == v);
          if (!seen) {
            if (k1 < K) un[k1++] = v; else over = true;
          }
        }
        if (over) {
          atomic_max_i32(st + 14, 1);
        } else {
          const int32_t* base[K];
          int len[K], eoff[K];
          int mm = 0;
#pragma unroll
          for (int i = 0; i < K; ++i) {
            eoff[i] = mm;
            len[i] = 0;
            base[i] = ncl;
            if (i < k1) {
              const int v = un[i];
              const int n = (hp[v + 1] - hp[v]) / nd;
              base[i] = ncl + hp[v] / nd;  // (read in place: L1 / L2 resident, see symbolic_face_rows_serial)
              len[i] = n;
              mm += n;
            }
            if (src_lds) {
              boffL[ci * K + i] = (int32_t)(base[i] - ncl);
              eoffL[ci * K + i] = eoff[i];
            }
          }
          const int64_t off = ids_base ? (ap ? (int64_t)ap[cell] : cell * SC) : 0;
          int32_t* ids = ids_base ? ids_base + off : nullptr;
          uint8_t* first_src = nullptr;
          if (out_lds) {
            ids = outL + (size_t)ci * ostride;
            offL[ci] = off;
          } else if (src_lds) {
            ids = nullptr;
            first_src = srcL + (size_t)ci * bstride;
            offL[ci] = off;
          }
          const int cntv = merge_lists_serial<K>(base, len, eoff, ids, nullptr, 0, first_src);
          if (out_lds || src_lds) cntL[ci] = cntv;
          if (ln) {
            ln[cell] = cntv;
            track_max_i32(st + 7, cntv);
          }
        }
      }
    }
    if (out_lds || src_lds) {
      w.sync();
      for (int r = 0; r < 64; ++r) {
        const int cntv = cntL[r];
        if (cntv > 0) {
          int32_t* dst = ids_base + offL[r];
          if (src_lds) {
            const uint8_t* sp = srcL + (size_t)r * bstride;
            PFV_LANES(t, cntv) {
              const int e = sp[t];
              int i = 0;
#pragma unroll
              for (int q = 1; q < K; ++q) i = e >= eoffL[r * K + q] ? q : i;  // (unused lists start at the total length)
              dst[t] = ncl[boffL[r * K + i] + (e - eoffL[r * K + i])];
            }
          } else {
            const int32_t* src = outL + (size_t)r * ostride;
            PFV_LANES(t, cntv) dst[t] = src[t];
          }
        }
      }
      w.sync();
    }
  });
}

static void finish_pattern(pfv_ctx_impl& c, CsrPattern& P, Buf<int64_t>& rowptr64, int64_t nrows,
                           int64_t ncols) {
  stream_t s = c.stream;
  const int64_t nnz = read_scalar<int64_t>(s, rowptr64.p + nrows);
  if (nnz >= (int64_t(1) << 31)) throw Error(PFV_ERR_UNSUPPORTED, "matrix with more than 2^31 entries");
  P.nrows = nrows;
  P.ncols = ncols;
  P.nnz = nnz;
  P.indptr.ensure(nrows + 1);
  P.indices.ensure(nnz);
  int32_t* ip = P.indptr;
  const int64_t* r64 = rowptr64;
  parallel_for(s, nrows + 1, PFV_LAMBDA(int64_t i) { ip[i] = (int32_t)r64[i]; });
}

PFV_HD inline unsigned long long mix64(unsigned long long z) {
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}
// 64-bit digest of a pattern's row pointers and column indices (sum of per-entry hashes of (value, position); one read
// of the index arrays, ~0.2 ms for 140 M entries), left in work[T + 1024] on the device: the evidence that a pattern
// equals the one a saved structure (AMG aggregate maps, SpMV windows) was built for -- together with equal sizes; a
// false match needs a 2^-64 hash collision.  Returns the device address of the result.
static const unsigned long long* launch_pattern_checksum(pfv_ctx_impl& c, Buf<unsigned long long>& work,
                                                         const CsrPattern& P) {
  stream_t s = c.stream;
  constexpr int64_t T = 1 << 20;  // (65 536 threads left the read latency-bound: 0.86 ms for 140 M entries)
  unsigned long long* part = work.ensure(T + 1024 + 1);
  const int32_t* ip = P.indptr;
  const int32_t* ix = P.indices;
  const int64_t nr = P.nrows + 1, nz = P.nnz;
  parallel_for(s, T, PFV_LAMBDA(int64_t t) {
    // per entry a non-linear mix of (value, position) -- multiply, xor-shift, multiply (the splitmix64 finaliser) --
    // summed: two patterns that differ in any entries collide with probability ~2^-64, not whenever a weighted SUM of
    // the differences cancels (an additive position-weighted sum, as before, is linear in the index values)
    unsigned long long h = 0;
    for (int64_t e = t; e < nz; e += T)
      h += mix64((((unsigned long long)(unsigned)ix[e]) << 32 | 0x1ull) ^ ((unsigned long long)e * 0x9E3779B97F4A7C15ull));
    for (int64_t r = t; r < nr; r += T)
      h += mix64((((unsigned long long)(unsigned)ip[r]) << 32 | 0x2ull) ^ ((unsigned long long)r * 0xC2B2AE3D27D4EB4Full));
    part[t] = h;
  });
  parallel_for(s, 1024, PFV_LAMBDA(int64_t t) {
    unsigned long long h = 0;
    for (int i = 0; i < 1024; ++i) h += part[t + 1024 * (int64_t)i];  // coalesced across t
    part[T + t] = h;
  });
  parallel_for(s, 1, PFV_LAMBDA(int64_t) {
    unsigned long long h = 0;
    for (int i = 0; i < 1024; ++i) h += part[T + i];
    part[T + 1024] = h ? h : 1ull;  // (0 means "no checksum")
  });
  return part + T + 1024;
}

// 64-bit digest of everything the symbolic phase (build_symbolic) reads of a freshly built topology: the node-major cell
// and boundary-face lists, their row pointers, the processing order of the faces, and the sizes / maxima that shape its
// launches.  (The face-node and cell-face arrays are the caller's grid: they only change through pfv_set_grid, which
// voids the saved key.)  Equal digests + equal sizes prove that build_symbolic would write, bit for bit, the patterns,
// column maps and face records the handle still holds -- a rebuilt discretization then keeps them (porefv.hip:
// symbolic_outputs_still_valid) instead of spending its longest integer phase on reproducing them; a false match needs a
// 2^-64 collision of a non-linear per-entry hash, as for launch_pattern_checksum.  ~13 M int32 at 2 M tetrahedra: 0.05 ms
// + one read-back.
static unsigned long long topology_digest(pfv_ctx_impl& c) {
  stream_t s = c.stream;
  constexpr int64_t T = 1 << 18;
  unsigned long long* part = c.csum_work.ensure((1 << 20) + 1024 + 1);
  const int nd = c.nd;
  const int64_t nn = c.nn, nf = c.nf;
  const int32_t* hp = c.node_hptr;
  const int32_t* ncl = c.node_cells;
  const int32_t* bp = c.node_bptr;
  const int32_t* bf = c.node_bfaces;
  const int32_t* fo = c.face_order;
  const int64_t ncells = c.nh / nd;
  parallel_for(s, T, PFV_LAMBDA(int64_t t) {
    unsigned long long h = 0;
    const int64_t nb = bp[nn];
    for (int64_t e = t; e < nn + 1; e += T) {
      h += mix64((((unsigned long long)(unsigned)hp[e]) << 32 | 0x1ull) ^ ((unsigned long long)e * 0x9E3779B97F4A7C15ull));
      h += mix64((((unsigned long long)(unsigned)bp[e]) << 32 | 0x2ull) ^ ((unsigned long long)e * 0xC2B2AE3D27D4EB4Full));
    }
    for (int64_t e = t; e < ncells; e += T)
      h += mix64((((unsigned long long)(unsigned)ncl[e]) << 32 | 0x3ull) ^ ((unsigned long long)e * 0x165667B19E3779F9ull));
    for (int64_t e = t; e < nb; e += T)
      h += mix64((((unsigned long long)(unsigned)bf[e]) << 32 | 0x4ull) ^ ((unsigned long long)e * 0x27D4EB2F165667C5ull));
    for (int64_t e = t; e < nf; e += T)
      h += mix64((((unsigned long long)(unsigned)fo[e]) << 32 | 0x5ull) ^ ((unsigned long long)e * 0x85EBCA77C2B2AE63ull));
    part[t] = h;
  });
  parallel_for(s, 1024, PFV_LAMBDA(int64_t t) {
    unsigned long long h = 0;
    for (int i = 0; i < (int)(T / 1024); ++i) h += part[t + 1024 * (int64_t)i];
    part[T + t] = h;
  });
  parallel_for(s, 1, PFV_LAMBDA(int64_t) {
    unsigned long long h = 0;
    for (int i = 0; i < 1024; ++i) h += part[T + i];
    part[T + 1024] = h;
  });
  unsigned long long dev = read_scalar<unsigned long long>(s, part + T + 1024);
  // host-side scalars: sizes and the maxima the launches are shaped by
  const long long sc[] = {(long long)nd, (long long)c.nc, (long long)nf, (long long)nn, (long long)c.ncf, (long long)c.nsf,
                          (long long)c.nh, (long long)c.max_face_nodes, (long long)c.max_deg,
                          (long long)c.max_bnd_per_node, (long long)c.max_cell_faces};
  int k = 0;
  for (long long v : sc) dev += mix64((unsigned long long)v ^ (0xD6E8FEB86659FD93ull * (unsigned long long)(++k)));
  return dev ? dev : 1ull;  // (0 means "no key")
}

// index array of the vector_source pattern (see build_symbolic), on first use
static void ensure_vs_indices(pfv_ctx_impl& c) {
  if (c.vs_implicit)
    throw Error(PFV_ERR_UNSUPPORTED, "vector_source has more than 2^31 entries on this handle: its CSR arrays are not "
                                     "formed -- fetch it by rows (pfv_get_matrix_rows), apply it with pfv_matrix_apply");
  if (!c.vs_indices_pending) return;
  stream_t s = c.stream;
  const int nd = c.nd;
  const int64_t nnz = c.pat_vs.nnz;
  const int32_t* ix = c.pat_flux.indices;
  int32_t* vx = c.pat_vs.indices.ensure(std::max<int64_t>(nnz, 1));
  parallel_for(s, nnz, PFV_LAMBDA(int64_t q) {
    const int64_t p = q / nd;
    vx[q] = ix[p] * nd + (int32_t)(q - p * nd);
  });
  c.vs_indices_pending = false;
}

// The patterns of the face matrices (flux, bound_flux, vector_source) and the face records -- what the face kernel
// needs --, then the pattern of A = div flux and its checksum -- what the assembly needs.
static void build_symbolic(pfv_ctx_impl& c) {
  ++c.symbolic_epoch;
  c.symb_key = 0;  // (the outputs are being replaced: valid again once the pattern of A is through)
  stream_t s = c.stream;
  const int nd = c.nd;
  const int64_t nc = c.nc, nf = c.nf;
  const int32_t* fn_ptr = c.fn_ptr;
  const int32_t* fn_idx = c.fn_idx;
  const int32_t* cf_ptr = c.cf_ptr;
  const int32_t* cf_idx = c.cf_idx;
  const int32_t* hp = c.node_hptr;
  const int32_t* ncl = c.node_cells;
  const int32_t* bp = c.node_bptr;
  const int32_t* bf = c.node_bfaces;
  int32_t* st = c.status;
  be_memset(st + 4, 0, sizeof(int32_t) * 3, s);
  // the patterns are replaced: values computed for the old ones must not be handed out against them
  for (int m = PFV_MAT_FLUX; m <= PFV_MAT_SYSTEM; ++m) c.filled[m] = false;
  c.have_symbolic = false;
  c.have_cmap = c.have_tpos_A = false;  // (flow_adjoint.inc: properties of the patterns replaced here)
  be_memset(st + 7, 0, sizeof(int32_t), s);
  Buf<int32_t> stage_ix;  // staging areas of the one-pass row builds (face rows, then the rows of A)
  Buf<uint8_t> stage_cp;

  Buf<int32_t> len;
  Buf<int64_t> ptr64;
  len.ensure(std::max(nf, nc) + 1);
  ptr64.ensure(std::max(nf, nc) + 1);
  int32_t* ln = len;

  const int maxfn = std::max(c.max_face_nodes, 1), maxdeg = std::max(c.max_deg, 1);
  // LDS per face: mask words | list offsets | gathered ids | merged ids (sorted distinct ids reuse the
  // gathered-id space) | rank of every element (bytes) | [column][node] -> element (bytes)
  const int cap_f = maxfn * std::max(maxdeg, std::max(c.max_bnd_per_node, 1));
  const int nw_f = cap_f / 64 + 1;
  const size_t lds_f = 8 * (size_t)nw_f + 4 * 20 + 8 * (size_t)cap_f + (size_t)cap_f + (size_t)cap_f * maxfn + 32;
  if (cap_f > 254) throw Error(PFV_ERR_UNSUPPORTED, "more than 254 (node, cell) pairs around one face");
  if (maxfn > 18) throw Error(PFV_ERR_UNSUPPORTED, "faces with more than 18 nodes");
  const int G_face = env_int("PFV_SYMB_G", 16);

  {  // patterns of the face matrices and the face records
  // faces that see a boundary face through one of their nodes (rows of bound_flux /
  // bound_pressure_face that are not empty): compact list, ascending
  Buf<int32_t> near_bnd;
  int64_t n_near = 0;
  {
    int32_t* flag = len.p;
    parallel_for(s, nf, PFV_LAMBDA(int64_t f) {
      int any = 0;
      for (int e = fn_ptr[f]; e < fn_ptr[f + 1]; ++e) {
        const int v = fn_idx[e];
        any |= (bp[v + 1] > bp[v]) ? 1 : 0;
      }
      flag[f] = any;
    });
    exclusive_scan<int32_t, int64_t>(s, c.scratch, len.p, ptr64.p, (size_t)nf);
    n_near = read_scalar<int64_t>(s, ptr64.p + nf);
    int32_t* lst = near_bnd.ensure(std::max<int64_t>(n_near, 1));
    const int64_t* pos = ptr64;
    parallel_for(s, nf, PFV_LAMBDA(int64_t f) {
      if (flag[f]) lst[pos[f]] = (int32_t)f;
    });
  }

  uint8_t* colpairs = nullptr;  // allocated once the flux pattern size is known (before its fill pass)
  // row f of flux / bound_pressure_cell = cells around the nodes of f;
  // row f of bound_flux / bound_pressure_face = boundary faces around the nodes of f.
  // pass 0 counts, pass 1 fills (cells: which = 0, boundary faces: which = 1)
  for (int which = 0; which < 2; ++which) {
    CsrPattern& P = which == 0 ? c.pat_flux : c.pat_bound;
    const int32_t* sub = which == 0 ? nullptr : near_bnd.p;
    const int64_t nitems = which == 0 ? nf : n_near;
    if (which == 1) be_memset(ln, 0, sizeof(int32_t) * (size_t)nf, s);
    // One pass when the rows fit a fixed-stride staging area (the union is the expensive part:
    // latency of dependent LDS searches): rows and column->pair maps go to the staging area together
    // with the count, a copy kernel compacts them once the row pointers are known.  Otherwise two
    // passes (count, fill).
    const int64_t SF = cap_f;
    const bool staged = which == 0 && env_int("PFV_SYMB_STAGED", 1) != 0 &&
                        (double)nf * (double)SF * (4.0 + maxfn) <= 6.0e9;
    int32_t* tix = nullptr;
    uint8_t* tcp = nullptr;
    if (staged) {
      tix = stage_ix.ensure((size_t)nf * SF);
      // the column -> pair maps stay where this pass leaves them: fixed stride per face (no compaction;
      // the face kernels address them by face)
      tcp = c.flux_colpairs.ensure((size_t)nf * SF * maxfn + 8);
      c.cp_stride = SF * maxfn;
      colpairs = tcp;
    } else if (which == 0) {
      c.cp_stride = 0;
    }
    // one lane per face (merge_lists_serial) whenever the 64 strips of a wavefront fit the LDS and a face has at
    // most 8 nodes; the cooperative kernel below is the general path (PFV_SYMB_SERIAL=0: A/B)
    const int kser = maxfn <= 3 ? 3 : (maxfn <= 4 ? 4 : (maxfn <= 8 ? 8 : 0));
    const bool serial = env_int("PFV_SYMB_SERIAL", 1) != 0 && kser != 0 &&
                        (env_int("PFV_SYMB_LDS", 1) == 0 || (size_t)64 * (cap_f | 1) * 4 <= 60 * 1024);
    for (int pass = 0; pass < (staged ? 1 : 2); ++pass) {
      const int32_t* ip = pass ? P.indptr.p : nullptr;
      int32_t* ix = pass ? P.indices.p : nullptr;
      if (serial) {
        int32_t* ids_base = ix ? ix : tix;  // null in the count pass of the two-pass form
        uint8_t* pairs_base = which == 0 ? (ix ? colpairs : tcp) : nullptr;
        int32_t* lnp = ix ? nullptr : ln;
        if (kser == 3) symbolic_face_rows_serial<3>(c, which, sub, nitems, cap_f, ip, SF, ids_base, pairs_base, lnp, st);
        else if (kser == 4) symbolic_face_rows_serial<4>(c, which, sub, nitems, cap_f, ip, SF, ids_base, pairs_base, lnp, st);
        else symbolic_face_rows_serial<8>(c, which, sub, nitems, cap_f, ip, SF, ids_base, pairs_base, lnp, st);
      } else
      wave_for_g(G_face, s, nitems, lds_f, PFV_LAMBDA(const WaveCtx& w) {
        const int64_t f = sub ? (int64_t)sub[w.item] : w.item;
        unsigned long long* mask = reinterpret_cast<unsigned long long*>(w.lds);
        int32_t* off = reinterpret_cast<int32_t*>(mask + nw_f);
        int32_t* buf = off + 20;
        int32_t* merged = buf + cap_f;
        int32_t* ures = buf;             // sorted distinct ids of the row (the gathered ids are dead by then)
        uint8_t* rankL = reinterpret_cast<uint8_t*>(merged + cap_f);  // rank of every gathered element
        uint8_t* pairL = rankL + cap_f;  // [column][node] -> element
        const int a = fn_ptr[f], nl = fn_ptr[f + 1] - a;
        int m = 0;
        for (int i = 0; i < nl; ++i) {
          const int v = fn_idx[a + i];
          const int32_t* src = which == 0 ? ncl + hp[v] / nd : bf + bp[v];
          const int n = which == 0 ? (hp[v + 1] - hp[v]) / nd : bp[v + 1] - bp[v];
          PFV_LANES(t, n) buf[m + t] = src[t];
          if (w.lane0()) off[i] = m;
          m += n;
        }
        if (w.lane0()) off[nl] = m;
        w.sync();
        const bool fill = ix != nullptr || tix != nullptr;
        const int cntv = merge_unique_lds(w, buf, off, nl, merged, mask, fill ? ures : nullptr,
                                          (fill && which == 0) ? rankL : nullptr);
        if (!ix) {
          if (w.lane0()) {
            ln[f] = cntv;
            track_max_i32(st + 5 + which, cntv);
          }
        }
        if (fill) {
          int32_t* row = ix ? ix + ip[f] : tix + f * SF;
          PFV_LANES(k, cntv) row[k] = ures[k];
          if (which == 0) {
            // for every column of the row, which (node of the face, cell of that node) pairs feed it:
            // the numeric face kernel then needs no searches.  Column of element e = number of run
            // heads up to its rank - 1 (popcount of the mask).
            PFV_LANES(x, cntv * maxfn) pairL[x] = 0xff;
            w.sync();
            PFV_LANES(e, m) {
              int li = 0;
              while (li + 1 < nl && e >= off[li + 1]) ++li;
              const int rk = rankL[e];
              int pos = popcount64(mask[rk >> 6] & (~0ull >> (63 - (rk & 63)))) - 1;
              for (int i = 0; i < (rk >> 6); ++i) pos += popcount64(mask[i]);
              pairL[pos * maxfn + li] = (uint8_t)e;
            }
            w.sync();
            uint8_t* dst = ix ? colpairs + (int64_t)ip[f] * maxfn : tcp + f * SF * maxfn;
            PFV_LANES(x, cntv * maxfn) dst[x] = pairL[x];
          }
        }
      });
      if (pass == 0) {
        exclusive_scan<int32_t, int64_t>(s, c.scratch, len.p, ptr64.p, (size_t)nf);
        finish_pattern(c, P, ptr64, nf, which == 0 ? nc : nf);
        if (which == 0 && !staged) colpairs = c.flux_colpairs.ensure((size_t)P.nnz * maxfn + 8);
      }
    }
    if (staged) {
      const int32_t* ip = P.indptr.p;
      int32_t* ix = P.indices.p;
      wave_for<16>(s, nf, 0, PFV_LAMBDA(const WaveCtx& w) {
        const int64_t f = w.item;
        const int p0 = ip[f], cntv = ip[f + 1] - p0;
        const int32_t* src = tix + f * SF;
        PFV_LANES(k, cntv) ix[p0 + k] = src[k];
      });
    }
  }

  // vector_source / bound_pressure_vector_source: every flux column c -> nd*c + k.  Row pointers now; the index array
  // (nd x the flux pattern, 2.6 GB at 2 M tetrahedra, a pure function of it) is written by ensure_vs_indices when the
  // first consumer asks for it: a matrix export or a product with one of the two matrices -- the discretization
  // itself and the system matrix never read it.  PFV_VS_INDICES_EAGER=1 fills it here (A/B, 1.3 ms).
  {
    // Beyond 2^31 entries (nd x 113 per face: ~6.3 M tetrahedra) neither the row pointers nor the indices fit the int32
    // of the CSR contract: the pattern then stays IMPLICIT in the flux pattern (c.vs_implicit) -- the face kernel addresses
    // the values by 64-bit nd * p + k anyway, products take spmv_vs_implicit, exports go by rows.  PFV_VS_IMPLICIT=1 forces
    // the implicit form at any size (tests).
    const int64_t nnz = c.pat_flux.nnz * nd;
    c.vs_implicit = nnz >= (int64_t(1) << 31) || env_int("PFV_VS_IMPLICIT", 0) != 0;
    c.pat_vs.nrows = nf;
    c.pat_vs.ncols = nc * nd;
    c.pat_vs.nnz = nnz;
    if (!c.vs_implicit) {
      c.pat_vs.indptr.ensure(nf + 1);
      const int32_t* ip = c.pat_flux.indptr;
      int32_t* vp = c.pat_vs.indptr;
      parallel_for(s, nf + 1, PFV_LAMBDA(int64_t f) { vp[f] = ip[f] * nd; });
      c.vs_indices_pending = true;
      if (env_int("PFV_VS_INDICES_EAGER", 0) != 0) ensure_vs_indices(c);
    } else {
      c.vs_indices_pending = false;
    }
  }

  int32_t sthf[3];
  be_d2h(sthf, st + 4, sizeof(sthf), s);
  if (sthf[1] > 256) throw Error(PFV_ERR_UNSUPPORTED, "more than 256 cells share a node with one face");
  c.pat_flux.max_row = sthf[1];
  c.pat_bound.max_row = sthf[2];
  c.pat_vs.max_row = sthf[1] * nd;
  {  // face records in processing order (pipelined face kernel)
    FaceRec* fr = c.face_rec.ensure(nf);
    const int32_t* order = c.face_order;
    const int32_t* ip = c.pat_flux.indptr;
    const int32_t* bip = c.pat_bound.indptr;
    parallel_for(s, nf, PFV_LAMBDA(int64_t i) {
      const int f = order[i];
      FaceRec r;
      r.f = f;
      r.a = fn_ptr[f];
      r.p0 = ip[f];
      r.q0 = bip[f];
      r.lens = (uint32_t)(ip[f + 1] - ip[f]) | ((uint32_t)(bip[f + 1] - bip[f]) << 16);  // (rows <= 256 / 65535 entries)
      r.nnf = (uint32_t)(fn_ptr[f + 1] - fn_ptr[f]);
      r.pad[0] = r.pad[1] = 0;
      fr[i] = r;
    });
  }
  }
  // A = div @ flux: row c = union of the flux rows of the faces of c = cells around the nodes of c
  {
    const int maxcf = std::max(c.max_cell_faces, 1);
    const int cap_n = maxcf * maxfn;   // gathered face nodes of a cell (lists = faces)
    const int cap_c = cap_n * maxdeg;  // gathered cells around its distinct nodes (upper bound)
    const int nw_c = cap_c / 64 + 1;
    const int noff = cap_n + 2;        // list offsets: at most cap_n lists in the second union
    const size_t lds_c = 8 * (size_t)nw_c + 4 * (size_t)noff + 4 * 3 * (size_t)cap_n + 8 * (size_t)cap_c + 64;
    if (lds_c > 150 * 1024) throw Error(PFV_ERR_UNSUPPORTED, "cell stencil too large for the symbolic phase");
    const int64_t SC = cap_c;
    const bool staged = env_int("PFV_SYMB_STAGED", 1) != 0 && (double)nc * (double)SC * 4.0 <= 6.0e9;
    int32_t* tax = staged ? stage_ix.ensure((size_t)nc * SC) : nullptr;
    for (int pass = 0; pass < (staged ? 1 : 2); ++pass) {
      const int32_t* ap = pass ? c.pat_A.indptr.p : nullptr;
      int32_t* ax = pass ? c.pat_A.indices.p : nullptr;
      auto cell_union = [=](auto epl1, auto epl2) {
        constexpr int E1 = decltype(epl1)::value, E2 = decltype(epl2)::value;
        wave_for_g(env_int("PFV_SYMB_CELL_G", 32), s, nc, lds_c, PFV_LAMBDA(const WaveCtx& w) {
        const int64_t cell = w.item;
        unsigned long long* mask = reinterpret_cast<unsigned long long*>(w.lds);
        int32_t* off = reinterpret_cast<int32_t*>(mask + nw_c);
        int32_t* nbuf = off + noff;     // face nodes, with duplicates
        int32_t* nmrg = nbuf + cap_n;   // merged face nodes
        int32_t* un = nmrg + cap_n;     // distinct nodes
        int32_t* cbuf = un + cap_n;     // cells around them
        int32_t* cmrg = cbuf + cap_c;
        const int e0 = cf_ptr[cell], nfc = cf_ptr[cell + 1] - e0;
        int m = 0;
        for (int i = 0; i < nfc; ++i) {
          const int f = cf_idx[e0 + i];
          const int a = fn_ptr[f], nl = fn_ptr[f + 1] - a;
          PFV_LANES(t, nl) nbuf[m + t] = fn_idx[a + t];
          if (w.lane0()) off[i] = m;
          m += nl;
        }
        if (w.lane0()) off[nfc] = m;
        w.sync();
        const int k1 = merge_unique_lds<uint8_t, E1>(w, nbuf, off, nfc, nmrg, mask, un);
        int m2 = 0;
        for (int i = 0; i < k1; ++i) {
          const int v = un[i];
          const int n = (hp[v + 1] - hp[v]) / nd;
          const int32_t* src = ncl + hp[v] / nd;
          PFV_LANES(t, n) cbuf[m2 + t] = src[t];
          if (w.lane0()) off[i] = m2;
          m2 += n;
        }
        if (w.lane0()) off[k1] = m2;
        w.sync();
        int32_t* dest = ax ? ax + ap[cell] : (tax ? tax + cell * SC : nullptr);
        const int cntv = merge_unique_lds<uint8_t, E2>(w, cbuf, off, k1, cmrg, mask, dest);
        if (!ax && w.lane0()) {
          ln[cell] = cntv;
          track_max_i32(st + 7, cntv);
        }
      });
      };
      // one lane per cell (merge_lists_serial over the cell lists of its <= K distinct nodes) when the strips fit
      // the LDS; a cell with more distinct nodes (general polyhedra) sends the whole pass to the cooperative kernel
      bool done = false;
      {
        const int kc = (maxfn <= 3 && maxcf <= 4) ? 4 : 8;  // simplices: 4 nodes per cell
        const bool fits = (size_t)64 * ((cap_n + kc) | 1) * 4 <= 60 * 1024;
        if (env_int("PFV_SYMB_SERIAL", 1) != 0 && fits) {
          be_memset(st + 14, 0, sizeof(int32_t), s);
          int32_t* ids_base = ax ? ax : tax;
          int32_t* lnp = ax ? nullptr : ln;
          if (kc == 4) symbolic_cell_rows_serial<4>(c, cap_n, maxdeg, ap, SC, ids_base, lnp, st);
          else symbolic_cell_rows_serial<8>(c, cap_n, maxdeg, ap, SC, ids_base, lnp, st);
          done = read_scalar<int32_t>(s, st + 14) == 0;
        }
      }
      if (!done) {
        using I1 = std::integral_constant<int, 1>;
        using I2 = std::integral_constant<int, 2>;
        using I4 = std::integral_constant<int, 4>;
        const int v = env_int("PFV_SYMB_CELL_EPL", 14);  // tens: first union (face nodes), units: second (cells)
        if (v == 11) cell_union(I1{}, I1{});
        else if (v == 14) cell_union(I1{}, I4{});
        else if (v == 44) cell_union(I4{}, I4{});
        else cell_union(I1{}, I2{});
      }
      if (pass == 0) {
        exclusive_scan<int32_t, int64_t>(s, c.scratch, len.p, ptr64.p, (size_t)nc);
        finish_pattern(c, c.pat_A, ptr64, nc, nc);
      }
    }
    if (staged) {
      const int32_t* ap = c.pat_A.indptr.p;
      int32_t* ax = c.pat_A.indices.p;
      wave_for<16>(s, nc, 0, PFV_LAMBDA(const WaveCtx& w) {
        const int64_t cell = w.item;
        const int p0 = ap[cell], cntv = ap[cell + 1] - p0;
        const int32_t* src = tax + cell * SC;
        PFV_LANES(k, cntv) ax[p0 + k] = src[k];
      });
    }
  }
  // checksum of A's pattern, read back with the sizes below (no extra synchronisation): what lets the next phases
  // prove that structures derived from the pattern alone (SpMV windows, AMG aggregate maps) still fit
  {
    const unsigned long long* cs = launch_pattern_checksum(c, c.csum_work, c.pat_A);
    parallel_for(s, 1, PFV_LAMBDA(int64_t) {
      st[8] = (int32_t)(unsigned)(*cs & 0xffffffffull);
      st[9] = (int32_t)(unsigned)(*cs >> 32);
    });
  }
  int32_t sth[3];
  be_d2h(sth, st + 7, sizeof(sth), s);
  c.pat_A_checksum = ((unsigned long long)(unsigned)sth[2] << 32) | (unsigned long long)(unsigned)sth[1];
  c.pat_A.max_row = sth[0];
  c.have_symbolic = true;
  c.symb_key = c.topo_key;  // (0 when the caller took no digest of the topology)
}

}  // namespace pfv
